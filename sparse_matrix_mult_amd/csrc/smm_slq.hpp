// smm_slq.hpp -- the device half of stochastic Lanczos quadrature for log det(H Q H^T + R): the +-1 probes
// (smm_probe_fill).  The other half is smm_cg.hpp's finish kernels with REC = true, which leave every column's alpha and
// beta in a history (smm_innovation_solve_coef); the tridiagonal work is the host's.  Host driver: smm_api.hip.
//
// X[i, c] depends on (seed, i, c) alone -- the hash is stated in include/smm_hip.h -- so neither k, ldx nor the launch
// geometry can change a probe.  No index comes from device data: rows and columns are arithmetic on the thread index.
#pragma once
#include "smm_cg.hpp"

namespace smm {

// +1.0, or -1.0 iff bit 63 of the mixed word is set (64-bit wrap-around arithmetic throughout)
__device__ __forceinline__ double slq_probe(unsigned long long seed, int64_t i, int64_t c)
{
    unsigned long long z = seed + (unsigned long long)c * 0xD1B54A32D192ED03ull + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (z >> 63) ? -1.0 : 1.0;
}

// One thread per row and group of VEC neighbouring columns (consecutive threads, consecutive addresses), grid-stride.
template <int VEC>
__global__ __launch_bounds__(256) void smm_probe_fill_k(int64_t n, int64_t k, unsigned long long seed, double *__restrict__ x, int64_t ldx)
{
    const int64_t kv = k / VEC, total = n * kv, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < total; f += step) {
        const int64_t i = f / kv, j = (f % kv) * VEC;
        CgVal<VEC> v;
#pragma unroll
        for (int u = 0; u < VEC; ++u) v.v[u] = slq_probe(seed, i, j + u);
        cg_store<VEC>(x + i * ldx + j, v);
    }
}

}  // namespace smm
