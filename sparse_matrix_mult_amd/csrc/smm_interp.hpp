// smm_interp.hpp -- kernels of smm_interp_build: the observation operator H that interpolates a field on a rectilinear
// grid to n points, as a canonical CSR built on the device.  Host driver: smm_api.hip; the contract is in
// include/smm_hip.h.  The points (n x DIM) are row-major float64 with leading dimension ldp; every offset into them is
// 64-bit.  The axes are one array of doubles, axis t at [off[t], off[t] + m[t]).
//
// The contract in two functions, shared by both methods (so columns and values cannot disagree):
//   ip_cell   c = (number of nodes <= x) - 1 by a bounded binary search, clamped to [0, m - 2] BEFORE it addresses the
//             axis; f = (x - a[c]) / (a[c + 1] - a[c]), one IEEE subtraction each and one IEEE division; a coordinate
//             below the first node gives f = 0.0, one above the last gives f = 1.0 (SMM_INTERP_CLAMP; SMM_INTERP_ZERO
//             keeps these columns and stores +0.0; under SMM_INTERP_REJECT the host never launches the fill with such a
//             point).
//   ip_entry  entry e of a row: bit b_t of e (axis 0 the most significant) picks node c_t + b_t and the weight f_t or
//             1.0 - f_t; the value is ((w_0 * w_1) * w_2) * w_3, every product rounded.  SMM_INTERP_NEAREST is the
//             one-entry case: node c_t + (f_t > 0.5), value 1.0.
//
//   smm_interp_check  two integer counts, before the operand exists: coordinates that are NaN or +-inf, and points with
//                     finite coordinates of which one lies outside [first node, last node] (one integer atomic per wave).
//   smm_interp_fill   the three arrays.  Every row holds E = 2^DIM entries (NEAREST: 1) at the closed-form position
//                     i * E: no count pass, no scan, no atomics.  A lane takes four consecutive entries whose position in
//                     the output is a multiple of four and writes them as one 16-byte store of columns and two of values:
//                     at E = 2 it owns two rows, at E = 1 four, at E = 16 four lanes share a row (each repeats the row's
//                     DIM searches: a dozen LDS reads against 192 bytes written).  Only the last chunk of the arrays can
//                     be ragged (E < 4); it goes out entry by entry.  The row pointer is filled by the same launch.
//                     STAGE: the axes are copied to LDS once per workgroup (the grid is capped, workgroups stride over
//                     the chunks) and the searches read them there; otherwise they are read where they are, through L2.
// Always-on clamps, as in smm_kron.hpp: the cell index is clamped into the axis before any read, and a column outside
// [0, K) is recorded in the context's error word (SMM_ERR_INTERNAL for the caller) and stored as column 0 with value
// +0.0 -- never a fault.  No float atomics: two calls give the same bits.
#pragma once
#include "smm_kron.hpp"

#include <cfloat>

namespace smm {

constexpr int IP_MAX_DIM = 4;
constexpr int IP_STAGE_NODES = 4096;        // most nodes (all axes together) that smm_interp_fill stages in LDS: 32 KB
enum { IP_LINEAR = 0, IP_NEAREST = 1 };                   // SMM_INTERP_* of include/smm_hip.h
enum { IP_REJECT = 0, IP_CLAMP = 1, IP_ZERO = 2 };

struct InterpArgs {
    int m[IP_MAX_DIM], off[IP_MAX_DIM], stride[IP_MAX_DIM];     // nodes of axis t, its first node in `axes`, its column stride
    double lo[IP_MAX_DIM], hi[IP_MAX_DIM];                       // first and last node of axis t
    int nodes;                                                   // all axes together
    int K;                                                       // columns of H
    int outside;                                                 // IP_*
    int64_t n, ldp;
    const double *pts;
    const double *axes;
    int *optr; int *oidx; double *oval;
    unsigned long long *counts;                                  // smm_interp_check: [0] non-finite coordinates, [1] outside points
    unsigned *err;
};

// ------------------------------------------------------------------------------ non-finite and outside counts
template <int DIM>
__global__ __launch_bounds__(256) void smm_interp_check(const InterpArgs A)
{
    unsigned long long bad = 0, out = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * blockDim.x) {
        int b = 0, o = 0;
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
            const double x = A.pts[i * A.ldp + t];
            if (!(fabs(x) <= DBL_MAX)) ++b;
            else if (x < A.lo[t] || x > A.hi[t]) o = 1;
        }
        bad += (unsigned)b;
        if (b == 0) out += (unsigned)o;
    }
    for (int o = 1; o < WAVE; o <<= 1) {
        bad += __shfl_xor(bad, o);
        out += __shfl_xor(out, o);
    }
    if (lane_id() == 0) {
        if (bad) atomicAdd(A.counts, bad);
        if (out) atomicAdd(A.counts + 1, out);
    }
}

// ------------------------------------------------------------------------------ cell and fraction of one coordinate
// a: the axis (m >= 2 nodes, strictly ascending), in LDS or in global memory.  At most 31 steps: m < 2^31.
__device__ __forceinline__ void ip_cell(const double *a, int m, double lo, double hi, double x, int &c, double &f, bool &out)
{
    int b = 0, e = m;                                           // nodes [0, b) are <= x, nodes [e, m) are > x
    for (int s = 0; s < 31 && b < e; ++s) {
        int mid = b + ((e - b) >> 1);
        mid = mid < 0 ? 0 : (mid > m - 1 ? m - 1 : mid);        // (always inside: 0 <= b <= mid < e <= m)
        if (a[mid] <= x) b = mid + 1; else e = mid;
    }
    c = b - 1;
    c = c < 0 ? 0 : (c > m - 2 ? m - 2 : c);
    const double x0 = a[c], x1 = a[c + 1];
    f = (x - x0) / (x1 - x0);
    if (x < lo) { f = 0.0; out = true; }
    if (x > hi) { f = 1.0; out = true; }
}

// Cells, fractions and the outside flag of row i.
template <int DIM>
__device__ __forceinline__ void ip_row(const InterpArgs &A, const double *ax, int64_t i, int (&c)[IP_MAX_DIM], double (&f)[IP_MAX_DIM], bool &out)
{
    out = false;
#pragma unroll
    for (int t = 0; t < DIM; ++t) ip_cell(ax + A.off[t], A.m[t], A.lo[t], A.hi[t], A.pts[i * A.ldp + t], c[t], f[t], out);
}

// Entry e of a row (LINEAR: e < 2^DIM; NEAREST: e == 0).
template <int DIM, bool NEAREST>
__device__ __forceinline__ void ip_entry(const InterpArgs &A, const int (&c)[IP_MAX_DIM], const double (&f)[IP_MAX_DIM], bool zero, int e,
                                         int64_t row, int &col, double &val)
{
    col = 0;
    val = 1.0;
#pragma unroll
    for (int t = 0; t < DIM; ++t) {
        const bool up = NEAREST ? f[t] > 0.5 : ((e >> (DIM - 1 - t)) & 1) != 0;
        col += (c[t] + (up ? 1 : 0)) * A.stride[t];             // (<= K - 1 < 2^31 - 1: c[t] + 1 <= m[t] - 1)
        if (!NEAREST) {
            const double w = up ? f[t] : 1.0 - f[t];
            val = t == 0 ? w : val * w;                         // ((w_0 * w_1) * w_2) * w_3, every product rounded
        }
    }
    if (zero) val = 0.0;
    if (col < 0 || col >= A.K) { plan_err(A.err, PLAN_ERR_LIST, (int)row); col = 0; val = 0.0; }
}

// ------------------------------------------------------------------------------ fill
template <int DIM, bool NEAREST, bool STAGE>
__global__ __launch_bounds__(256) void smm_interp_fill(const InterpArgs A)
{
    constexpr int E = NEAREST ? 1 : (1 << DIM);                 // entries per row
    extern __shared__ __attribute__((aligned(16))) double ip_axes[];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
    const double *ax = A.axes;
    if (STAGE) {
        for (int q = threadIdx.x; q < A.nodes; q += blockDim.x) ip_axes[q] = A.axes[q];
        __syncthreads();
        ax = ip_axes;
    }
    for (int64_t i = tid; i <= A.n; i += nthreads) A.optr[i] = (int)(i * E);          // (n * E <= 2^31 - 2: checked by the host)
    const int64_t total = A.n * E;
    for (int64_t s = 4 * tid; s < total; s += 4 * nthreads) {
        const int u1 = (int)(total - s < 4 ? total - s : 4);
        int c[IP_MAX_DIM] = {0, 0, 0, 0}, col[4] = {0, 0, 0, 0};
        double f[IP_MAX_DIM] = {0.0, 0.0, 0.0, 0.0}, val[4] = {0.0, 0.0, 0.0, 0.0};
        bool out = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u >= u1) continue;
            const int64_t row = (s + u) / E;
            const int e = (int)((s + u) % E);
            if (u == 0 || e == 0) ip_row<DIM>(A, ax, row, c, f, out);         // (E >= 4: once per lane; E == 2: rows s/2, s/2 + 1)
            ip_entry<DIM, NEAREST>(A, c, f, out && A.outside == IP_ZERO, e, row, col[u], val[u]);
        }
        if (u1 == 4) {
            *reinterpret_cast<int4 *>(A.oidx + s) = make_int4(col[0], col[1], col[2], col[3]);
            *reinterpret_cast<double2 *>(A.oval + s) = make_double2(val[0], val[1]);
            *reinterpret_cast<double2 *>(A.oval + s + 2) = make_double2(val[2], val[3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < u1) { A.oidx[s + u] = col[u]; A.oval[s + u] = val[u]; }
        }
    }
}

}  // namespace smm
