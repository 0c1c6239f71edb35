// smm_cg.hpp -- vector kernels of the conjugate-gradient solve (S + R) Z = D with S = H Q H^T (smm_innovation_solve).
// Host driver: smm_api.hip.  The sparse x dense products of an iteration are the kernels of smm_spmm.hpp, launched from
// class lists that are binned once per column block; this file holds what runs between them.
//
// Every vector is a row-major n x k block (k right-hand sides, each its own CG).  One thread owns partial t of VEC
// neighbouring columns and walks the rows i = t, t + T, t + 2T, ... (T = SMM_CG_LANES): consecutive threads touch
// consecutive addresses, and a kernel that updates vectors leaves the T partial sums of the dot product it feeds in
// part[t * k + j] on the way.  The finish kernels (one workgroup per column) combine the partials by the tree
// s[t] = s[t] + s[t + h], h = T/2 .. 1, and do the scalar work of the column: alpha, beta, the convergence and
// breakdown tests, the count of live columns.  The order of every sum is fixed -- no float atomics, and under SMM_EXACT
// every multiply is rounded before its add (the Makefile builds with -ffp-contract=off; default mode asks for fma).
//
// Per-column scalars sc[6 * k]: rho, alpha, beta, thr, rhs_sq, res_sq.  Per-column state st[3 * k + 1]: status, iterations,
// frozen, and the count of live columns.  A frozen column is never written again by any kernel here.
// No index in this file comes from device data: rows and columns are arithmetic on the launch geometry.
#pragma once
#include "smm_spmm.hpp"
#include "../../include/smm_hip.h"

namespace smm {

constexpr int CG_T = SMM_CG_LANES;
constexpr int CG_FIN = CG_T / 2;                 // threads of a finish workgroup: the tree's first step reads HBM
static_assert(CG_T == 2048 && (CG_T & (CG_T - 1)) == 0, "the finish kernels are written for T = 2048");
enum { CG_RHO = 0, CG_ALPHA = 1, CG_BETA = 2, CG_THR = 3, CG_RHS = 4, CG_RES = 5, CG_NSC = 6 };
enum { CG_CONVERGED = 0, CG_LIMIT = 1, CG_BREAKDOWN = 2 };

struct CgArgs {
    int64_t n, k;
    const double *b; int64_t ldb;                // right-hand sides
    double *x; int64_t ldx;                      // solution
    double *r, *p, *w; const double *rp;         // n x k, packed: residual, direction, (S + R) p, R p
    double *part;                                // T x k partial sums
    double *sc; int *st;
};

template <int VEC> struct CgVal { double v[VEC]; };
template <int VEC> __device__ __forceinline__ CgVal<VEC> cg_load(const double *p)
{
    CgVal<VEC> o;
    if constexpr (VEC == 2) { const double2 t = *reinterpret_cast<const double2 *>(p); o.v[0] = t.x; o.v[1] = t.y; }
    else o.v[0] = p[0];
    return o;
}
template <int VEC> __device__ __forceinline__ void cg_store(double *p, const CgVal<VEC> &a)
{
    if constexpr (VEC == 2) *reinterpret_cast<double2 *>(p) = make_double2(a.v[0], a.v[1]);
    else p[0] = a.v[0];
}
// acc + a * b: the product rounded first under SMM_EXACT, fused otherwise
template <bool EXACT> __device__ __forceinline__ double cg_mad(double a, double b, double acc)
{
    if constexpr (EXACT) return acc + a * b;
    else return fma(a, b, acc);
}
// Partial t and first column j of this thread; false past the last (t, column group).
template <int VEC> __device__ __forceinline__ bool cg_thread(const CgArgs &A, int64_t &t, int64_t &j)
{
    const int64_t kv = A.k / VEC, f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    t = f / kv; j = (f % kv) * VEC;
    return t < CG_T;
}

// r = p = d, x = 0, partials of dot(r, r)
template <int VEC, bool EXACT>
__global__ __launch_bounds__(256) void smm_cg_init(const CgArgs A)
{
    int64_t t, j;
    if (!cg_thread<VEC>(A, t, j)) return;
    CgVal<VEC> acc, zero;
#pragma unroll
    for (int u = 0; u < VEC; ++u) acc.v[u] = zero.v[u] = 0.0;
#pragma unroll 4
    for (int64_t i = t; i < A.n; i += CG_T) {
        const CgVal<VEC> d = cg_load<VEC>(A.b + i * A.ldb + j);
        cg_store<VEC>(A.r + i * A.k + j, d);
        cg_store<VEC>(A.p + i * A.k + j, d);
        cg_store<VEC>(A.x + i * A.ldx + j, zero);
#pragma unroll
        for (int u = 0; u < VEC; ++u) acc.v[u] = cg_mad<EXACT>(d.v[u], d.v[u], acc.v[u]);
    }
    cg_store<VEC>(A.part + t * A.k + j, acc);
}

// w = w + R p (one add per element), partials of dot(p, w)
template <int VEC, bool EXACT, bool HAS_R>
__global__ __launch_bounds__(256) void smm_cg_pw(const CgArgs A)
{
    int64_t t, j;
    if (!cg_thread<VEC>(A, t, j)) return;
    CgVal<VEC> acc;
#pragma unroll
    for (int u = 0; u < VEC; ++u) acc.v[u] = 0.0;
#pragma unroll 4
    for (int64_t i = t; i < A.n; i += CG_T) {
        const int64_t o = i * A.k + j;
        const CgVal<VEC> p = cg_load<VEC>(A.p + o);
        CgVal<VEC> w = cg_load<VEC>(A.w + o);
        if constexpr (HAS_R) {
            const CgVal<VEC> rp = cg_load<VEC>(A.rp + o);
#pragma unroll
            for (int u = 0; u < VEC; ++u) w.v[u] = w.v[u] + rp.v[u];
            cg_store<VEC>(A.w + o, w);
        }
#pragma unroll
        for (int u = 0; u < VEC; ++u) acc.v[u] = cg_mad<EXACT>(p.v[u], w.v[u], acc.v[u]);
    }
    cg_store<VEC>(A.part + t * A.k + j, acc);
}

// live columns: x = x + alpha p, r = r - alpha w, partials of dot(r, r)
template <int VEC, bool EXACT>
__global__ __launch_bounds__(256) void smm_cg_update(const CgArgs A)
{
    int64_t t, j;
    if (!cg_thread<VEC>(A, t, j)) return;
    CgVal<VEC> acc;
    double al[VEC];
    bool live[VEC], any = false;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
        acc.v[u] = 0.0;
        live[u] = A.st[2 * A.k + j + u] == 0;
        al[u] = A.sc[CG_ALPHA * A.k + j + u];
        any = any || live[u];
    }
    if (any) {
#pragma unroll 4
        for (int64_t i = t; i < A.n; i += CG_T) {
            const int64_t o = i * A.k + j;
            const CgVal<VEC> p = cg_load<VEC>(A.p + o), w = cg_load<VEC>(A.w + o);
            CgVal<VEC> r = cg_load<VEC>(A.r + o), x = cg_load<VEC>(A.x + i * A.ldx + j);
#pragma unroll
            for (int u = 0; u < VEC; ++u) {
                if (!live[u]) continue;
                x.v[u] = cg_mad<EXACT>(al[u], p.v[u], x.v[u]);
                if constexpr (EXACT) r.v[u] = r.v[u] - al[u] * w.v[u];
                else r.v[u] = fma(-al[u], w.v[u], r.v[u]);
                acc.v[u] = cg_mad<EXACT>(r.v[u], r.v[u], acc.v[u]);
            }
            cg_store<VEC>(A.r + o, r);                    // (a frozen column of the pair gets its own bits back)
            cg_store<VEC>(A.x + i * A.ldx + j, x);
        }
    }
    cg_store<VEC>(A.part + t * A.k + j, acc);
}

// live columns: p = r + beta p
template <int VEC, bool EXACT>
__global__ __launch_bounds__(256) void smm_cg_direction(const CgArgs A)
{
    int64_t t, j;
    if (!cg_thread<VEC>(A, t, j)) return;
    double be[VEC];
    bool live[VEC], any = false;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
        live[u] = A.st[2 * A.k + j + u] == 0;
        be[u] = A.sc[CG_BETA * A.k + j + u];
        any = any || live[u];
    }
    if (!any) return;
#pragma unroll 4
    for (int64_t i = t; i < A.n; i += CG_T) {
        const int64_t o = i * A.k + j;
        const CgVal<VEC> r = cg_load<VEC>(A.r + o);
        CgVal<VEC> p = cg_load<VEC>(A.p + o);
#pragma unroll
        for (int u = 0; u < VEC; ++u)
            if (live[u]) p.v[u] = cg_mad<EXACT>(be[u], p.v[u], r.v[u]);
        cg_store<VEC>(A.p + o, p);
    }
}

// One workgroup per column: the tree over the T partials, then the column's scalar step.
//   STEP 0 (after smm_cg_init)    rho = rhs_sq = res_sq = s, thr = tol2 * s; frozen at once when rho <= thr
//   STEP 1 (after smm_cg_pw)      pw = s; not (pw > 0): breakdown, else alpha = rho / pw
//   STEP 2 (after smm_cg_update)  rho_new = s; rho_new <= thr: converged, else beta = rho_new / rho, rho = rho_new
// REC (smm_innovation_solve_coef): hist is the block's maxiter x k history of alpha (STEP 1) or beta (STEP 2), zeroed by the
// host; row it - 1 gets the coefficient where the column computes one.  Without REC hist is never read (NULL) and the
// kernels are the code they were before the history existed.
template <int STEP, bool REC = false>
__global__ __launch_bounds__(CG_FIN) void smm_cg_finish(const double *__restrict__ part, int64_t k, double *__restrict__ sc, int *__restrict__ st,
                                                        double tol2, int it, double *__restrict__ hist)
{
    __shared__ double s[CG_FIN];
    const int64_t j = blockIdx.x;
    const int tid = (int)threadIdx.x;
    s[tid] = part[(int64_t)tid * k + j] + part[(int64_t)(tid + CG_FIN) * k + j];
    __syncthreads();
    for (int h = CG_FIN / 2; h > 0; h >>= 1) {
        if (tid < h) s[tid] = s[tid] + s[tid + h];
        __syncthreads();
    }
    if (tid != 0) return;
    const double sum = s[0];
    int *status = st, *iters = st + k, *frozen = st + 2 * k, *live = st + 3 * k;
    if constexpr (STEP == 0) {
        const double thr = tol2 * sum;
        sc[CG_RHO * k + j] = sum; sc[CG_RHS * k + j] = sum; sc[CG_RES * k + j] = sum; sc[CG_THR * k + j] = thr;
        sc[CG_ALPHA * k + j] = 0.0; sc[CG_BETA * k + j] = 0.0;
        iters[j] = 0;
        if (sum <= thr) { status[j] = CG_CONVERGED; frozen[j] = 1; }
        else { status[j] = CG_LIMIT; frozen[j] = 0; atomicAdd(live, 1); }
    } else {
        if (frozen[j]) return;
        if constexpr (STEP == 1) {
            if (!(sum > 0.0)) { status[j] = CG_BREAKDOWN; frozen[j] = 1; iters[j] = it - 1; atomicSub(live, 1); }
            else {
                const double alpha = sc[CG_RHO * k + j] / sum;
                sc[CG_ALPHA * k + j] = alpha;
                if constexpr (REC) hist[(int64_t)(it - 1) * k + j] = alpha;
            }
        } else {
            sc[CG_RES * k + j] = sum;
            iters[j] = it;
            if (sum <= sc[CG_THR * k + j]) { status[j] = CG_CONVERGED; frozen[j] = 1; atomicSub(live, 1); }
            else {
                const double beta = sum / sc[CG_RHO * k + j];
                sc[CG_BETA * k + j] = beta; sc[CG_RHO * k + j] = sum;
                if constexpr (REC) hist[(int64_t)(it - 1) * k + j] = beta;
            }
        }
    }
}

}  // namespace smm
