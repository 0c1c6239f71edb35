// smm_spmm.hpp -- kernels of the sparse x dense product Y = op(A) * X (smm_spmm, smm_triple_apply).  Host driver:
// smm_api.hip.  op(A) arrives as a CSR: A itself, or A^T as the cached transpose of A (smm_csr::trv).  X (K x k) and
// Y (m x k) are row-major float64 with leading dimensions ldx / ldy; every offset into them is 64-bit.
//
// Every nonzero A[i,p] gathers the row segment X[col_p, j0 .. j0 + width) -- a row gather.  Rows of op(A) are binned by
// their length (smm_spmm_bin, one atomic per wave and class) and each class has its kernel:
//   k == 1 (SpMV)   lanes take entries.  smm_spmv_group: groups of GS lanes per row (16 for short rows, four rows per
//                   wave; 64 otherwise).  smm_spmv_long: a long row split across the waves of a workgroup.
//   k > 1           lanes own output columns and keep Y[i, j] in registers.  smm_spmm_group: groups of G lanes per row
//                   (64 / G rows per wave), each lane VEC consecutive columns (16-byte loads of X when VEC == 2), column
//                   tiles of G * VEC cover any k; the row's (column, value) pairs are loaded by the group's lanes once
//                   per batch and broadcast.  smm_spmm_long: a long row split across the waves of a workgroup.
// Order of the sum:
//   SMM_EXACT  Y[i, j] starts at +0.0 and adds A[i,p] * X[col_p, j] for p in row i's stored order, one product at a
//              time, no fused multiply-add (the loop of scipy's csr_matvec / csr_matvecs).  The column-owning kernels
//              do exactly that per lane; the SpMV kernel adds the lane products of a batch one after another in
//              ascending lane order.  Long rows are walked by one wave.
//   default    fused multiply-adds; SpMV lanes keep partial sums that are combined by a butterfly in a fixed order, and
//              long rows are split across the waves of a workgroup, whose partial sums are added in LDS in wave order.
//              No float atomics in either mode: the result is bitwise reproducible from run to run.
// A pair that row i does not store is never multiplied, so an inf in X[c, :] reaches Y[i, :] only through A[i, c].
// Always-on clamps: a row-list entry outside [0, m), a row range outside [0, nnz) and a column outside [0, K) are
// recorded in the context's error word (SMM_ERR_INTERNAL for the caller) and skipped -- never a fault.
#pragma once
#include "smm_rowclass.hpp"

namespace smm {

enum { SP_TINY = 0, SP_GROUP = 1, SP_LONG = 2, SP_NCLS = 3 };
constexpr int SP_TINY_NNZ = 16;          // k == 1: rows of at most this many entries take 16 lanes (four rows per wave)
constexpr int SP_LONG_NNZ_VEC = 4096;    // k == 1: longer rows are split across the waves of a workgroup
constexpr int SP_LONG_NNZ_WIDE = 1024;   // k > 1: ditto
constexpr int SP_LONG_WAVES = 8;         // waves per workgroup of the long-row kernels

struct SpmmArgs {
    int m, K, nnz;                                                    // op(A): m x K with nnz entries
    const int *ptr; const int *idx; const double *val;
    int64_t k, ldx, ldy;
    const double *x; double *y;
    const int *rowlist; int nrows;                                    // rows of this class
    unsigned *err;
};

// Class of every row (mode 0: from nnz(row) and k; 1 / 2 / 3: every row in SP_TINY / SP_GROUP / SP_LONG) and the
// class lists lists[c * m ..], counts[c]: one atomic per wave and class.
__global__ __launch_bounds__(256) void smm_spmm_bin(int m, const int *__restrict__ ptr, int64_t k, int mode, int *__restrict__ lists,
                                                    int *__restrict__ counts)
{
    for (int r0 = blockIdx.x * blockDim.x; r0 < m; r0 += gridDim.x * blockDim.x) {     // (uniform over the block)
        const int r = r0 + (int)threadIdx.x;
        int b = -1;
        if (r < m) {
            const int len = ptr[r + 1] - ptr[r];
            if (mode > 0) b = mode - 1;
            else if (k == 1) b = len <= SP_TINY_NNZ ? SP_TINY : (len > SP_LONG_NNZ_VEC ? SP_LONG : SP_GROUP);
            else b = len > SP_LONG_NNZ_WIDE ? SP_LONG : SP_GROUP;
        }
        class_list_append(b, SP_NCLS, m, r, lists, counts);
    }
}

// Row li of the class list and its entry range, clamped: r = -1 for a list entry outside [0, m) (nothing is written).
__device__ __forceinline__ int sp_row(const SpmmArgs &A, int li, int &p0, int &p1)
{
    p0 = p1 = 0;
    const int r = A.rowlist[li];
    if (r < 0 || r >= A.m) { plan_err(A.err, PLAN_ERR_LIST, 0); return -1; }
    p0 = A.ptr[r]; p1 = A.ptr[r + 1];
    if (p0 < 0 || p1 < p0 || p1 > A.nnz) { plan_err(A.err, PLAN_ERR_COUNT, r); p0 = p1 = 0; }
    return r;
}
// Column of entry p, -1 (skipped) outside [0, K).
__device__ __forceinline__ int sp_col(const SpmmArgs &A, int p, int r)
{
    const int c = A.idx[p];
    if (c < 0 || c >= A.K) { plan_err(A.err, PLAN_ERR_LIST, r); return -1; }
    return c;
}

// Broadcast from lane src of the wave: readlane when src is wave-uniform, else a shuffle.
template <bool UNIFORM, typename T> __device__ __forceinline__ T sp_bcast(T v, int src)
{
    if constexpr (UNIFORM) return rl(v, src);
    else return __shfl(v, src);
}

// ------------------------------------------------------------------------------ k == 1
// Groups of GS lanes per row, 64 / GS rows per wave; the lanes of a group take consecutive entries of the row.
template <int GS, bool EXACT>
__global__ __launch_bounds__(256) void smm_spmv_group(const SpmmArgs A)
{
    constexpr int RPW = WAVE / GS;
    const int lane = lane_id(), gl = lane & (GS - 1), gbase = lane & ~(GS - 1);
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int)(gridDim.x * blockDim.x / WAVE);
    for (int li0 = wave * RPW; li0 < A.nrows; li0 += nwaves * RPW) {                 // (uniform over the wave)
        const int li = li0 + lane / GS;
        int p0 = 0, p1 = 0;
        const int r = li < A.nrows ? sp_row(A, li, p0, p1) : -1;
        const int len = p1 - p0;
        int wlen = len;                                               // longest row of the wave's groups
        for (int o = GS; o < WAVE; o <<= 1) wlen = max(wlen, __shfl_xor(wlen, o));
        double acc = 0.0;
        for (int b = 0; b < wlen; b += GS) {                          // (uniform over the wave)
            const int e = b + gl;
            double prod = 0.0;
            if (e < len) {
                const int c = sp_col(A, p0 + e, r);
                if (c >= 0) {
                    if constexpr (EXACT) prod = A.val[p0 + e] * A.x[(int64_t)c * A.ldx];
                    else acc = fma(A.val[p0 + e], A.x[(int64_t)c * A.ldx], acc);
                }
            }
            if constexpr (EXACT) {                                    // the batch's products one after another, ascending lanes
                const int n = len - b;
#pragma unroll 8
                for (int l = 0; l < GS; ++l) {
                    const double s = sp_bcast<GS == WAVE>(prod, gbase + l);
                    if (l < n) acc = acc + s;
                }
            }
        }
        if constexpr (!EXACT)
            for (int o = GS / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (gl == 0 && r >= 0) A.y[(int64_t)r * A.ldy] = acc;
    }
}

// Default mode, long rows: wave w of the workgroup takes the w-th contiguous share of the row; the waves' partial sums
// are added in LDS in wave order.
template <int NW>
__global__ __launch_bounds__(NW * WAVE) void smm_spmv_long(const SpmmArgs A)
{
    __shared__ double part[NW];
    const int lane = lane_id(), w = (int)(threadIdx.x / WAVE);
    for (int li = blockIdx.x; li < A.nrows; li += gridDim.x) {                       // (uniform over the block)
        int p0 = 0, p1 = 0;
        const int r = sp_row(A, li, p0, p1);
        const int64_t len = p1 - p0;
        const int q0 = p0 + (int)(len * w / NW), q1 = p0 + (int)(len * (w + 1) / NW);
        double acc = 0.0;
#pragma unroll 4
        for (int p = q0 + lane; p < q1; p += WAVE) {
            const int c = sp_col(A, p, r);
            if (c >= 0) acc = fma(A.val[p], A.x[(int64_t)c * A.ldx], acc);
        }
        for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) part[w] = acc;
        __syncthreads();
        if (threadIdx.x == 0 && r >= 0) {
            double s = part[0];
            for (int v = 1; v < NW; ++v) s += part[v];
            A.y[(int64_t)r * A.ldy] = s;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------ k > 1
// acc[0 .. VEC) += a * X[c, j .. j + VEC): one 16-byte load for VEC == 2 (host: k, ldx, ldy even, X and Y 16-byte aligned)
template <int VEC, bool EXACT>
__device__ __forceinline__ void sp_axpy(double (&acc)[VEC], double a, const double *xp)
{
    if constexpr (VEC == 2) {
        const double2 xv = *reinterpret_cast<const double2 *>(xp);
        if constexpr (EXACT) { acc[0] = acc[0] + a * xv.x; acc[1] = acc[1] + a * xv.y; }
        else { acc[0] = fma(a, xv.x, acc[0]); acc[1] = fma(a, xv.y, acc[1]); }
    } else {
        if constexpr (EXACT) acc[0] = acc[0] + a * xp[0];
        else acc[0] = fma(a, xp[0], acc[0]);
    }
}
template <int VEC> __device__ __forceinline__ void sp_store(double *yp, const double (&acc)[VEC])
{
    if constexpr (VEC == 2) *reinterpret_cast<double2 *>(yp) = make_double2(acc[0], acc[1]);
    else yp[0] = acc[0];
}

// Groups of G lanes per row, 64 / G rows per wave; lane gl of a group owns columns j0 + gl * VEC .. + VEC of the column
// tile j0 (tiles of G * VEC columns).  Per batch the group's lanes load G consecutive (column, value) pairs of the row,
// and every pair is broadcast to the group in stored order: each lane adds its products in that order.
template <int G, int VEC, bool EXACT>
__global__ __launch_bounds__(256) void smm_spmm_group(const SpmmArgs A)
{
    constexpr int RPW = WAVE / G, TW = G * VEC;
    const int lane = lane_id(), gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int)(gridDim.x * blockDim.x / WAVE);
    for (int li0 = wave * RPW; li0 < A.nrows; li0 += nwaves * RPW) {                 // (uniform over the wave)
        const int li = li0 + lane / G;
        int p0 = 0, p1 = 0;
        const int r = li < A.nrows ? sp_row(A, li, p0, p1) : -1;
        const int len = p1 - p0;
        int wlen = len;
        for (int o = G; o < WAVE; o <<= 1) wlen = max(wlen, __shfl_xor(wlen, o));
        for (int64_t j0 = 0; j0 < A.k; j0 += TW) {                                   // (uniform over the wave)
            const int64_t j = j0 + (int64_t)gl * VEC;
            const bool own = r >= 0 && j < A.k;                       // (VEC divides k)
            double acc[VEC];
#pragma unroll
            for (int u = 0; u < VEC; ++u) acc[u] = 0.0;
            for (int b = 0; b < wlen; b += G) {                       // (uniform over the wave)
                const int e = b + gl;
                int c = -1;
                double v = 0.0;
                if (e < len) { c = sp_col(A, p0 + e, r); v = A.val[p0 + e]; }
#pragma unroll 8
                for (int l = 0; l < G; ++l) {
                    const int cl = sp_bcast<G == WAVE>(c, gbase + l);
                    const double vl = sp_bcast<G == WAVE>(v, gbase + l);
                    if (cl >= 0 && own) sp_axpy<VEC, EXACT>(acc, vl, A.x + (int64_t)cl * A.ldx + j);
                }
            }
            if (own) sp_store<VEC>(A.y + (int64_t)r * A.ldy + j, acc);
        }
    }
}

// Default mode, long rows: one workgroup per (row, column tile of 64 * VEC); wave w takes the w-th contiguous share of
// the row, lanes own columns, and the waves' partial sums are added in LDS in wave order.
template <int VEC, int NW>
__global__ __launch_bounds__(NW * WAVE) void smm_spmm_long(const SpmmArgs A, int ntiles)
{
    constexpr int TW = WAVE * VEC;
    __shared__ double part[NW][TW];
    const int lane = lane_id(), w = (int)(threadIdx.x / WAVE);
    const int64_t items = (int64_t)A.nrows * ntiles;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {                      // (uniform over the block)
        const int li = (int)(it / ntiles), tile = (int)(it % ntiles);
        int p0 = 0, p1 = 0;
        const int r = sp_row(A, li, p0, p1);
        const int64_t len = p1 - p0;
        const int q0 = p0 + (int)(len * w / NW), q1 = p0 + (int)(len * (w + 1) / NW);
        const int64_t j = (int64_t)tile * TW + (int64_t)lane * VEC;
        const bool own = j < A.k;
        double acc[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) acc[u] = 0.0;
        for (int b = q0; b < q1; b += WAVE) {                         // (uniform over the wave)
            const int e = b + lane;
            int c = -1;
            double v = 0.0;
            if (e < q1) { c = sp_col(A, e, r); v = A.val[e]; }
            const int n = min(WAVE, q1 - b);
            for (int l = 0; l < n; ++l) {
                const int cl = rl(c, l);
                const double vl = rl(v, l);
                if (cl >= 0 && own) sp_axpy<VEC, false>(acc, vl, A.x + (int64_t)cl * A.ldx + j);
            }
        }
#pragma unroll
        for (int u = 0; u < VEC; ++u) part[w][lane * VEC + u] = acc[u];
        __syncthreads();
        if (w == 0 && own && r >= 0) {
            double s[VEC];
#pragma unroll
            for (int u = 0; u < VEC; ++u) s[u] = part[0][lane * VEC + u];
            for (int v = 1; v < NW; ++v)
#pragma unroll
                for (int u = 0; u < VEC; ++u) s[u] += part[v][lane * VEC + u];
            sp_store<VEC>(A.y + (int64_t)r * A.ldy + j, s);
        }
        __syncthreads();
    }
}

}  // namespace smm
