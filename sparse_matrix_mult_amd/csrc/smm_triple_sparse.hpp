// smm_triple_sparse.hpp -- kernels of the device CSR transpose (smm_csr_transpose) and of the sparse-output triple
// product H * Q * H^T (smm_triple_product_sparse).  Host driver: smm_api.hip.
//
//   transpose      count per column -> smm_scan -> scatter of source positions (atomics: arrival order) -> segmented
//                  sort of every output row by source position -> gather of (source row, value).  Source positions
//                  are distinct and ascending in (row, slot) order, so the sorted rows are exactly scipy's tocsc().
//   triple, per row block of H:
//                  T_b = H[b] * Q (smm_spgemm_*), S_b's pattern = T_b * pattern(H^T) with the triangle filter
//                  (smm_spgemm_* with SMM_SYMMETRIC), rows sorted ascending (segmented sort), then the values:
//                  S[i,k] = sum over H_k in stored order of T[i, H.col] * H.val -- the reference's loop
//                  (sparse_sparse_dense.cpp:201-211), T_i looked up in an LDS hash (wave / workgroup per row) or a
//                  zeroed global row of K doubles (rows whose T_i exceeds LDS).
#pragma once
#include "smm_rowclass.hpp"

namespace smm {

// ------------------------------------------------------------------------------ segmented sort of distinct int keys
// Segment s is key[off[s] .. off[s+1]).  Three lengths: <= SEG_SHORT (one thread, insertion sort), <= SEG_LDS (one
// workgroup, bitonic in LDS), longer (one workgroup, bitonic in global memory).  The bitonic network is the
// all-ascending ("flip") form: padding the length to a power of two with +inf never moves a real key, so positions
// past the segment are simply skipped.
constexpr int SEG_SHORT = 32;
constexpr int SEG_LDS = 8192;

__device__ __forceinline__ void seg_cmpswap(int *k, int64_t lo, int64_t hi, int64_t len)
{
    if (hi < len) {
        const int a = k[lo], b = k[hi];
        if (a > b) { k[lo] = b; k[hi] = a; }
    }
}
// Sorts k[0, len) with all threads of the workgroup (k in LDS or global memory); P = len rounded up to a power of two.
__device__ void seg_bitonic(int *k, int64_t len)
{
    int64_t P = 1;
    while (P < len) P <<= 1;
    for (int64_t sz = 2; sz <= P; sz <<= 1) {
        const int64_t half = sz >> 1;
        for (int64_t i = threadIdx.x; i < P / 2; i += blockDim.x) {
            const int64_t blk = i / half, o = i % half;
            seg_cmpswap(k, blk * sz + o, blk * sz + sz - 1 - o, len);
        }
        __syncthreads();
        for (int64_t j = half >> 1; j >= 1; j >>= 1) {
            for (int64_t i = threadIdx.x; i < P / 2; i += blockDim.x) {
                const int64_t lo = (i / j) * 2 * j + i % j;
                seg_cmpswap(k, lo, lo + j, len);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void smm_seg_sort_short(int64_t nseg, const int64_t *__restrict__ off, int *__restrict__ key)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = off[s], len = off[s + 1] - b;
        if (len < 2 || len > SEG_SHORT) continue;
        int *k = key + b;
        for (int i = 1; i < (int)len; ++i) {
            const int x = k[i];
            int j = i - 1;
            while (j >= 0 && k[j] > x) { k[j + 1] = k[j]; --j; }
            k[j + 1] = x;
        }
    }
}

// LONG = false: SEG_SHORT < len <= SEG_LDS, sorted in LDS;  LONG = true: len > SEG_LDS, sorted in place in global memory.
template <bool LONG>
__global__ __launch_bounds__(1024) void smm_seg_sort(int64_t nseg, const int64_t *__restrict__ off, int *__restrict__ key)
{
    __shared__ int sk[LONG ? 1 : SEG_LDS];
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t b = off[s], len = off[s + 1] - b;
        if (LONG ? len <= SEG_LDS : (len <= SEG_SHORT || len > SEG_LDS)) continue;        // (uniform over the block)
        if constexpr (LONG) {
            seg_bitonic(key + b, len);
        } else {
            for (int64_t i = threadIdx.x; i < len; i += blockDim.x) sk[i] = key[b + i];
            __syncthreads();
            seg_bitonic(sk, len);
            for (int64_t i = threadIdx.x; i < len; i += blockDim.x) key[b + i] = sk[i];
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------ transpose
__global__ __launch_bounds__(256) void smm_transpose_count(int64_t nnz, const int *__restrict__ idx, int cols, int *__restrict__ cnt)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int j = idx[p];
        if (j >= 0 && j < cols) atomicAdd(&cnt[j], 1);          // (validated operand: always true)
    }
}
__global__ __launch_bounds__(256) void smm_transpose_scatter(int64_t nnz, const int *__restrict__ idx, int cols, const int64_t *__restrict__ off,
                                                             int *__restrict__ cursor, int *__restrict__ key)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int j = idx[p];
        if (j < 0 || j >= cols) continue;
        const int slot = atomicAdd(&cursor[j], 1);
        const int64_t q = off[j] + slot;
        if (q < off[j + 1]) key[q] = (int)p;
    }
}
// key[q] (sorted source positions) -> source row (binary search in A's indptr) and value; also the int32 row pointer
__global__ __launch_bounds__(256) void smm_transpose_gather(int64_t nnz, int rows, const int *__restrict__ a_ptr, const double *__restrict__ a_val,
                                                            const int *__restrict__ key, int cols, const int64_t *__restrict__ off,
                                                            int *__restrict__ t_ptr, int *__restrict__ t_idx, double *__restrict__ t_val)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = tid; j <= cols; j += stride) t_ptr[j] = (int)off[j];
    for (int64_t q = tid; q < nnz; q += stride) {
        int p = key[q];
        p = p < 0 ? 0 : (p >= nnz ? (int)nnz - 1 : p);
        int lo = 0, hi = rows;                                 // last row r with a_ptr[r] <= p
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a_ptr[mid] <= p) lo = mid; else hi = mid;
        }
        t_idx[q] = lo;
        t_val[q] = a_val[p];
    }
}

// ------------------------------------------------------------------------------ triple product, sparse output
__global__ __launch_bounds__(256) void smm_triple_sparse_narrow(int64_t n, const int64_t *__restrict__ src, int *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (int)src[i];
}
__global__ __launch_bounds__(256) void smm_triple_sparse_rebase(int64_t n, const int64_t *__restrict__ src, int64_t base, int64_t *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i] + base;
}

// Rows of the block with a non-empty row of S, by the length of T_i: lists[0..m) wave hash, [m..2m) workgroup hash,
// [2m..3m) global row.  counts[0..2].  One atomic per wave and class (almost every row of a local H falls into one
// class: per-row atomics on one counter cost 2.3 ms at 200 000 rows).
__global__ __launch_bounds__(256) void smm_triple_sparse_bin(int m, const int64_t *__restrict__ t_ptr, const int64_t *__restrict__ s_ptr,
                                                             int *__restrict__ lists, int *__restrict__ counts)
{
    for (int r0 = blockIdx.x * blockDim.x; r0 < m; r0 += gridDim.x * blockDim.x) {     // (uniform over the block)
        const int r = r0 + (int)threadIdx.x;
        int b = -1;
        if (r < m && s_ptr[r + 1] != s_ptr[r]) {
            const int64_t len = t_ptr[r + 1] - t_ptr[r];
            b = len <= WaveHash::MAX ? 0 : (len <= WgHash::MAX ? 1 : 2);
        }
        class_list_append(b, 3, m, r, lists, counts);
    }
}

struct Triple3Args {
    int m;                              // rows of the block
    int64_t row0;                       // global index of the block's row 0 (for the error word only)
    const int *rowlist; int nrows;      // rows of this class
    const int64_t *t_ptr; const int *t_idx; const double *t_val;      // T_b (columns distinct)
    const int64_t *s_ptr; const int *s_idx; double *s_val;            // S_b: pattern in, values out
    const int *h_ptr; const int *h_idx; const double *h_val; int n; int K;
    double *dense;                      // global path: one zeroed row of K doubles per workgroup
    unsigned *err;
};

// S[i,k] for the k of row i: lanes take consecutive k, each walks H_k in stored order.  look(col) -> T[i,col] or +0.0.
template <bool FMA, typename Look>
__device__ __forceinline__ void t3_row_values(const Triple3Args &A, int r, int t, int nt, Look look)
{
    const int64_t s0 = A.s_ptr[r], s1 = A.s_ptr[r + 1];
    for (int64_t kp = s0 + t; kp < s1; kp += nt) {
        int k = A.s_idx[kp];
        if (k < 0 || k >= A.n) { plan_err(A.err, PLAN_ERR_LIST, (int)(A.row0 + r)); k = 0; }
        const int e = A.h_ptr[k + 1];
        double sum = 0.0;
        for (int jp = A.h_ptr[k]; jp < e; ++jp) {
            const double x = look(A.h_idx[jp]), hv = A.h_val[jp];
            sum = FMA ? __builtin_fma(x, hv, sum) : sum + x * hv;     // (-ffp-contract=off: no fused multiply-add here)
        }
        A.s_val[kp] = sum;
    }
}

// LDS hash of T_i: HS slots per row group of TPR threads, RPB row groups per workgroup; dynamic LDS t3_hash_lds<H>().
template <int HS, int BITS, int TPR, int RPB, bool FMA>
__global__ __launch_bounds__(TPR * RPB) void smm_triple_sparse_s2_hash(const Triple3Args A)
{
    extern __shared__ double t3_lds[];
    const int g = threadIdx.x / TPR, t = threadIdx.x % TPR;
    double *hv = t3_lds + (size_t)g * HS;
    const LdsHash<HS, BITS> h{(int *)(t3_lds + (size_t)RPB * HS) + (size_t)g * HS};
    for (int base = blockIdx.x * RPB; base < A.nrows; base += gridDim.x * RPB) {     // (uniform over the block)
        const int li = base + g;
        const bool have = li < A.nrows;
        int r = have ? A.rowlist[li] : 0;
        if (r < 0 || r >= A.m) { plan_err(A.err, PLAN_ERR_LIST, 0); r = 0; }
        h.clear(t, TPR);
        __syncthreads();
        const int64_t t0 = A.t_ptr[r];
        int64_t tl = A.t_ptr[r + 1] - t0;
        if (tl > HS / 2) { if (have && t == 0) plan_err(A.err, PLAN_ERR_HASH, (int)(A.row0 + r)); tl = HS / 2; }
        if (have) {
            for (int64_t e = t; e < tl; e += TPR) {
                const int s = h.insert(A.t_idx[t0 + e]);
                if (s >= 0) hv[s] = A.t_val[t0 + e];
            }
        }
        __syncthreads();
        if (have)
            t3_row_values<FMA>(A, r, t, TPR, [&](int col) { return h.find(col, 0.0, [&](int s) { return hv[s]; }); });
        __syncthreads();
    }
}
// Its instance for hash class H and its dynamic LDS: the values of the RPB rows (HS doubles each), then their keys.
template <class H, bool FMA> constexpr auto t3_hash_kernel = smm_triple_sparse_s2_hash<H::HS, H::BITS, H::TPR, H::RPB, FMA>;
template <class H> constexpr size_t t3_hash_lds() { return (size_t)H::RPB * H::HS * (sizeof(double) + sizeof(int)); }

// Rows whose T_i exceeds LDS: T_i scattered into this workgroup's zeroed row of K doubles, put back to zero afterwards.
template <bool FMA>
__global__ __launch_bounds__(256) void smm_triple_sparse_s2_global(const Triple3Args A)
{
    double *d = A.dense + (size_t)blockIdx.x * (size_t)A.K;
    for (int li = blockIdx.x; li < A.nrows; li += gridDim.x) {
        int r = A.rowlist[li];
        if (r < 0 || r >= A.m) { if (threadIdx.x == 0) plan_err(A.err, PLAN_ERR_LIST, 0); continue; }
        const int64_t t0 = A.t_ptr[r], t1 = A.t_ptr[r + 1];
        for (int64_t e = t0 + threadIdx.x; e < t1; e += blockDim.x) {
            const int col = A.t_idx[e];
            if (col >= 0 && col < A.K) d[col] = A.t_val[e];
        }
        __syncthreads();
        t3_row_values<FMA>(A, r, threadIdx.x, blockDim.x, [&](int col) -> double { return d[col]; });
        __syncthreads();
        for (int64_t e = t0 + threadIdx.x; e < t1; e += blockDim.x) {
            const int col = A.t_idx[e];
            if (col >= 0 && col < A.K) d[col] = 0.0;
        }
        __syncthreads();
    }
}

}  // namespace smm
