// smm_masked.hpp -- kernels of the masked SpGEMM C = (A * B) on the pattern of a mask M (smm_spgemm_masked) and the
// pattern step of the masked sparse triple product (smm_triple_product_sparse_masked).  Host driver: smm_api.hip.
//
// Every value is written in the mask's order (C's pattern IS the mask's), so rows of either path mix freely:
//   dot path (B^T-driven)   C[i,j] = sum over row j of B^T (ascending k) of A[i,k] * B^T[j,k].  A_i is held in a
//                           lookup table (wave / workgroup LDS hash, or a zeroed global row of K ints holding source
//                           positions for long A_i); groups of lanes take consecutive mask entries, the lanes of a group
//                           consecutive entries of B^T_j.  Only for a canonical A: then ascending k IS the reference
//                           order (A_i in stored order, B_k in stored order).
//   row path (Gustavson)    M_i's columns in a column -> slot table (wave / workgroup LDS hash, or a zeroed global slot
//                           map of B.cols ints); A_i walked in stored order, lanes take consecutive entries of B_k,
//                           misses skipped, hits added with ds_add_f64.  SMM_EXACT: one wave owns the row, so the
//                           hardware's in-order, ascending-lane application of ds_add_f64 (exact_guard) gives the
//                           reference order for any legal A and B.  The global class accumulates in HBM with plain
//                           read-modify-writes of that one wave (lanes of one batch one after another when B may repeat
//                           a column inside a row).
// Accumulators start at -0.0 (the identity of +: the first product lands unchanged, as the reference's first touch
// acc = a*b) next to a touched flag; a mask position no product reaches is written as +0.0.  A pair (k, j) that A_i
// does not store is never multiplied, so an inf in B cannot leak into C through a missing A[i,k].
#pragma once
#include "smm_rowclass.hpp"

namespace smm {

constexpr int MK_TOUCH = 1 << 30;      // row-global slot map: "some product reached this slot"
enum { MK_DOT_WAVE = 0, MK_DOT_WG = 1, MK_DOT_GLOBAL = 2, MK_ROW_WAVE = 3, MK_ROW_WG = 4, MK_ROW_GLOBAL = 5, MK_NCLS = 6 };

struct MaskedArgs {
    int m;                                                            // rows of A / the mask
    const int *rowlist; int nrows;                                    // rows of this class
    const int *a_ptr; const int *a_idx; const double *a_val; int K;   // A (m x K)
    const int *b_ptr; const int *b_idx; const double *b_val; int n;   // B (K x n)
    const int *t_ptr; const int *t_idx; const double *t_val;          // B^T with values (n x K), dot path only
    const int *m_ptr; const int *m_idx;                               // mask (m x n), canonical
    double *out;                                                      // nnz(mask) values in the mask's order
    int *map;                                                         // global classes: one zeroed row per workgroup
    int bdup;                                                         // B may repeat a column inside a row
    unsigned *err;
};

__device__ __forceinline__ int mk_clamp(int v, int hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : v); }

// ------------------------------------------------------------------------------ cost model and binning
// One wave per mask row.  mode: 0 auto, 1 dot, 2 row; t_ptr == nullptr means the dot path is not available (A not
// canonical, or forced row).  cls[r] = MK_* class, -1 for an empty mask row.
//   dot cost  nnz(A_i) + sum over j in M_i of nnz(B^T_j)       row cost  sum over k in A_i of nnz(B_k)
__global__ __launch_bounds__(256) void smm_masked_cost(int m, const int *__restrict__ m_ptr, const int *__restrict__ m_idx,
                                                       const int *__restrict__ a_ptr, const int *__restrict__ a_idx,
                                                       const int *__restrict__ b_ptr, int K, const int *__restrict__ t_ptr, int n,
                                                       int mode, int *__restrict__ cls)
{
    const int lane = lane_id(), wpb = blockDim.x / WAVE;
    for (int r = blockIdx.x * wpb + (int)(threadIdx.x / WAVE); r < m; r += gridDim.x * wpb) {
        const int m0 = m_ptr[r], ml = m_ptr[r + 1] - m0;
        if (ml <= 0) { if (lane == 0) cls[r] = -1; continue; }
        const int a0 = a_ptr[r], al = a_ptr[r + 1] - a0;
        bool dot = t_ptr != nullptr && mode != 2;
        if (dot && mode == 0) {
            long long dc = 0, rc = 0;
            for (int q = lane; q < ml; q += WAVE) {
                const int j = mk_clamp(m_idx[m0 + q], n);
                dc += t_ptr[j + 1] - t_ptr[j];
            }
            for (int p = lane; p < al; p += WAVE) {
                const int k = mk_clamp(a_idx[a0 + p], K);
                rc += b_ptr[k + 1] - b_ptr[k];
            }
            for (int o = WAVE / 2; o > 0; o >>= 1) { dc += __shfl_xor(dc, o); rc += __shfl_xor(rc, o); }
            dot = dc + al <= rc;
        }
        if (lane == 0)
            cls[r] = dot ? (al <= WaveHash::MAX ? MK_DOT_WAVE : (al <= WgHash::MAX ? MK_DOT_WG : MK_DOT_GLOBAL))
                         : (ml <= WaveHash::MAX ? MK_ROW_WAVE : (ml <= WgHash::MAX ? MK_ROW_WG : MK_ROW_GLOBAL));
    }
}

// lists[c*m ..] = rows of class c, counts[c]; one atomic per wave and class.
__global__ __launch_bounds__(256) void smm_masked_bin(int m, const int *__restrict__ cls, int *__restrict__ lists, int *__restrict__ counts)
{
    for (int r0 = blockIdx.x * blockDim.x; r0 < m; r0 += gridDim.x * blockDim.x) {     // (uniform over the block)
        const int r = r0 + (int)threadIdx.x;
        class_list_append(r < m ? cls[r] : -1, MK_NCLS, m, r, lists, counts);
    }
}

__device__ __forceinline__ int mk_row(const MaskedArgs &A, int li)
{
    int r = A.rowlist[li];
    if (r < 0 || r >= A.m) { plan_err(A.err, PLAN_ERR_LIST, 0); r = 0; }
    return r;
}

// ------------------------------------------------------------------------------ dot path
// C[i,j] for the mask entries of row r: groups of G lanes (G a power of two <= 64, from the mean length of a row of
// B^T) take consecutive mask entries; the lanes of a group take consecutive entries of B^T_j, look k up and form their
// products, and the hits of one batch are added one after another in ascending lane order -- ascending k, the order
// of B^T_j -- from the group's ballot.  Misses are skipped, never multiplied.  t: thread of the row's nt threads.
// look(k) -> source position of A[i,k] in A, or -1.
template <typename Look>
__device__ __forceinline__ void mk_dot_values(const MaskedArgs &A, int r, int t, int nt, int G, Look look)
{
    const int m0 = A.m_ptr[r], m1 = A.m_ptr[r + 1];
    const int gl = t & (G - 1), base = lane_id() & ~(G - 1);
    const unsigned long long gmask = G >= WAVE ? ~0ull : ((1ull << G) - 1ull);
    for (int q = m0 + t / G; q < m1; q += nt / G) {               // (uniform over the group)
        const int j = mk_clamp(A.m_idx[q], A.n);
        double sum = -0.0;
        bool touched = false;
        const int e1 = A.t_ptr[j + 1];
        for (int eb = A.t_ptr[j]; eb < e1; eb += G) {               // (uniform over the group)
            const int e = eb + gl;
            const int p = e < e1 ? look(A.t_idx[e]) : -1;
            const double v = p >= 0 ? A.a_val[p] * A.t_val[e] : 0.0;
            unsigned long long hits = (__ballot(p >= 0) >> base) & gmask;
            touched |= hits != 0;
            while (hits) {
                const int l = __ffsll((long long)hits) - 1;
                sum = sum + __shfl(v, base + l);
                hits &= hits - 1ull;
            }
        }
        if (gl == 0) A.out[q] = touched ? sum : 0.0;
    }
}

// A_i in an LDS hash k -> source position: HS slots per row group of TPR threads, RPB row groups per workgroup;
// dynamic LDS mk_dot_lds<H>().
template <int HS, int BITS, int TPR, int RPB>
__global__ __launch_bounds__(TPR * RPB) void smm_masked_dot_hash(const MaskedArgs A, int G)
{
    extern __shared__ int mk_dlds[];
    const int g = threadIdx.x / TPR, t = threadIdx.x % TPR;
    const LdsHash<HS, BITS> h{mk_dlds + (size_t)g * 2 * HS};
    int *hp = h.key + HS;
    for (int base = blockIdx.x * RPB; base < A.nrows; base += gridDim.x * RPB) {     // (uniform over the block)
        const int li = base + g;
        const bool have = li < A.nrows;
        const int r = have ? mk_row(A, li) : 0;
        h.clear(t, TPR);
        __syncthreads();
        const int a0 = A.a_ptr[r];
        int al = A.a_ptr[r + 1] - a0;
        if (al > HS / 2) { if (have && t == 0) plan_err(A.err, PLAN_ERR_HASH, r); al = HS / 2; }
        if (have) {
            for (int e = t; e < al; e += TPR) {
                const int s = h.insert(A.a_idx[a0 + e]);
                if (s >= 0) hp[s] = a0 + e;
            }
        }
        __syncthreads();
        if (have)
            mk_dot_values(A, r, t, TPR, G, [&](int k) { return h.find(k, -1, [&](int s) { return hp[s]; }); });
        __syncthreads();
    }
}
// Its instance for hash class H and its dynamic LDS: per row, HS keys then HS source positions.
template <class H> constexpr auto mk_dot_kernel = smm_masked_dot_hash<H::HS, H::BITS, H::TPR, H::RPB>;
template <class H> constexpr size_t mk_dot_lds() { return (size_t)H::RPB * H::HS * 2 * sizeof(int); }

// Long A_i: source positions + 1 scattered into this workgroup's zeroed row of K ints, put back to zero afterwards.
__global__ __launch_bounds__(256) void smm_masked_dot_global(const MaskedArgs A, int G)
{
    int *d = A.map + (size_t)blockIdx.x * (size_t)A.K;
    for (int li = blockIdx.x; li < A.nrows; li += gridDim.x) {
        const int r = mk_row(A, li);
        const int a0 = A.a_ptr[r], a1 = A.a_ptr[r + 1];
        for (int p = a0 + threadIdx.x; p < a1; p += blockDim.x) d[mk_clamp(A.a_idx[p], A.K)] = p + 1;
        __syncthreads();
        mk_dot_values(A, r, threadIdx.x, blockDim.x, G, [&](int k) -> int { return (k >= 0 && k < A.K) ? d[k] - 1 : -1; });
        __syncthreads();
        for (int p = a0 + threadIdx.x; p < a1; p += blockDim.x) d[mk_clamp(A.a_idx[p], A.K)] = 0;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------ row path
// M_i in an LDS hash column -> accumulator (-0.0) + touched byte: HS slots per row group of TPR threads, RPB row groups
// per workgroup; dynamic LDS mk_row_lds<H>().  A_i is walked by one wave (EXACT, or TPR == WAVE) or by all waves
// of the group, each taking every (TPR / WAVE)-th k.
template <int HS, int BITS, int TPR, int RPB, bool EXACT>
__global__ __launch_bounds__(TPR * RPB) void smm_masked_row_hash(const MaskedArgs A)
{
    extern __shared__ double mk_rlds[];
    const int g = threadIdx.x / TPR, t = threadIdx.x % TPR;
    const int lane = t % WAVE, w = t / WAVE, nw = EXACT ? 1 : TPR / WAVE;
    double *hv = mk_rlds + (size_t)g * HS;
    const LdsHash<HS, BITS> h{(int *)(mk_rlds + (size_t)RPB * HS) + (size_t)g * HS};
    unsigned char *ht = (unsigned char *)((int *)(mk_rlds + (size_t)RPB * HS) + (size_t)RPB * HS) + (size_t)g * HS;
    for (int base = blockIdx.x * RPB; base < A.nrows; base += gridDim.x * RPB) {     // (uniform over the block)
        const int li = base + g;
        const bool have = li < A.nrows;
        const int r = have ? mk_row(A, li) : 0;
        h.clear(t, TPR, [&](int s) { hv[s] = -0.0; ht[s] = 0; });
        __syncthreads();
        const int m0 = A.m_ptr[r], m1 = A.m_ptr[r + 1];
        int ml = m1 - m0;
        if (ml > HS / 2) { if (have && t == 0) plan_err(A.err, PLAN_ERR_HASH, r); ml = HS / 2; }
        if (have) {
            for (int q = t; q < ml; q += TPR) (void)h.insert(A.m_idx[m0 + q]);
        }
        __syncthreads();
        if (have && w < nw) {
            const int a1 = A.a_ptr[r + 1];
            for (int p = A.a_ptr[r] + w; p < a1; p += nw) {
                const int k = mk_clamp(A.a_idx[p], A.K);
                const double a = A.a_val[p];
                const int e1 = A.b_ptr[k + 1];
                for (int e = A.b_ptr[k] + lane; e < e1; e += WAVE) {
                    const int s = h.find(A.b_idx[e]);
                    if (s < 0) continue;
                    lds_add(&hv[s], a * A.b_val[e]);
                    ht[s] = 1;
                }
            }
        }
        __syncthreads();
        if (have)
            for (int q = m0 + t; q < m1; q += TPR) {
                const int s = h.find(A.m_idx[q]);
                A.out[q] = (s >= 0 && ht[s]) ? hv[s] : 0.0;
            }
        __syncthreads();
    }
}

// Its instance for hash class H and its dynamic LDS: the accumulators of the RPB rows (HS doubles each), their keys,
// their touched bytes.
template <class H, bool EXACT> constexpr auto mk_row_kernel = smm_masked_row_hash<H::HS, H::BITS, H::TPR, H::RPB, EXACT>;
template <class H> constexpr size_t mk_row_lds() { return (size_t)H::RPB * H::HS * (sizeof(double) + sizeof(int) + 1); }

// Long mask rows: slot + 1 (| MK_TOUCH once a product lands) in this workgroup's zeroed map of n ints, accumulators in
// the output itself.  EXACT: wave 0 alone walks A_i with plain read-modify-writes (one wave's accesses to global memory
// are seen by its own later accesses in order; the fences keep the compiler from reordering them), lanes of one batch
// one after another when B may repeat a column.  Default: every wave takes its own k, global atomics.
template <bool EXACT>
__global__ __launch_bounds__(256) void smm_masked_row_global(const MaskedArgs A)
{
    int *map = A.map + (size_t)blockIdx.x * (size_t)A.n;
    const int lane = lane_id(), w = threadIdx.x / WAVE, nw = EXACT ? 1 : (int)(blockDim.x / WAVE);
    for (int li = blockIdx.x; li < A.nrows; li += gridDim.x) {
        const int r = mk_row(A, li);
        const int m0 = A.m_ptr[r], m1 = A.m_ptr[r + 1];
        for (int q = m0 + threadIdx.x; q < m1; q += blockDim.x) {
            map[mk_clamp(A.m_idx[q], A.n)] = q - m0 + 1;
            A.out[q] = -0.0;
        }
        __syncthreads();
        if (w < nw) {
            const int a1 = A.a_ptr[r + 1];
            for (int p = A.a_ptr[r] + w; p < a1; p += nw) {
                const int k = mk_clamp(A.a_idx[p], A.K);
                const double a = A.a_val[p];
                const int e0 = A.b_ptr[k], e1 = A.b_ptr[k + 1];
                for (int eb = e0; eb < e1; eb += WAVE) {            // (uniform over the wave)
                    const int e = eb + lane;
                    int j = 0, s = 0;
                    double v = 0.0;
                    if (e < e1) {
                        j = mk_clamp(A.b_idx[e], A.n);
                        s = map[j] & ~MK_TOUCH;
                        if (s > m1 - m0) { plan_err(A.err, PLAN_ERR_HASH, r); s = 0; }
                        v = a * A.b_val[e];
                    }
                    if constexpr (EXACT) {
                        if (!A.bdup) {
                            if (s > 0) { A.out[m0 + s - 1] = A.out[m0 + s - 1] + v; map[j] = s | MK_TOUCH; }
                        } else {
                            for (int l = 0; l < WAVE; ++l) {
                                if (lane == l && s > 0) { A.out[m0 + s - 1] = A.out[m0 + s - 1] + v; map[j] = s | MK_TOUCH; }
                                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    } else {
                        if (s > 0) { glb_add(&A.out[m0 + s - 1], v); map[j] = s | MK_TOUCH; }
                    }
                }
            }
        }
        __syncthreads();
        for (int q = m0 + threadIdx.x; q < m1; q += blockDim.x) {
            const int j = mk_clamp(A.m_idx[q], A.n);
            const bool touched = (map[j] & MK_TOUCH) != 0;
            const double x = EXACT ? A.out[q] : __hip_atomic_load(&A.out[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            A.out[q] = touched ? x : 0.0;
            map[j] = 0;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------ masked triple product: stage-2 pattern
// Rows [b0, b0 + nb) of the mask filtered to k >= i (mask canonical: a lower bound per row).
__global__ __launch_bounds__(256) void smm_masked_tri_count(int nb, int64_t b0, const int *__restrict__ m_ptr, const int *__restrict__ m_idx,
                                                            int *__restrict__ cnt, int *__restrict__ first)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nb; r += gridDim.x * blockDim.x) {
        const int64_t i = b0 + r;
        int lo = m_ptr[i], hi = m_ptr[i + 1];
        const int end = hi;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)m_idx[mid] < i) lo = mid + 1; else hi = mid;
        }
        first[r] = lo;
        cnt[r] = end - lo;
    }
}
__global__ __launch_bounds__(256) void smm_masked_tri_copy(int nb, const int *__restrict__ first, const int *__restrict__ cnt,
                                                           const int64_t *__restrict__ s_ptr, const int *__restrict__ m_idx, int *__restrict__ s_idx)
{
    const int lane = lane_id(), wpb = blockDim.x / WAVE;
    for (int r = blockIdx.x * wpb + (int)(threadIdx.x / WAVE); r < nb; r += gridDim.x * wpb) {
        const int f = first[r], c = cnt[r];
        const int64_t o = s_ptr[r];
        for (int q = lane; q < c; q += WAVE) s_idx[o + q] = m_idx[f + q];
    }
}

}  // namespace smm
