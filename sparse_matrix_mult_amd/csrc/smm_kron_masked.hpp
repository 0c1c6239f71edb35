// smm_kron_masked.hpp -- kernels of the masked products with the factor form Q = D (x) E: H * (D (x) E) * H^T on the pattern
// of a mask (smm_triple_product_sparse_masked_kron) and A * (D (x) E) on the pattern of a mask (smm_spgemm_masked_kron).
// Host driver: smm_api.hip; the contract is in include/smm_hip.h.  Neither Q nor T = H * Q nor a transpose is formed: every
// value is built from the stored entries of one or two rows of H and two look-ups, D[t, t'] (a table in LDS) and E[j, j'] (bisection).
// D is p x pc, E is r x rc, both canonical (the host checks it); column t * r + j of H is the pair (t, j).
//
//   smm_kron_masked_prep    per stored entry of H: (t, j) = divmod(column, r) and the entry ranges of row t of D and row j of
//                           E, once, so that no pair of entries repeats the division or the four row-pointer loads.
//   smm_kron_masked_class   one wave per pattern row: the lanes per position G, a power of two in [4, 64], from the mean
//                           length of the rows of H the row's positions meet (triple) or the length of A_i (A * Q); the
//                           rows are binned by smm_masked_bin.
//   smm_kron_masked_triple  S[i,k]: a group of G lanes per position.  Lane l owns entry a2 = l (+ G, ...) of row k of H, column
//                           (t', j'), and forms T[i, (t', j')] alone, walking row i of H in stored order: first product
//                           lands unchanged (accumulator starts at -0.0, the identity of +), later ones are added one at a
//                           time.  Then the group adds T * H.val over a2 in stored order, starting from +0.0; a T that no
//                           product reached reads as +0.0 and is still multiplied, as smm_triple_sparse.hpp does.
//   smm_kron_masked_spgemm  C[i,c]: a group of G lanes per position, column (t', j') = divmod(c, rc).  The lanes take
//                           consecutive entries of A_i, search their pair, and the hits of a batch are added one after
//                           another in ascending lane order (the stored order of A_i) from the group's ballot, as
//                           mk_dot_values does.  A pair the factors do not store is never multiplied.
// SMM_EXACT adds one rounded product at a time; default mode uses fused multiply-adds in the same order.  q = D[t,t'] *
// E[j,j'] is rounded once in both modes: it is the value smm_kron_build stores.  No float atomics: a value depends on
// the rows of H (A) and the factors only, never on the mask, the row range, G or the launch shape.
// Always-on clamps, as in smm_kron.hpp: an inconsistent row range and a column outside its matrix are recorded in the
// context's error word and skipped; every index read is inside [0, nnz) of its array.
#pragma once
#include "smm_kron.hpp"
#include "smm_masked.hpp"

namespace smm {

template <typename PT>
struct KronMaskedArgs {
    int nb; int64_t row0;                                             // rows of the pattern; global row of its row 0
    const int *rowlist; int nrows;                                    // pattern rows of this class
    const int *h_ptr; const int *h_idx; const double *h_val; int n; int K; int nnz_h;     // H (n x K) / A (m x K)
    int4 *h_rng; int2 *h_tj;                                          // per stored entry of H: {d0, d1, e0, e1} and {t, j}
    const PT *s_ptr; const int *s_idx; double *s_val; int cols;       // pattern (nb x cols), canonical; values out
    int p, pc, r, rc, nnz_d, nnz_e;
    const int *dptr; const int *didx; const double *dval;
    const int *eptr; const int *eidx; const double *eval;
    unsigned *err;
};

// Position of column x in the strictly ascending idx[lo, hi), or -1.
__device__ __forceinline__ int km_find(const int *__restrict__ idx, int lo, int hi, int x)
{
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idx[mid] < x) lo = mid + 1; else hi = mid;
    }
    return (lo < end && idx[lo] == x) ? lo : -1;
}

// ------------------------------------------------------------------------------ per entry of H: its pair and its two rows
template <typename PT>
__global__ __launch_bounds__(256) void smm_kron_masked_prep(const KronMaskedArgs<PT> A)
{
    const int lane = lane_id(), wpb = blockDim.x / WAVE;
    for (int i = blockIdx.x * wpb + (int)(threadIdx.x / WAVE); i < A.n; i += gridDim.x * wpb) {
        int a0, al;
        kr_row(A.h_ptr, A.nnz_h, i, A.err, a0, al);
        for (int a = a0 + lane; a < a0 + al; a += WAVE) {
            const int c = A.h_idx[a];
            int4 g = make_int4(0, 0, 0, 0);
            int2 tj = make_int2(-1, -1);
            if (c < 0 || c >= A.K) {
                plan_err(A.err, PLAN_ERR_LIST, i);
            } else {
                const int t = c / A.r, j = c % A.r;                  // (t < p: the host checked p * r == K)
                int d0, ld, e0, le;
                kr_row(A.dptr, A.nnz_d, t, A.err, d0, ld);
                kr_row(A.eptr, A.nnz_e, j, A.err, e0, le);
                g = make_int4(d0, d0 + ld, e0, e0 + le);
                tj = make_int2(t, j);
            }
            A.h_rng[a] = g;
            A.h_tj[a] = tj;
        }
    }
}

// ------------------------------------------------------------------------------ lanes per position, per pattern row
// cls[r] = log2(G) - 2 for G in {4, 8, 16, 32, 64}, -1 for a row without positions.
template <bool TRIPLE, typename PT>
__global__ __launch_bounds__(256) void smm_kron_masked_class(const KronMaskedArgs<PT> A, int *__restrict__ cls)
{
    const int lane = lane_id(), wpb = blockDim.x / WAVE;
    for (int r = blockIdx.x * wpb + (int)(threadIdx.x / WAVE); r < A.nb; r += gridDim.x * wpb) {
        const int64_t s0 = A.s_ptr[r], ml = A.s_ptr[r + 1] - s0;
        if (ml <= 0) { if (lane == 0) cls[r] = -1; continue; }
        long long mean;
        if constexpr (TRIPLE) {
            long long tot = 0;
            for (int64_t q = lane; q < ml; q += WAVE) {
                const int k = mk_clamp(A.s_idx[s0 + q], A.n);
                tot += A.h_ptr[k + 1] - A.h_ptr[k];
            }
            for (int o = WAVE / 2; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
            mean = (tot + ml - 1) / ml;
        } else {
            mean = A.h_ptr[r + 1] - A.h_ptr[r];
        }
        int c = 0;
        while (c < 4 && (4ll << c) < mean) ++c;
        if (lane == 0) cls[r] = c;
    }
}

template <typename PT>
__device__ __forceinline__ int km_row(const KronMaskedArgs<PT> &A, int li)
{
    int r = A.rowlist[li];
    if (r < 0 || r >= A.nb) { plan_err(A.err, PLAN_ERR_LIST, 0); r = 0; }
    return r;
}

// D[t, t']: when p * pc <= KM_DLDS (16 KB of LDS) every workgroup holds the positions of D's entries as a dense p x pc table
// (-1: not stored) and a look-up is one LDS read; a larger D is bisected in its sorted rows like E.  Measured: the table
// takes the triple kernel from 1.16 to 0.76 ms (identity) and from 3.3 to 1.9 ms (band 16, dense D), DESIGN.md section 21.
constexpr int KM_DLDS = 4096;
template <typename PT>
__device__ __forceinline__ void km_dfill(const KronMaskedArgs<PT> &A, int *dpos)
{
    for (int x = threadIdx.x; x < A.p * A.pc; x += blockDim.x) dpos[x] = -1;
    __syncthreads();
    for (int t = threadIdx.x; t < A.p; t += blockDim.x) {
        int d0, ld;
        kr_row(A.dptr, A.nnz_d, t, A.err, d0, ld);
        for (int a = d0; a < d0 + ld; ++a) {
            const int c = A.didx[a];
            if (c >= 0 && c < A.pc) dpos[t * A.pc + c] = a;
        }
    }
    __syncthreads();
}
template <bool DLDS, typename PT>
__device__ __forceinline__ int km_dfind(const KronMaskedArgs<PT> &A, const int *dpos, const int4 &g, int a, int tc)
{
    if constexpr (DLDS) { const int t = A.h_tj[a].x; return t >= 0 ? dpos[t * A.pc + tc] : -1; }
    else return km_find(A.didx, g.x, g.y, tc);
}

// ------------------------------------------------------------------------------ T[i, (tc, jc)], one lane, row i = H[a0, a1)
template <bool EXACT, bool DLDS, typename PT>
__device__ __forceinline__ double km_t(const KronMaskedArgs<PT> &A, const int *dpos, int a0, int a1, int tc, int jc)
{
    double acc = -0.0;
    bool touched = false;
    for (int a = a0; a < a1; ++a) {
        const int4 g = A.h_rng[a];
        const int pd = km_dfind<DLDS>(A, dpos, g, a, tc);
        if (pd < 0) continue;
        const int pe = km_find(A.eidx, g.z, g.w, jc);
        if (pe < 0) continue;
        const double q = A.dval[pd] * A.eval[pe];                    // one rounded multiply: the entry of D (x) E
        const double hv = A.h_val[a];
        acc = EXACT ? acc + hv * q : __builtin_fma(hv, q, acc);      // (-ffp-contract=off: fused only where written)
        touched = true;
    }
    return touched ? acc : 0.0;
}

// ------------------------------------------------------------------------------ S[i,k] at the pattern's positions
// One wave per pattern row, 64 / G positions at a time.  Pattern rows are local (row0 + r is the row of H).
template <bool EXACT, bool DLDS>
__global__ __launch_bounds__(256) void smm_kron_masked_triple(const KronMaskedArgs<int64_t> A, int G)
{
    __shared__ int dpos[DLDS ? KM_DLDS : 1];
    if constexpr (DLDS) km_dfill(A, dpos);
    const int lane = lane_id(), gl = lane & (G - 1), base = lane & ~(G - 1), gi = lane / G, ng = WAVE / G;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int)(gridDim.x * blockDim.x / WAVE);
    for (int li = wave; li < A.nrows; li += nwaves) {                                  // (uniform over the wave)
        const int r = km_row(A, li);
        int64_t i = A.row0 + r;
        if (i < 0 || i >= A.n) { plan_err(A.err, PLAN_ERR_LIST, r); i = 0; }
        int a0, al;
        kr_row(A.h_ptr, A.nnz_h, (int)i, A.err, a0, al);
        const int64_t s0 = A.s_ptr[r], s1 = A.s_ptr[r + 1];
        for (int64_t q0 = s0; q0 < s1; q0 += ng) {                                     // (uniform over the wave)
            const int64_t q = q0 + gi;
            const bool have = q < s1;
            int b0 = 0, len = 0;
            if (have) kr_row(A.h_ptr, A.nnz_h, mk_clamp(A.s_idx[q], A.n), A.err, b0, len);
            int wlen = len;
            for (int o = G; o < WAVE; o <<= 1) wlen = max(wlen, __shfl_xor(wlen, o));
            double sum = 0.0;
            for (int bb = 0; bb < wlen; bb += G) {                                     // (uniform over the wave)
                double x = 0.0, hv = 0.0;
                if (bb + gl < len) {
                    const int e = b0 + bb + gl;
                    const int2 tj = A.h_tj[e];
                    if (tj.x >= 0) { x = km_t<EXACT, DLDS>(A, dpos, a0, a0 + al, tj.x, tj.y); hv = A.h_val[e]; }
                }
                const int cnt = len - bb, wcnt = min(G, wlen - bb);
                for (int l = 0; l < wcnt; ++l) {                                       // (uniform over the wave)
                    const double xl = __shfl(x, base + l), hl = __shfl(hv, base + l);
                    if (l < cnt) sum = EXACT ? sum + xl * hl : __builtin_fma(xl, hl, sum);
                }
            }
            if (have && gl == 0) A.s_val[q] = sum;
        }
    }
}

// ------------------------------------------------------------------------------ (A * Q)[i,c] at the mask's positions
template <bool EXACT, bool DLDS>
__global__ __launch_bounds__(256) void smm_kron_masked_spgemm(const KronMaskedArgs<int> A, int G)
{
    __shared__ int dpos[DLDS ? KM_DLDS : 1];
    if constexpr (DLDS) km_dfill(A, dpos);
    const int lane = lane_id(), gl = lane & (G - 1), base = lane & ~(G - 1), gi = lane / G, ng = WAVE / G;
    const unsigned long long gmask = G >= WAVE ? ~0ull : ((1ull << G) - 1ull);
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int)(gridDim.x * blockDim.x / WAVE);
    for (int li = wave; li < A.nrows; li += nwaves) {                                  // (uniform over the wave)
        const int r = km_row(A, li);
        int a0, al;
        kr_row(A.h_ptr, A.nnz_h, r, A.err, a0, al);
        const int s0 = A.s_ptr[r], s1 = A.s_ptr[r + 1];
        for (int q0 = s0; q0 < s1; q0 += ng) {                                         // (uniform over the wave)
            const int q = q0 + gi;
            const bool have = q < s1;
            const int c = have ? mk_clamp(A.s_idx[q], A.cols) : 0;
            const int tc = c / A.rc, jc = c % A.rc;
            double sum = -0.0;
            bool touched = false;
            for (int ab = 0; ab < al; ab += G) {                                       // (uniform over the wave)
                const int a = a0 + ab + gl;
                bool hit = false;
                double qv = 0.0, hv = 0.0;
                if (have && ab + gl < al) {
                    const int4 g = A.h_rng[a];
                    const int pd = km_dfind<DLDS>(A, dpos, g, a, tc);
                    const int pe = pd >= 0 ? km_find(A.eidx, g.z, g.w, jc) : -1;
                    if (pe >= 0) {
                        hit = true;
                        qv = A.dval[pd] * A.eval[pe];                // one rounded multiply: the entry of D (x) E
                        hv = A.h_val[a];
                        if (EXACT) qv = hv * qv;
                    }
                }
                unsigned long long hits = (__ballot(hit) >> base) & gmask;
                touched |= hits != 0;
                while (hits) {
                    const int l = __ffsll((long long)hits) - 1;
                    const double ql = __shfl(qv, base + l);
                    if constexpr (EXACT) {
                        sum = sum + ql;
                    } else {
                        const double hl = __shfl(hv, base + l);
                        sum = __builtin_fma(hl, ql, sum);
                    }
                    hits &= hits - 1ull;
                }
            }
            if (have && gl == 0) A.s_val[q] = touched ? sum : 0.0;
        }
    }
}

}  // namespace smm
