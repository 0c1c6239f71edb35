// smm_sddmm.hpp -- kernel of the sampled dense product (smm_sddmm): C[p] = X[i,:] . Y[j,:] for every stored entry
// p = (i, j) of a CSR mask, optionally times the mask's value.  Host driver: smm_api.hip.  X (m x k) and Y (n x k) are
// row-major float64 with leading dimensions ldx / ldy; every offset into them is 64-bit.  The mask may be any legal
// CSR (unsorted rows, repeated columns): entries are independent and each writes its own slot of the output.
//
// Lane groups.  G lanes share one entry; lane g of the group owns elements t0 + 2g and t0 + 2g + 1 of every tile
// [t0, t0 + NP) of NP = 2 G elements, so a group reads a row segment of X_i and of Y_j as consecutive 16-byte pieces
// (one 16-byte load per lane with VEC == 2 -- host: k, ldx, ldy even, X and Y 16-byte aligned -- else two 8-byte
// loads of the same two elements: the element-to-lane map, and with it every bit of the result, is that of VEC == 2).
// G = ceil(k / 2) rounded up to a power of two in [4, 64]: it depends on k alone.  A wave holds 64 / G entries.
//
// Work split: flat over the entries.  The stored entries [0, nnz) are cut into runs of `run` consecutive entries and
// the lane groups of the grid take runs round robin; a group finds the row of its run's first entry by bisection of
// the row pointer and follows the row pointer from there.  No row binning: an arrow's full row is cut like any other
// stretch of entries, and a mask with two entries per row fills its waves.
//   run == 1   (class 1, "interleaved") neighbouring groups take neighbouring entries: the mask's columns and values are
//              read coalesced; X_i is gathered per entry.
//   run == SD_RUN (class 2, "runs") a group walks SD_RUN consecutive entries, which mostly share their row: for k <= NP
//              (one tile) the group keeps its two elements of X_i in registers until the row changes.
// Order of the sum (it depends on k only -- not on the mask, the row's length, the entry's place, the class or VEC):
//   SMM_EXACT  s = +0.0; s = s + X[i,e] * Y[j,e] for e = 0 .. k-1, every product rounded before its add: the lanes of a
//              group form the products of a tile in parallel, then every lane adds them one after another in ascending
//              lane (= element) order, the technique of smm_spmv_group.
//   default    partial q of NP starts at +0.0 and takes s[q] = fma(X[i,e], Y[j,e], s[q]) for e = q, q + NP, q + 2 NP, ...
//              in ascending e; then s[q] = s[q] + s[q + h] for every q that is a multiple of 2 h, for h = 1, 2, 4, ...,
//              NP / 2; the result is s[0].  (h = 1 is the add of a lane's two partials, the rest a butterfly.)
//   With SMM_SCALE_BY_MASK the stored value is w[p] * s, the multiply always carried out.  No float atomics.
// X[i,:] and Y[j,:] are loaded only for entries that name them.
// Always-on clamps: an entry whose row is not found inside its row's range, and a column outside [0, n), is recorded in
// the context's error word (SMM_ERR_INTERNAL for the caller) and skipped -- never a fault.
#pragma once
#include "smm_spmm.hpp"

namespace smm {

constexpr int SD_RUN = 8;                 // class 2: consecutive entries per lane group

struct SddmmArgs {
    int m, n, nnz;                                                    // the mask: m x n with nnz entries
    const int *ptr; const int *idx; const double *w;
    int64_t k, ldx, ldy;
    const double *x; const double *y; double *out;
    int run;                                                          // consecutive entries per lane group (1 or SD_RUN)
    int scale;                                                        // out[p] = w[p] * s
    unsigned *err;
};

// The row whose range holds entry p: the largest r in [0, m) with ptr[r] <= p (m >= 1).  Every index read is in
// [1, m - 1] whatever ptr holds.
__device__ __forceinline__ int sd_row_of(const int *__restrict__ ptr, int m, int p)
{
    int lo = 0, hi = m;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// Elements e and e + 1 of a row (e even within its tile), 0.0 at and beyond k; nothing is read there.
template <int VEC> __device__ __forceinline__ void sd_load(const double *row, int64_t e, int64_t k, double &a, double &b)
{
    a = 0.0; b = 0.0;
    if constexpr (VEC == 2) {
        if (e < k) { const double2 v = *reinterpret_cast<const double2 *>(row + e); a = v.x; b = v.y; }      // (k is even)
    } else {
        if (e < k) a = row[e];
        if (e + 1 < k) b = row[e + 1];
    }
}

template <int G, int VEC, bool EXACT>
__global__ __launch_bounds__(256) void smm_sddmm(const SddmmArgs A)
{
    constexpr int GPW = WAVE / G, NP = 2 * G;
    const int lane = lane_id(), gl = lane & (G - 1), gbase = lane & ~(G - 1), gi = lane / G;
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int64_t)(gridDim.x * blockDim.x / WAVE);
    const int64_t nnz = A.nnz, run = A.run;
    const bool one_tile = A.k <= NP;
    double x0 = 0.0, x1 = 0.0;                                         // X[xrow, 2 gl], X[xrow, 2 gl + 1] while one_tile
    int xrow = -1;
    for (int64_t g0 = wave * GPW; g0 * run < nnz; g0 += nwaves * GPW) {                // (uniform over the wave)
        const int64_t pb = (g0 + gi) * run, pe = min(pb + run, nnz);
        int r = -1, p1 = 0;                                            // current row and the end of its range
        for (int64_t s = 0; s < run; ++s) {                           // (uniform over the wave)
            const int p = (int)min(pb + s, nnz - 1);
            bool active = pb + s < pe;
            if (active && p >= p1) {                                   // the run's first entry, or its row ended
                if (r >= 0 && r + 1 < A.m && p < A.ptr[r + 2]) ++r;    // the next row holds it: the common case
                else r = sd_row_of(A.ptr, A.m, p);
                p1 = A.ptr[r + 1];
                if (p < A.ptr[r] || p >= p1) { plan_err(A.err, PLAN_ERR_COUNT, r); p1 = 0; active = false; }
            }
            int j = 0;
            if (active) {
                j = A.idx[p];
                if (j < 0 || j >= A.n) { plan_err(A.err, PLAN_ERR_LIST, r); active = false; }
            }
            const double *xr = A.x + (int64_t)(active ? r : 0) * A.ldx;
            const double *yr = A.y + (int64_t)j * A.ldy;
            double sum = 0.0, acc0 = 0.0, acc1 = 0.0;
            for (int64_t t0 = 0; t0 < A.k; t0 += NP) {                 // (uniform over the wave)
                const int64_t e = t0 + 2 * gl;
                double y0 = 0.0, y1 = 0.0;
                if (active) {
                    if (!one_tile) sd_load<VEC>(xr, e, A.k, x0, x1);
                    else if (r != xrow) { sd_load<VEC>(xr, e, A.k, x0, x1); xrow = r; }
                    sd_load<VEC>(yr, e, A.k, y0, y1);
                }
                if constexpr (EXACT) {                                 // the tile's products one after another, ascending elements
                    const double q0 = active ? x0 * y0 : 0.0, q1 = active ? x1 * y1 : 0.0;
                    const int64_t left = A.k - t0;
#pragma unroll 8
                    for (int l = 0; l < G; ++l) {
                        const double a = sp_bcast<G == WAVE>(q0, gbase + l), b = sp_bcast<G == WAVE>(q1, gbase + l);
                        if (2 * l < left) sum = sum + a;
                        if (2 * l + 1 < left) sum = sum + b;
                    }
                } else if (active) {
                    if (e < A.k) acc0 = fma(x0, y0, acc0);
                    if (e + 1 < A.k) acc1 = fma(x1, y1, acc1);
                }
            }
            if constexpr (!EXACT) {
                sum = acc0 + acc1;
                for (int o = 1; o < G; o <<= 1) sum = sum + __shfl_xor(sum, o);
            }
            if (active && gl == 0) A.out[p] = A.scale ? A.w[p] * sum : sum;
        }
    }
}

}  // namespace smm
