// smm_taper.hpp -- kernels of smm_taper_build: the localisation taper L[i,j] = w(|a_i - b_j|) for every pair of points
// closer than a cutoff, as a canonical CSR built on the device.  Host driver: smm_api.hip.  a (na x DIM) and b (nb x DIM)
// are row-major float64 with leading dimensions lda / ldb; every offset into them is 64-bit.
//
// The contract in three functions, shared by every pass (so the count, the fill and the values cannot disagree):
//   tp_d2      d2 = +0.0; for t = 0 .. DIM-1: df = a[t] - b[t]; d2 = d2 + df * df      (the product rounded before the add)
//   tp_member  d2 < cut2, cut2 = cutoff * cutoff rounded once on the host.  This test ALONE decides the pattern.
//   tp_weight  boxcar 1.0, or Gaspari & Cohn (1999) eq. 4.10 in the Horner order of include/smm_hip.h, clamped at +0.0.
//
// Passes:  bounding box of b and a count of non-finite coordinates (per-block partials, reduced on the host) -> cell of
// every point of b (integer atomics count the cells) -> smm_scan -> scatter into cell order (a counting sort: sorted
// copy of b's coordinates + original indices; the order inside a cell is the atomics' arrival order and never reaches
// the result) -> count per row of a -> smm_scan -> fill (original b indices, any order) -> segmented sort of every row
// (smm_seg_sort: distinct keys) -> values from the sorted columns and the int32 row pointer.
//
// The cell search and why it loses no pair.  A point x has cell coordinate
//     g_t(x) = clamp(trunc((x - lo_t) * inv_h), 0, nc_t - 1)                     per dimension t (0 where nc_t == 1)
// one IEEE subtraction of a constant, one IEEE multiplication by a positive constant, a clamp and a truncation of a
// non-negative number: every step is monotone non-decreasing in x, so g_t is, whatever the rounding does to the
// quotient.  A pair that passes tp_member has fl(df_t * df_t) <= d2 < fl(cutoff * cutoff) in every dimension (d2 only
// grows: it adds non-negative terms, and rounding is monotone), hence |fl(a_t - b_t)| < cutoff (squaring and rounding
// are monotone), hence |a_t - b_t| < cutoff in real numbers (cutoff is representable and rounding is monotone).  The
// query computes xl = nextafter(fl(a_t - cutoff), -inf) <= a_t - cutoff and xh = nextafter(fl(a_t + cutoff), +inf) >=
// a_t + cutoff (a correctly rounded sum is within one neighbour of the real one), so xl < b_t < xh, and by monotonicity
// g_t(xl) <= g_t(b_t) <= g_t(xh).  The query therefore walks the cells [g_t(xl), g_t(xh)] in every dimension -- a range
// it derives from the SAME function that binned b, not "own cell +- 1".  Nothing here needs the edge to exceed the
// cutoff or the quotient to round any particular way; an edge 1 + 2^-20 times the cutoff only makes the range three
// cells wide except for coordinates beyond 2^32 cutoffs.  With x the fastest cell coordinate the cells [g_0(xl), g_0(xh)]
// of one (y, z) are one contiguous range of sorted points: a query walks (cells in y) * (cells in z) ranges.
//
// Lane mapping: TP_G lanes share a query.  They stride over a candidate range together, test one candidate each, and
// a ballot over the group gives every hit its slot in the row (count pass: only the number).  The lanes of a group
// always execute the same loop iteration, so the ballot sees all of them.  Queries are taken in cell order (the
// counting sort's order, also made for a when a is not b's buffer), so the groups of a wave walk the same ranges and
// find them in L2; rows are addressed through the row pointer, so the processing order never reaches the result.
// Always-on clamps: a fill that would leave its row, a row whose fill does not end at its end and a column outside
// [0, nb) are recorded in the context's error word (SMM_ERR_INTERNAL for the caller) and skipped -- never a fault.
#pragma once
#include "smm_triple_sparse.hpp"

#include <cfloat>

namespace smm {

constexpr int TP_G = 16;                    // lanes per query (count / fill) and per row (values)
constexpr int TP_PART = 8;                  // doubles per block partial of smm_taper_bbox: min[3], max[3], non-finite count, pad
enum { TP_BOXCAR = 0, TP_GASPARI_COHN = 1 };      // SMM_TAPER_* of include/smm_hip.h

struct TaperGrid {
    int nc[3];                              // cells per dimension (1 beyond DIM)
    double lo[3], hi[3];                    // bounding box of b
    double inv_h;                           // 1 / edge
    double cutoff, cut2, half;              // cutoff, fl(cutoff * cutoff), 0.5 * cutoff
};

template <int DIM> __device__ __forceinline__ void tp_load(const double *__restrict__ p, double (&x)[3])
{
    x[0] = p[0];
    x[1] = DIM > 1 ? p[DIM > 1 ? 1 : 0] : 0.0;
    x[2] = DIM > 2 ? p[DIM > 2 ? 2 : 0] : 0.0;
}

template <int DIM> __device__ __forceinline__ double tp_d2(const double (&a)[3], const double (&b)[3])
{
    double d2 = 0.0;
#pragma unroll
    for (int t = 0; t < DIM; ++t) {
        const double df = a[t] - b[t];
        d2 = d2 + df * df;
    }
    return d2;
}
__device__ __forceinline__ bool tp_member(double d2, double cut2) { return d2 < cut2; }

__device__ __forceinline__ double tp_weight(int kind, double d2, double half)
{
    if (kind == TP_BOXCAR) return 1.0;
    const double z = sqrt(d2) / half;
    double p;
    if (z <= 1.0) {
        p = -0.25 * z + 0.5;
        p = p * z + 0.625;
        p = p * z - (5.0 / 3.0);
        p = p * z;
        p = p * z + 1.0;
    } else {
        p = (1.0 / 12.0) * z - 0.5;
        p = p * z + 0.625;
        p = p * z + (5.0 / 3.0);
        p = p * z - 5.0;
        p = p * z + 4.0;
        p = p - 2.0 / (3.0 * z);
    }
    return p < 0.0 ? 0.0 : p;
}

// Cell coordinate of x in dimension t: monotone non-decreasing in x (see the head of this file).  x may be +-inf.
__device__ __forceinline__ int tp_cell1(const TaperGrid &g, int t, double x)
{
    if (g.nc[t] == 1) return 0;
    double q = (x - g.lo[t]) * g.inv_h;
    const double top = (double)(g.nc[t] - 1);
    q = q > 0.0 ? q : 0.0;
    q = q < top ? q : top;
    return (int)q;
}
template <int DIM> __device__ __forceinline__ int tp_cell(const TaperGrid &g, const double (&x)[3])
{
    int cell = tp_cell1(g, 0, x[0]);
    if (DIM > 1) cell += g.nc[0] * tp_cell1(g, 1, x[1]);
    if (DIM > 2) cell += g.nc[0] * g.nc[1] * tp_cell1(g, 2, x[2]);
    return cell;
}

// ------------------------------------------------------------------------------ bounding box + non-finite count
// partial[block * TP_PART ..]: min[3], max[3] over the block's finite coordinates, then the number of non-finite ones.
template <int DIM>
__global__ __launch_bounds__(256) void smm_taper_bbox(int64_t n, const double *__restrict__ pts, int64_t ld, double *__restrict__ partial)
{
    __shared__ double sh[4][TP_PART];
    double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX}, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
            const double v = pts[i * ld + t];
            if (!(fabs(v) <= DBL_MAX)) bad = bad + 1.0;                 // (counts < 2^53: exact)
            else { mn[t] = v < mn[t] ? v : mn[t]; mx[t] = v > mx[t] ? v : mx[t]; }
        }
    }
    for (int o = 1; o < WAVE; o <<= 1) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const double a = __shfl_xor(mn[t], o), b = __shfl_xor(mx[t], o);
            mn[t] = a < mn[t] ? a : mn[t];
            mx[t] = b > mx[t] ? b : mx[t];
        }
        bad = bad + __shfl_xor(bad, o);
    }
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int t = 0; t < 3; ++t) { sh[wave][t] = mn[t]; sh[wave][3 + t] = mx[t]; }
        sh[wave][6] = bad; sh[wave][7] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < TP_PART) {
        const int s = threadIdx.x;
        double r = sh[0][s];
        for (int w = 1; w < 4; ++w) {
            const double v = sh[w][s];
            r = s < 3 ? (v < r ? v : r) : s < 6 ? (v > r ? v : r) : r + v;
        }
        partial[(int64_t)blockIdx.x * TP_PART + s] = r;
    }
}

// ------------------------------------------------------------------------------ counting sort by cell
template <int DIM>
__global__ __launch_bounds__(256) void smm_taper_cell_count(const TaperGrid g, int64_t n, const double *__restrict__ pts, int64_t ld,
                                                            int ncells, int *__restrict__ cell_of, int *__restrict__ cnt)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double x[3];
        tp_load<DIM>(pts + i * ld, x);
        int cell = tp_cell<DIM>(g, x);
        cell = cell < 0 ? 0 : (cell >= ncells ? ncells - 1 : cell);        // (always inside: the clamps of tp_cell1)
        cell_of[i] = cell;
        atomicAdd(&cnt[cell], 1);
    }
}
// order[q] = original index of the point at sorted position q; sorted (may be NULL): its coordinates, packed DIM per point
template <int DIM>
__global__ __launch_bounds__(256) void smm_taper_cell_scatter(int64_t n, const double *__restrict__ pts, int64_t ld, int ncells,
                                                              const int *__restrict__ cell_of, const int64_t *__restrict__ start,
                                                              int *__restrict__ cursor, int *__restrict__ order, double *__restrict__ sorted,
                                                              unsigned *__restrict__ err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int cell = cell_of[i];
        if (cell < 0 || cell >= ncells) { plan_err(err, PLAN_ERR_LIST, 0); continue; }
        const int slot = atomicAdd(&cursor[cell], 1);
        const int64_t q = start[cell] + slot;
        if (slot < 0 || q >= start[cell + 1] || q >= n) { plan_err(err, PLAN_ERR_COUNT, 0); continue; }
        order[q] = (int)i;
        if (sorted) {
#pragma unroll
            for (int t = 0; t < DIM; ++t) sorted[q * DIM + t] = pts[i * ld + t];
        }
    }
}

// ------------------------------------------------------------------------------ count / fill
struct TaperSearch {
    TaperGrid g;
    int64_t na, nb;
    int ncells;
    const double *a; int64_t lda;
    const int *order_a;                     // queries in cell order: query q is row order_a[q] of a
    const int64_t *start;                   // ncells + 1: first sorted position of every cell of b
    const double *sorted_b;                 // b's coordinates in cell order, DIM per point
    const int *order_b;                     // original index of the sorted point (FILL)
    int *rowcnt;                            // COUNT: na row lengths
    const int64_t *rowoff;                  // FILL: na + 1 row offsets
    int *idx;                               // FILL: the columns, any order inside a row
    unsigned *err;
};

template <int DIM, bool FILL>
__global__ __launch_bounds__(256) void smm_taper_search(const TaperSearch A)
{
    constexpr int GPW = WAVE / TP_G;
    const int lane = lane_id(), gl = lane & (TP_G - 1), gbase = lane & ~(TP_G - 1), gi = lane / TP_G;
    const unsigned below = (1u << gl) - 1u;
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int64_t)(gridDim.x * blockDim.x / WAVE);
    const TaperGrid &g = A.g;
    for (int64_t q0 = wave * GPW; q0 < A.na; q0 += nwaves * GPW) {           // (uniform over the wave)
        const int64_t qi = q0 + gi;
        if (qi >= A.na) continue;                                              // (uniform over the group)
        int row = A.order_a[qi];
        if (row < 0 || row >= A.na) { if (gl == 0) plan_err(A.err, PLAN_ERR_LIST, 0); continue; }
        double p[3];
        tp_load<DIM>(A.a + (int64_t)row * A.lda, p);
        int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
        bool empty = false;
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
            const double xl = nextafter(p[t] - g.cutoff, -HUGE_VAL), xh = nextafter(p[t] + g.cutoff, HUGE_VAL);
            if (xh < g.lo[t] || xl > g.hi[t]) empty = true;                   // every b_t lies in [lo_t, hi_t] and in (xl, xh)
            c0[t] = tp_cell1(g, t, xl);
            c1[t] = tp_cell1(g, t, xh);
        }
        int64_t r0 = 0, r1 = 0;
        if (FILL) { r0 = A.rowoff[row]; r1 = A.rowoff[row + 1]; }
        int w = 0;                                                            // hits so far (uniform over the group)
        if (!empty) {
            for (int cz = c0[2]; cz <= c1[2]; ++cz) {
                for (int cy = c0[1]; cy <= c1[1]; ++cy) {
                    const int base = g.nc[0] * (cy + g.nc[1] * cz);
                    int first = base + c0[0], last = base + c1[0];
                    if (first < 0 || last >= A.ncells || first > last) continue;       // (always inside: the clamps of tp_cell1)
                    int64_t beg = A.start[first], end = A.start[last + 1];
                    beg = beg < 0 ? 0 : beg;
                    end = end > A.nb ? A.nb : end;
                    for (int64_t s = beg; s < end; s += TP_G) {               // (uniform over the group)
                        const int64_t j = s + gl;
                        bool hit = false;
                        if (j < end) {
                            double x[3];
                            tp_load<DIM>(A.sorted_b + j * DIM, x);
                            hit = tp_member(tp_d2<DIM>(p, x), g.cut2);
                        }
                        const unsigned m = (unsigned)(__ballot(hit) >> gbase) & ((1u << TP_G) - 1u);
                        if (FILL && hit) {
                            const int64_t pos = r0 + w + __popc(m & below);
                            if (pos < r1) A.idx[pos] = A.order_b[j];
                            else plan_err(A.err, PLAN_ERR_COUNT, row);
                        }
                        w += __popc(m);
                    }
                }
            }
        }
        if (gl == 0) {
            if (!FILL) A.rowcnt[row] = w;
            else if (r0 + w != r1) plan_err(A.err, PLAN_ERR_COUNT, row);
        }
    }
}

// ------------------------------------------------------------------------------ values + int32 row pointer
// One lane group per row: d2 again, in the contract's order, from a_i and the ORIGINAL b_j of every sorted column.
template <int DIM>
__global__ __launch_bounds__(256) void smm_taper_values(int kind, double half, int64_t na, const double *__restrict__ a, int64_t lda, int64_t nb,
                                                        const double *__restrict__ b, int64_t ldb, const int64_t *__restrict__ off,
                                                        const int *__restrict__ idx, int *__restrict__ ptr, double *__restrict__ val,
                                                        unsigned *__restrict__ err)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i <= na; i += nthreads) ptr[i] = (int)off[i];
    const int gl = (int)(tid & (TP_G - 1));
    for (int64_t i = tid / TP_G; i < na; i += nthreads / TP_G) {
        double p[3];
        tp_load<DIM>(a + i * lda, p);
        const int64_t e = off[i + 1];
        for (int64_t q = off[i] + gl; q < e; q += TP_G) {
            const int j = idx[q];
            if (j < 0 || j >= nb) { plan_err(err, PLAN_ERR_LIST, (int)i); continue; }
            double x[3];
            tp_load<DIM>(b + (int64_t)j * ldb, x);
            val[q] = tp_weight(kind, tp_d2<DIM>(p, x), half);
        }
    }
}

}  // namespace smm
