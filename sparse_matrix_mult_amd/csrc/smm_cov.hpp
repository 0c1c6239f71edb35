// smm_cov.hpp -- kernel of smm_cov_eval: a parametric covariance, and optionally its derivative with respect to a
// correlation length, at every stored entry p = (i, j) of a CSR pattern, from the coordinates a_i and b_j.  Host driver:
// smm_api.hip; contract: include/smm_hip.h.  a (m x DIM) and b (n x DIM) are row-major float64 with leading dimensions
// lda / ldb; every offset into them is 64-bit.  The pattern may be any legal CSR (unsorted rows, repeated columns, empty
// rows): entries are independent and each writes its own slot of val and / or dval.
//
// The contract in three functions (every product rounded before its add: the library is built with -ffp-contract=off):
//   cv_scaled  u_t = (a[t] - b[t]) / len[t] (IEEE division); h2 = +0.0; h2 = h2 + u_t * u_t for t = 0 .. DIM-1; h = sqrt(h2)
//   cv_model   c(h) and g(h) = -dc/dh of the five models, e = exp(x) the device library's double exp
//   cv_dlength +0.0 when h == 0, else ((variance * g) * (u_t * u_t)) / (h * len[t]), or ((variance * g) * h) / len for the
//              common length
// The value is variance * c; with `scale` each output is multiplied last by the pattern's stored value, always.
//
// Lane map: one lane per entry -- there is no k to share.  The entries [0, nnz) are cut into runs of CV_RUN = 64 * CV_STEPS
// consecutive entries and the WAVES of the grid take runs round robin; in step s of a run lane l has entry
// base + 64 s + l, so the columns and weights are read and both outputs written as 64 consecutive elements.  A lane
// finds the row of its first entry by bisection of the row pointer (sd_row_of) and follows the row pointer from there
// (cv_row_from: a gallop from the row it has, so 64 entries further down costs one or two cached loads in rows of dozens
// of entries and log2 of the rows skipped elsewhere).  No row binning: an arrow's full row is cut like any other stretch,
// and a pattern with two entries per row fills its waves.  a_i is reloaded only when the lane's row changes.
// Always-on clamps: an entry whose row is not found inside its row's range, and a column outside [0, n), is recorded in
// the context's error word (SMM_ERR_INTERNAL for the caller) and skipped -- never a fault.  No LDS, no float atomics,
// no cross-lane operation: lanes of a wave may leave the loops at different times.
#pragma once
#include "smm_sddmm.hpp"
#include "smm_taper.hpp"

namespace smm {

constexpr int CV_STEPS = 4;                   // entries per lane and run
constexpr int CV_RUN = WAVE * CV_STEPS;       // consecutive entries per wave and run
enum { CV_SPHERICAL = 0, CV_EXPONENTIAL = 1, CV_GAUSSIAN = 2, CV_MATERN32 = 3, CV_MATERN52 = 4 };      // SMM_COV_* of include/smm_hip.h
constexpr int CV_WRT_NONE = -1, CV_WRT_ALL = 3;                                                          // SMM_COV_WRT_*
constexpr double CV_SQRT3 = 1.7320508075688772, CV_SQRT5 = 2.23606797749979;                             // the nearest doubles

struct CovArgs {
    int m, n, nnz;                                                    // the pattern: m x n with nnz entries
    const int *ptr; const int *idx; const double *w;
    const double *a; int64_t lda;
    const double *b; int64_t ldb;
    double len[3], variance;
    int model, wrt, scale;
    double *val, *dval;                                               // either may be NULL
    unsigned *err;
};

// The largest row r' in [r, m) with ptr[r'] <= p, given ptr[r] <= p: doubling steps from r, then bisection between the
// last two probes.  Every index read is in [1, m - 1] whatever ptr holds.
__device__ __forceinline__ int cv_row_from(const int *__restrict__ ptr, int m, int r, int p)
{
    int lo = r, step = 1, hi = r + 1;
    while (hi < m && ptr[hi] <= p) { lo = hi; step <<= 1; hi = (m - lo > step) ? lo + step : m; }
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

template <int DIM>
__device__ __forceinline__ void cv_scaled(const double (&a)[3], const double (&b)[3], const double (&len)[3], double (&u)[3], double &h2)
{
    h2 = 0.0;
    u[0] = u[1] = u[2] = 0.0;
#pragma unroll
    for (int t = 0; t < DIM; ++t) {
        u[t] = (a[t] - b[t]) / len[t];
        h2 = h2 + u[t] * u[t];
    }
}

// c = the correlation at scaled distance h (h2 = its square as summed), g = -dc/dh.  A NaN distance gives NaN in every
// model: for the spherical one neither h < 1 nor h >= 1 holds.
__device__ __forceinline__ void cv_model(int model, double h2, double h, double &c, double &g)
{
    if (model == CV_SPHERICAL) {
        if (h < 1.0) { c = ((0.5 * h) * h - 1.5) * h + 1.0; g = 1.5 - 1.5 * (h * h); }
        else if (h >= 1.0) { c = 0.0; g = 0.0; }
        else { c = h; g = h; }
        return;
    }
    const double s = model == CV_MATERN32 ? CV_SQRT3 * h : (model == CV_MATERN52 ? CV_SQRT5 * h : h);
    const double e = exp(model == CV_GAUSSIAN ? -h2 : -s);
    if (model == CV_EXPONENTIAL) { c = e; g = e; }
    else if (model == CV_GAUSSIAN) { c = e; g = (2.0 * h) * e; }
    else if (model == CV_MATERN32) { c = (1.0 + s) * e; g = (3.0 * h) * e; }
    else { c = ((1.0 + s) + (5.0 / 3.0) * h2) * e; g = (((5.0 / 3.0) * h) * (1.0 + s)) * e; }
}

__device__ __forceinline__ double cv_dlength(int wrt, double variance, double g, double h, const double (&u)[3], const double (&len)[3])
{
    if (h == 0.0) return 0.0;
    const double vg = variance * g;
    if (wrt == CV_WRT_ALL) return (vg * h) / len[0];
    const double ut = wrt == 0 ? u[0] : (wrt == 1 ? u[1] : u[2]), lt = wrt == 0 ? len[0] : (wrt == 1 ? len[1] : len[2]);
    return (vg * (ut * ut)) / (h * lt);
}

template <int DIM>
__global__ __launch_bounds__(256) void smm_cov_eval(const CovArgs A)
{
    const int lane = lane_id();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int64_t)(gridDim.x * blockDim.x / WAVE);
    const int64_t nnz = A.nnz;
    const double len[3] = {A.len[0], A.len[1], A.len[2]};
    for (int64_t base = wave * CV_RUN; base < nnz; base += nwaves * CV_RUN) {          // (uniform over the wave)
        int r = -1, p1 = 0, arow = -1;                                 // the lane's row, the end of its range, the row pa holds
        double pa[3] = {0.0, 0.0, 0.0};
        for (int s = 0; s < CV_STEPS; ++s) {
            const int64_t q = base + (int64_t)s * WAVE + lane;
            if (q >= nnz) break;
            const int p = (int)q;
            if (p >= p1) {                                             // the lane's first entry, or its row ended
                r = r < 0 ? sd_row_of(A.ptr, A.m, p) : cv_row_from(A.ptr, A.m, r, p);
                p1 = A.ptr[r + 1];
                if (p < A.ptr[r] || p >= p1) { plan_err(A.err, PLAN_ERR_COUNT, r); r = -1; p1 = 0; continue; }
            }
            const int j = A.idx[p];
            if (j < 0 || j >= A.n) { plan_err(A.err, PLAN_ERR_LIST, r); continue; }
            if (r != arow) { tp_load<DIM>(A.a + (int64_t)r * A.lda, pa); arow = r; }
            double pb[3], u[3], h2, c, g;
            tp_load<DIM>(A.b + (int64_t)j * A.ldb, pb);
            cv_scaled<DIM>(pa, pb, len, u, h2);
            const double h = sqrt(h2);
            cv_model(A.model, h2, h, c, g);
            const double w = A.scale ? A.w[p] : 1.0;
            if (A.val) {
                const double v = A.variance * c;
                A.val[p] = A.scale ? v * w : v;
            }
            if (A.dval) {
                const double d = cv_dlength(A.wrt, A.variance, g, h, u, len);
                A.dval[p] = A.scale ? d * w : d;
            }
        }
    }
}

}  // namespace smm
