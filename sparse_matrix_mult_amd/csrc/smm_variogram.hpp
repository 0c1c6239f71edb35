// smm_variogram.hpp -- kernels of smm_variogram: the empirical variogram of the values y at the points a, binned by
// distance over the stored entries e = (i, j) of a square CSR pattern: per bin the number of pairs, the sum of their
// distances h and the sum of their squared increments s.  Host driver: smm_api.hip; contract: include/smm_hip.h.
// a (n x DIM) and y (n x k) are row-major float64 with leading dimensions lda / ldy; every offset into them is 64-bit.
// The pattern may be any legal CSR (unsorted rows, repeated columns, empty rows).
//
// The contract per entry (every product rounded before its add: the library is built with -ffp-contract=off):
//   tp_d2      d2 = +0.0; df = a[i,t] - a[j,t]; d2 = d2 + df * df for t = 0 .. DIM-1; h = sqrt(d2)       (the taper's recipe)
//   vg_bin     -1 unless edges[0] <= h, else the number of q in 1 .. nb with edges[q] <= h; the entry takes part iff that
//              is in [0, nb) -- comparisons only, so a NaN distance is in no bin
//   increment  s = +0.0; dv = y[i,c] - y[j,c]; s = s + dv * dv for c = 0 .. k-1
//
// Lane map, that of smm_cov_eval on a grid of exactly VG_SLOTS lanes: the entries [0, nnz) are cut into runs of VG_RUN
// = 64 * VG_STEPS consecutive entries and the VG_SLOTS / 64 waves take runs round robin; in step s of a run lane l has
// entry base + 64 s + l.  So slot t = 64 * wave + lane owns the entries e with (e / VG_RUN) mod (VG_SLOTS / 64) = wave
// and e mod 64 = lane, and adds them in ascending e.  A lane finds the row of its first entry of a run by bisection
// of the row pointer (sd_row_of) and follows the row pointer from there (cv_row_from).
//
// Accumulators: every lane owns, per bin, two doubles and an int32 in LDS, laid out [bin][lane of the workgroup]: the
// lanes of a wave hit consecutive words whatever bins they hold (the bin stride is a multiple of 256 bytes), so the
// read-modify-write of a step is conflict-free, and no other lane ever touches a lane's slots: no atomics, no barrier
// inside the loop.  20 bytes per lane and bin: VG_BLOCK = 128 lanes x 32 bins = 80 KiB, two workgroups per compute unit,
// one wave per SIMD -- the whole grid is resident at once on 256 compute units.  The four steps of a run are unrolled
// with their loads issued together (columns, then coordinates, then values), since at one wave per SIMD nothing else
// hides a dependent load.
//
// Reduction, per bin: p[t] = p[t] + p[t + g] for every t that is a multiple of 2 g, for g = 1, 2, 4, ..., VG_SLOTS / 2.
//   g = 1 .. 32        a __shfl_down ladder: lane 0 of a wave holds exactly this tree over its 64 slots
//   g = 64 ..          the waves of a workgroup, through lane 0's own slots in LDS, by one lane per bin
//   g = VG_BLOCK ..    smm_variogram_finish: one wave per (bin, sum); lane l takes the VG_GROUPS / 64 consecutive workgroup
//                      partials from l * VG_GROUPS / 64, runs their tree in registers, then the ladder again
// Adjacent pairs at every level, so the result does not depend on VG_BLOCK.  Counts are integers: any order.
// Always-on clamps: an entry whose row is not found inside its row's range, and a column outside [0, n), is recorded in
// the context's error word (SMM_ERR_INTERNAL for the caller) and skipped -- never a fault.
#pragma once
#include "smm_cov.hpp"
#include "../../include/smm_hip.h"

namespace smm {

constexpr int VG_RUN = SMM_VG_RUN;                 // consecutive entries per wave and run
constexpr int VG_SLOTS = SMM_VG_SLOTS;             // lanes of the grid = leaves of the tree
constexpr int VG_MAX_BINS = SMM_VG_MAX_BINS;
constexpr int VG_STEPS = VG_RUN / WAVE;            // entries per lane and run
constexpr int VG_BLOCK = 128;                      // lanes per workgroup (80 KiB of LDS)
constexpr int VG_WAVES = VG_BLOCK / WAVE;
constexpr int VG_GROUPS = VG_SLOTS / VG_BLOCK;     // workgroups of the grid = partials per bin
constexpr int VG_NWAVES = VG_SLOTS / WAVE;
constexpr int VG_PER = VG_GROUPS / WAVE;           // finish: consecutive partials per lane
static_assert(VG_RUN % WAVE == 0 && VG_SLOTS % VG_BLOCK == 0 && VG_GROUPS % WAVE == 0, "the tree needs whole waves at every level");
static_assert((VG_SLOTS & (VG_SLOTS - 1)) == 0 && (VG_PER & (VG_PER - 1)) == 0 && (VG_WAVES & (VG_WAVES - 1)) == 0, "powers of two");
static_assert(VG_MAX_BINS <= VG_BLOCK && VG_MAX_BINS * VG_BLOCK * 20 <= 80 * 1024, "one lane per bin combines the waves; two workgroups per CU");

struct VgArgs {
    int n, nnz, nb;                                                   // the pattern: n x n with nnz entries; bins
    int all;                                                          // SMM_VG_ALL_ENTRIES: entries with j <= i take part too
    const int *ptr; const int *idx;
    const double *a; int64_t lda;
    const double *y; int64_t ldy, k;
    double edges[VG_MAX_BINS + 1];                                    // edges[q] = +inf for q > nb
    double *part_h, *part_s; int64_t *part_c;                         // [bin][workgroup]
    unsigned *err;
};

// The bin of distance h, or -1 / a number >= nb when it is in none.  Only constant indices into the kernel's arguments.
__device__ __forceinline__ int vg_bin(const VgArgs &A, double h)
{
    if (!(A.edges[0] <= h)) return -1;
    int b = 0;
#pragma unroll
    for (int q = 1; q <= VG_MAX_BINS; ++q) b += A.edges[q] <= h ? 1 : 0;
    return b;
}

template <int DIM>
__global__ __launch_bounds__(VG_BLOCK) void smm_variogram_bins(const VgArgs A)
{
    __shared__ double sh_h[VG_MAX_BINS * VG_BLOCK], sh_s[VG_MAX_BINS * VG_BLOCK];
    __shared__ int sh_c[VG_MAX_BINS * VG_BLOCK];
    const int tid = threadIdx.x, lane = lane_id();
    const int nb = A.nb < VG_MAX_BINS ? A.nb : VG_MAX_BINS;
    for (int b = 0; b < nb; ++b) { sh_h[b * VG_BLOCK + tid] = 0.0; sh_s[b * VG_BLOCK + tid] = 0.0; sh_c[b * VG_BLOCK + tid] = 0; }
    const int64_t wave = (int64_t)((blockIdx.x * VG_BLOCK + tid) / WAVE);
    const int64_t nnz = A.nnz;
    for (int64_t base = wave * VG_RUN; base < nnz; base += (int64_t)VG_NWAVES * VG_RUN) {          // (uniform over the wave)
        int row[VG_STEPS], col[VG_STEPS];                              // col < 0: the entry takes no part
#pragma unroll
        for (int s = 0; s < VG_STEPS; ++s) {
            const int64_t q = base + (int64_t)s * WAVE + lane;
            col[s] = q < nnz ? A.idx[q] : -1;
        }
        int r = -1, p1 = 0;                                            // the lane's row and the end of its range
#pragma unroll
        for (int s = 0; s < VG_STEPS; ++s) {
            const int64_t q = base + (int64_t)s * WAVE + lane;
            row[s] = 0;
            if (q >= nnz) continue;
            const int p = (int)q, j = col[s];
            col[s] = -1;
            if (p >= p1) {                                             // the lane's first entry, or its row ended
                r = r < 0 ? sd_row_of(A.ptr, A.n, p) : cv_row_from(A.ptr, A.n, r, p);
                p1 = A.ptr[r + 1];
                if (p < A.ptr[r] || p >= p1) { plan_err(A.err, PLAN_ERR_COUNT, r); r = -1; p1 = 0; continue; }
            }
            if (j < 0 || j >= A.n) { plan_err(A.err, PLAN_ERR_LIST, r); continue; }
            if (A.all || j > r) { row[s] = r; col[s] = j; }
        }
        double h[VG_STEPS], sq[VG_STEPS];
#pragma unroll
        for (int s = 0; s < VG_STEPS; ++s) {
            h[s] = 0.0; sq[s] = 0.0;
            if (col[s] < 0) continue;
            double pa[3], pb[3];
            tp_load<DIM>(A.a + (int64_t)row[s] * A.lda, pa);
            tp_load<DIM>(A.a + (int64_t)col[s] * A.lda, pb);
            h[s] = sqrt(tp_d2<DIM>(pa, pb));
        }
        for (int64_t c = 0; c < A.k; ++c) {
#pragma unroll
            for (int s = 0; s < VG_STEPS; ++s) {
                if (col[s] < 0) continue;
                const double dv = A.y[(int64_t)row[s] * A.ldy + c] - A.y[(int64_t)col[s] * A.ldy + c];
                sq[s] = sq[s] + dv * dv;
            }
        }
#pragma unroll
        for (int s = 0; s < VG_STEPS; ++s) {                           // ascending entries: the order of the slot's sums
            if (col[s] < 0) continue;
            const int b = vg_bin(A, h[s]);
            if (b < 0 || b >= nb) continue;
            const int o = b * VG_BLOCK + tid;
            sh_h[o] = sh_h[o] + h[s];
            sh_s[o] = sh_s[o] + sq[s];
            sh_c[o] = sh_c[o] + 1;
        }
    }
    // the tree over the wave's 64 slots, per bin; lane 0 keeps the wave's sums in its own slots
    const int w0 = tid - lane;
    for (int b = 0; b < nb; ++b) {                                     // (uniform over the wave)
        double vh = sh_h[b * VG_BLOCK + tid], vs = sh_s[b * VG_BLOCK + tid];
        int vc = sh_c[b * VG_BLOCK + tid];
        for (int g = 1; g < WAVE; g <<= 1) {
            vh = vh + __shfl_down(vh, g);
            vs = vs + __shfl_down(vs, g);
            vc = vc + __shfl_down(vc, g);
        }
        if (lane == 0) { sh_h[b * VG_BLOCK + w0] = vh; sh_s[b * VG_BLOCK + w0] = vs; sh_c[b * VG_BLOCK + w0] = vc; }
    }
    __syncthreads();
    if (tid < nb) {                                                    // the tree over the workgroup's waves, one lane per bin
        double *ph = sh_h + tid * VG_BLOCK, *ps = sh_s + tid * VG_BLOCK;
        int *pc = sh_c + tid * VG_BLOCK;
        for (int g = 1; g < VG_WAVES; g <<= 1)
            for (int t = 0; t + g < VG_WAVES; t += 2 * g) {
                ph[t * WAVE] = ph[t * WAVE] + ph[(t + g) * WAVE];
                ps[t * WAVE] = ps[t * WAVE] + ps[(t + g) * WAVE];
                pc[t * WAVE] = pc[t * WAVE] + pc[(t + g) * WAVE];
            }
        const int64_t o = (int64_t)tid * VG_GROUPS + blockIdx.x;
        A.part_h[o] = ph[0]; A.part_s[o] = ps[0]; A.part_c[o] = pc[0];
    }
}

// The remaining levels of the tree: wave `task` of the one workgroup takes bin task % nb of sum task / nb (distances,
// squared increments, counts) and writes out[0 .. nb) of it.
__global__ __launch_bounds__(1024) void smm_variogram_finish(int nb, const double *__restrict__ part_h, const double *__restrict__ part_s,
                                                             const int64_t *__restrict__ part_c, double *__restrict__ out_h,
                                                             double *__restrict__ out_s, int64_t *__restrict__ out_c)
{
    const int lane = lane_id(), wave = threadIdx.x / WAVE, nwaves = blockDim.x / WAVE;
    for (int task = wave; task < 3 * nb; task += nwaves) {             // (uniform over the wave)
        const int b = task % nb, what = task / nb;
        const int64_t o = (int64_t)b * VG_GROUPS + lane * VG_PER;
        if (what < 2) {
            const double *p = (what == 0 ? part_h : part_s) + o;
            double v[VG_PER];
#pragma unroll
            for (int i = 0; i < VG_PER; ++i) v[i] = p[i];
#pragma unroll
            for (int g = 1; g < VG_PER; g <<= 1)
#pragma unroll
                for (int t = 0; t + g < VG_PER; t += 2 * g) v[t] = v[t] + v[t + g];
            double x = v[0];
            for (int g = 1; g < WAVE; g <<= 1) x = x + __shfl_down(x, g);
            if (lane == 0) (what == 0 ? out_h : out_s)[b] = x;
        } else {
            long long x = 0;
#pragma unroll
            for (int i = 0; i < VG_PER; ++i) x += (long long)part_c[o + i];
            for (int g = 1; g < WAVE; g <<= 1) x += __shfl_down(x, g);
            if (lane == 0) out_c[b] = (int64_t)x;
        }
    }
}

}  // namespace smm
