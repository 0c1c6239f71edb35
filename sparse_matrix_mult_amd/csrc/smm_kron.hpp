// smm_kron.hpp -- kernels of the Kronecker operand Q = D (x) E (smm_kron_build, smm_kron_apply and the *_kron forms of
// smm_triple_apply / smm_innovation_solve).  Host driver: smm_api.hip; the contract is in include/smm_hip.h.
// D is p x pc, E is r x rc; row t * r + j of D (x) E is the pair (t, j), column tc * rc + jc the pair (tc, jc).
//
//   smm_kron_fill   the explicit CSR.  Row (t, j) holds len_D(t) * len_E(j) entries at the closed-form position
//                   D.ptr[t] * nnz(E) + len_D(t) * E.ptr[j]: no count pass, no scan, no atomics.  A group of G lanes takes
//                   a row; a lane takes four consecutive entries whose position in the output is a multiple of four and
//                   writes them as one 16-byte store of columns and two of values (a row's ragged head and tail go out
//                   entry by entry).  Entry q of the row is (a, b) = (q / len_E, q % len_E), computed once per lane and
//                   pass and stepped from there.
//   smm_kron_inner  U = (I (x) E) X in ONE launch: a group of G lanes takes a row j of E and owns the pc * k elements
//                   U[(tc, j), c] -- tc-major "virtual columns" v = tc * k + c -- so the row's (column, value) pairs are
//                   loaded once per tile of G * VEC virtual columns and serve every tc; at k = 1 the lanes of a group
//                   are pc different blocks of X, not idle.  Any row length: the group walks the whole row in stored
//                   order in both modes (lanes own elements, nothing is split), which is what makes default-mode
//                   results independent of the column blocking.
//   smm_kron_outer  Y = (D (x) I) U: a streaming kernel.  A workgroup takes row t of D and 256 * VEC consecutive elements
//                   of the contiguous (j, c) span of r * k; a lane owns VEC of them.  Row t's entries of D are uniform
//                   over the workgroup (scalar loads); every load of U is contiguous across the lanes.  Each element
//                   of U is read once per entry of D's column (a variant that read it once, through an LDS tile of all pc
//                   slabs, was measured and lost: DESIGN.md section 16).
// Order of the sums: SMM_EXACT adds one rounded product at a time in stored order; default mode uses fused multiply-adds
// in the same order.  No float atomics and no cross-lane reduction anywhere, so every result is bitwise reproducible.
// Always-on clamps, as in smm_spmm.hpp: a row range outside [0, nnz) and a column outside its factor's range are
// recorded in the context's error word (SMM_ERR_INTERNAL for the caller) and skipped -- never a fault.
#pragma once
#include "smm_spmm.hpp"

namespace smm {

struct KronArgs {
    int p, pc, r, rc;                                                 // D: p x pc, E: r x rc
    int nnz_d, nnz_e;
    const int *dptr; const int *didx; const double *dval;
    const int *eptr; const int *eidx; const double *eval;
    int64_t k, ldx, ldy;                                              // apply: X (pc * rc) x k, Y (p * r) x k
    const double *x; double *u; double *y;                            // U: (pc * r) x k, packed (leading dimension k)
    int *optr; int *oidx; double *oval;                               // build: the three arrays of D (x) E
    unsigned *err;
};

// Entry range of a factor's row, clamped (an inconsistent range is recorded and read as empty).
__device__ __forceinline__ void kr_row(const int *ptr, int nnz, int row, unsigned *err, int &p0, int &len)
{
    p0 = ptr[row];
    const int p1 = ptr[row + 1];
    len = p1 - p0;
    if (p0 < 0 || p1 < p0 || p1 > nnz) { plan_err(err, PLAN_ERR_COUNT, row); p0 = 0; len = 0; }
}

// ------------------------------------------------------------------------------ build
template <int G>
__global__ __launch_bounds__(256) void smm_kron_fill(const KronArgs A)
{
    constexpr int RPW = WAVE / G;
    const int gl = lane_id() & (G - 1);
    const int64_t rows = (int64_t)A.p * A.r;
    const int64_t group = (int64_t)(blockIdx.x * blockDim.x + threadIdx.x) / G, ngroups = (int64_t)gridDim.x * blockDim.x / G;
    static_assert(RPW >= 1, "group");
    for (int64_t ro = group; ro < rows; ro += ngroups) {
        const int t = (int)(ro / A.r), j = (int)(ro % A.r);
        int d0, ld, e0, le;
        kr_row(A.dptr, A.nnz_d, t, A.err, d0, ld);
        kr_row(A.eptr, A.nnz_e, j, A.err, e0, le);
        const int64_t base = (int64_t)d0 * A.nnz_e + (int64_t)ld * e0, L = (int64_t)ld * le;
        if (gl == 0) {
            A.optr[ro] = (int)base;
            if (ro == rows - 1) A.optr[rows] = (int)(base + L);
        }
        if (L == 0) continue;
        // chunks of four entries at output positions that are multiples of four: [s, s + 4) with s = c0 + 4 * chunk
        const int64_t c0 = base & ~(int64_t)3, end = base + L;
        for (int64_t s = c0 + 4 * (int64_t)gl; s < end; s += 4 * G) {
            int64_t q = s - base;                                     // (negative in the row's first chunk)
            const int u0 = q < 0 ? (int)-q : 0, u1 = (int)(end - s < 4 ? end - s : 4);
            q += u0;
            int a = (int)(q / le), b = (int)(q % le);
            int col[4] = {0, 0, 0, 0};
            double val[4] = {0.0, 0.0, 0.0, 0.0};
            int dc = A.didx[d0 + a];
            double dv = A.dval[d0 + a];
            if (dc < 0 || dc >= A.pc) { plan_err(A.err, PLAN_ERR_LIST, t); dc = 0; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (u < u0 || u >= u1) continue;
                int ec = A.eidx[e0 + b];
                if (ec < 0 || ec >= A.rc) { plan_err(A.err, PLAN_ERR_LIST, j); ec = 0; }
                col[u] = dc * A.rc + ec;                              // (< pc * rc < 2^31 - 1: checked by the host)
                val[u] = dv * A.eval[e0 + b];                         // one rounded multiply
                if (++b == le && u + 1 < u1) {
                    b = 0; ++a;
                    dc = A.didx[d0 + a]; dv = A.dval[d0 + a];
                    if (dc < 0 || dc >= A.pc) { plan_err(A.err, PLAN_ERR_LIST, t); dc = 0; }
                }
            }
            if (u0 == 0 && u1 == 4) {
                *reinterpret_cast<int4 *>(A.oidx + s) = make_int4(col[0], col[1], col[2], col[3]);
                *reinterpret_cast<double2 *>(A.oval + s) = make_double2(val[0], val[1]);
                *reinterpret_cast<double2 *>(A.oval + s + 2) = make_double2(val[2], val[3]);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u >= u0 && u < u1) { A.oidx[s + u] = col[u]; A.oval[s + u] = val[u]; }
            }
        }
    }
}

// ------------------------------------------------------------------------------ apply, E-step: U = (I (x) E) X
// Groups of G lanes per row j of E, 64 / G rows per wave.  Lane gl of a group owns the virtual columns v0 + gl * VEC ..
// + VEC of the tile v0 (VEC == 2: k even, so a pair never straddles two blocks tc).  Per batch the group's lanes load G
// consecutive (column, value) pairs of the row and every pair is broadcast in stored order, as smm_spmm_group does.
template <int G, int VEC, bool EXACT>
__global__ __launch_bounds__(256) void smm_kron_inner(const KronArgs A)
{
    constexpr int RPW = WAVE / G, TW = G * VEC;
    const int lane = lane_id(), gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE), nwaves = (int)(gridDim.x * blockDim.x / WAVE);
    const int64_t W = (int64_t)A.pc * A.k;
    for (int64_t j0 = (int64_t)wave * RPW; j0 < A.r; j0 += (int64_t)nwaves * RPW) {  // (uniform over the wave)
        const int j = (int)j0 + lane / G;
        int e0 = 0, len = 0;
        if (j < A.r) kr_row(A.eptr, A.nnz_e, j, A.err, e0, len);
        int wlen = len;
        for (int o = G; o < WAVE; o <<= 1) wlen = max(wlen, __shfl_xor(wlen, o));
        for (int64_t v0 = 0; v0 < W; v0 += TW) {                                     // (uniform over the wave)
            const int64_t v = v0 + (int64_t)gl * VEC;
            const bool own = j < A.r && v < W;
            const int64_t tc = own ? v / A.k : 0, c = own ? v % A.k : 0;
            const double *xb = A.x + tc * A.rc * A.ldx + c;
            double acc[VEC];
#pragma unroll
            for (int u = 0; u < VEC; ++u) acc[u] = 0.0;
            for (int b = 0; b < wlen; b += G) {                       // (uniform over the wave)
                const int e = b + gl;
                int cl_own = -1;
                double vl_own = 0.0;
                if (e < len) {
                    cl_own = A.eidx[e0 + e];
                    vl_own = A.eval[e0 + e];
                    if (cl_own < 0 || cl_own >= A.rc) { plan_err(A.err, PLAN_ERR_LIST, j); cl_own = -1; }
                }
#pragma unroll 8
                for (int l = 0; l < G; ++l) {
                    const int cl = sp_bcast<G == WAVE>(cl_own, gbase + l);
                    const double vl = sp_bcast<G == WAVE>(vl_own, gbase + l);
                    if (cl >= 0 && own) sp_axpy<VEC, EXACT>(acc, vl, xb + (int64_t)cl * A.ldx);
                }
            }
            if (own) sp_store<VEC>(A.u + (tc * A.r + j) * A.k + c, acc);
        }
    }
}

// ------------------------------------------------------------------------------ apply, D-step: Y = (D (x) I) U
// One workgroup per (row t of D, chunk of 256 * VEC elements of the span r * k); VEC == 2: k and ldy even, Y 16-byte aligned.
template <int VEC, bool EXACT>
__global__ __launch_bounds__(256) void smm_kron_outer(const KronArgs A, int64_t chunks)
{
    const int64_t S = (int64_t)A.r * A.k, items = (int64_t)A.p * chunks;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {                      // (uniform over the block)
        const int t = (int)(it / chunks);
        const int64_t e = ((it % chunks) * 256 + threadIdx.x) * VEC;
        int d0, ld;
        kr_row(A.dptr, A.nnz_d, t, A.err, d0, ld);
        if (e >= S) continue;
        const double *ub = A.u + e;
        double acc[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) acc[u] = 0.0;
#pragma unroll 4
        for (int a = 0; a < ld; ++a) {
            const int tc = A.didx[d0 + a];
            if (tc < 0 || tc >= A.pc) { plan_err(A.err, PLAN_ERR_LIST, t); continue; }
            sp_axpy<VEC, EXACT>(acc, A.dval[d0 + a], ub + (int64_t)tc * S);
        }
        const int64_t j = e / A.k, c = e % A.k;
        sp_store<VEC>(A.y + ((int64_t)t * A.r + j) * A.ldy + c, acc);
    }
}

}  // namespace smm
