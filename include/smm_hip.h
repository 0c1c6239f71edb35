/*
 * smm_hip.h -- C ABI of libsmm_hip.so, the MI355X (gfx950) engine behind
 * sparse_matrix_multiply().  Plain C: pointers and sizes only, no C++/torch types.
 *
 * Two layers are exported by the same library:
 *
 *  (1) The LEGACY entry points the reference's Python wrapper binds by name
 *      (reference sparse_matrix_mult/matrix_ops.py:147-171, call sites :195,333,346,348,
 *      360,362,336,351,365; declarations include/functions.h:43-84).  Struct layout is the
 *      one that wrapper declares -- `int` dims (matrix_ops.py:26-33: 40-byte sparsemat,
 *      :44-48: 16-byte darray) -- NOT the size_t layout of include/matrix_def.h at HEAD
 *      (SURVEY F1).  Host arrays in, libc-malloc'd host arrays out, freed by destroy_*.
 *
 *  (2) The v2 API our own matrix_ops.py, bench.py and the multi-GPU driver call: operands
 *      live in HBM behind opaque handles, results are written into caller-owned DEVICE (or
 *      host) buffers, row pointers / nnz are int64 (nnz(C) of the 50k x 50k d=0.01 config
 *      is 2.48e9 > INT32_MAX), every call returns 0 or a negative smm_status and
 *      smm_last_error() gives the message.  Nothing here falls back to a CPU path: with no
 *      usable GPU every compute entry point fails with SMM_ERR_NO_DEVICE.
 */
#ifndef SMM_HIP_H
#define SMM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status / flags */
enum smm_status {
    SMM_OK = 0,
    SMM_ERR_NO_DEVICE = -1,   /* no gfx950 device visible / HIP init failed            */
    SMM_ERR_INVALID   = -2,   /* bad argument, shape mismatch, malformed CSR            */
    SMM_ERR_ALLOC     = -3,   /* hipMalloc / malloc failed                              */
    SMM_ERR_HIP       = -4,   /* a HIP runtime call or kernel launch failed             */
    SMM_ERR_OVERFLOW  = -5,   /* result does not fit the legacy int32 ABI               */
    SMM_ERR_UNSUPPORTED = -6, /* the device does not behave as SMM_EXACT needs (smm_ctx_exact_selftest) */
    SMM_ERR_INTERNAL  = -7    /* inconsistent plan metadata caught by a kernel's bounds clamp or by the plan
                                 checker: a defect of this library, reported instead of a hang or a fault
                                 (reference convention: message + early return, src/sparsework.cpp:33-36,
                                 src/sparse_sparse_sparse.cpp:257-262)                                   */
};

enum smm_flags {
    SMM_SYMMETRIC   = 1,  /* keep only i <= col   (sparsework.cpp:217, sparse_sparse_dense.cpp:59) */
    SMM_FULL_MATRIX = 2,  /* triple_product compute_full_matrix=1 (sparse_sparse_dense.cpp:201,213) */
    SMM_MIRROR      = 8,  /* mirror epilogue (not in the reference): after an upper-triangle result -- dense with
                             SMM_SYMMETRIC, or the triple product without SMM_FULL_MATRIX -- the lower triangle
                             is filled with the mirror image of the upper one, i.e. the full symmetric matrix
                             (what compute_full_matrix=1 was meant to give; SMM_FULL_MATRIX reproduces its
                             doubling bug instead).  Whole square results only.                          */
    SMM_TRANSPOSE   = 16, /* op(A) = A^T in the sparse x dense product (smm_spmm* only)                      */
    SMM_SCALE_BY_MASK = 32, /* smm_sddmm* only: multiply each result by the mask's stored value                 */
    SMM_EXACT       = 4   /* add every product in exactly the reference's order: float64 values
                             are then bit-identical to the CPU loop, for any legal CSR operand (B with
                             unsorted rows or repeated columns takes an ordered read-modify-write
                             path instead of the tile kernels: exact, not fast).  Without it the numeric phase lets the waves of a workgroup
                             add concurrently (LDS atomics): values agree to rounding -- tested
                             to the north star's 1e-10 relative -- and the kernel is ~3x faster.
                             indptr / indices are bit-exact in both modes.                     */
};

typedef struct smm_ctx  smm_ctx;   /* one device + one stream + a workspace arena        */
typedef struct smm_csr  smm_csr;   /* a CSR operand resident in HBM (+ cached tile index) */
typedef struct smm_plan smm_plan;  /* result of the symbolic phase of one product         */

/* ------------------------------------------------------------------ context
 * A context owns one device, one stream and a workspace pool.  Every entry point takes the
 * context's lock, so host threads may share one context (their calls serialise; the reference's
 * library has no global state and is called with the GIL released, matrix_ops.py:136).
 * Handles (smm_csr, smm_plan) belong to the context that made them; a plan borrows its two
 * operands, which must stay alive until the plan is destroyed. */
int         smm_device_count(void);              /* number of usable devices, 0 if none  */
const char *smm_last_error(void);                /* thread-local message of the last failure */
/* hip_stream: a hipStream_t to launch on, NULL for a non-blocking stream the context creates and
 * owns, or SMM_STREAM_DEFAULT for the device's null stream (what torch's default stream is:
 * torch.cuda.current_stream().cuda_stream == 0 -- pass SMM_STREAM_DEFAULT for it, not NULL).
 * Device buffers handed to smm_csr_from_device must be complete on that stream (or the
 * caller synchronises first): the library orders its work only against its own stream. */
#define SMM_STREAM_DEFAULT ((void *)(intptr_t)-1)
int  smm_ctx_create(int device, void *hip_stream, smm_ctx **out);
void smm_ctx_destroy(smm_ctx *ctx);
/* Waits for the context's stream and reports what the kernels recorded since the last report: SMM_ERR_INTERNAL when
 * a numeric kernel met inconsistent plan metadata (see smm_plan_check) -- the way an error of the asynchronous
 * smm_spgemm_numeric reaches the caller. */
int  smm_ctx_synchronize(smm_ctx *ctx);
/* 1: every smm_spgemm_symbolic ends with smm_plan_check (also: env SMM_CHECK=1 when the context is created).  Off by
 * default: the checker streams the ordered lists once more (~2 ms at 50k x 50k); the kernels' own clamps are always on. */
int  smm_ctx_set_check(smm_ctx *ctx, int enable);
/* The context keeps freed scratch (the lists and tables of destroyed plans, result staging) in a pool for reuse.
 * smm_ctx_release_pool returns the pool's free blocks to the device (matrix_ops.clear_cache() calls it);
 * smm_ctx_pool_bytes says how much is held.  Every allocation that fails flushes the pool and retries once by itself.
 * smm_ctx_live_bytes is the total of the pool blocks handed out: those of open plans and results only, once every
 * call has returned -- whether it succeeded or failed. */
int     smm_ctx_release_pool(smm_ctx *ctx);
int64_t smm_ctx_pool_bytes(smm_ctx *ctx);
int64_t smm_ctx_live_bytes(smm_ctx *ctx);
/* TEST HOOK: the nth device allocation from now fails -- its first attempt only (the library's own flush-and-retry
 * must make the call succeed), or with hard != 0 both attempts (the call returns SMM_ERR_ALLOC).  smm_ctx_alloc_retries
 * counts the allocations that needed the retry. */
int     smm_ctx_inject_alloc_failure(smm_ctx *ctx, int nth, int hard);
int64_t smm_ctx_alloc_retries(smm_ctx *ctx);
/* Per-kernel timing with HIP events on the context's stream (bench.py's roofline leg).
 * enable=1 starts recording; smm_ctx_kernel_time returns the accumulated milliseconds and
 * launch count of the named kernel since the last reset (name as printed by rocprofv3,
 * without template arguments: "smm_numeric", "smm_symbolic", ...). */
int  smm_ctx_timing(smm_ctx *ctx, int enable);
int  smm_ctx_timing_reset(smm_ctx *ctx);
int  smm_ctx_kernel_time(smm_ctx *ctx, const char *kernel, double *ms_total, int64_t *launches);
/* Tuning knobs (0 keeps the default): LDS accumulator columns per workgroup (x 8 bytes of
 * LDS; default 20000 = one workgroup per CU) and waves per workgroup of the numeric kernels.
 * In SMM_EXACT mode results do not depend on them, bit for bit. */
int  smm_ctx_tune(smm_ctx *ctx, int lds_cols, int waves);             /* SMM_EXACT walk          */
int  smm_ctx_tune_shared(smm_ctx *ctx, int lds_cols, int waves);      /* default walk (4/8/16)   */
/* Rows of C with at most small_max (<= 256) / medium_max (<= 2048) nonzeros are accumulated in an
 * LDS hash table (one wave / one workgroup per row) instead of dense LDS tiles; 0, 0 turns the
 * hash kernels off.  Defaults 256 / 2048. */
int  smm_ctx_tune_hash(smm_ctx *ctx, int small_max, int medium_max);
/* Row-block x column-slab numeric kernels (B's gather served by the XCD's L2; values always in the
 * reference's order).  mode 0 = used where they pay (default), 1 = never, 2 = wherever they can run;
 * ws = slab width in columns (0 = sized so that one slab of B is L2-resident); rows_per_wave 2 or 4
 * (0 keeps the setting).  Results do not depend on any of it beyond default-mode rounding. */
int  smm_ctx_tune_slab(smm_ctx *ctx, int mode, int ws, int rows_per_wave);
/* 1 (default): products whose B has < 65535 columns run the symbolic phase on uint16 -- a 16-bit copy of
 * B's column indices (cached on the operand) and 16-bit ordered lists: half the bytes of that phase's gather
 * and of the list traffic.  0: always int32.  Results are identical. */
int  smm_ctx_tune_narrow(smm_ctx *ctx, int enable);
/* The symbolic phase walks B as a chunk-padded stream of 16-bit columns, one column slab of at most
 * max_slab_cols columns at a time (0 = the default, 63 456: products whose B has fewer columns are one slab).  A
 * wider B is walked slab by slab -- every (slab, row) has its own ordered list, the numeric phase reads them
 * through a table of (source, length, destination) sub-runs -- which keeps the marker bitmaps small (many waves
 * per CU) and the lists 16-bit at any width.  Results do not depend on it, bit for bit. */
int  smm_ctx_tune_symbolic(smm_ctx *ctx, int max_slab_cols);
/* Symbolic walk for operands B with dense runs of columns (bands, blocks): 0 never, 1 (default) chosen per operand from the
   share of neighbouring entries that fall into one 32-column word of the marker bitmap, 2 always.  Results never depend on it. */
int  smm_ctx_tune_dense_runs(smm_ctx *ctx, int mode);
/* Triple product, stage 2: ring != 0 selects the ring kernel of round 4 (the tile of T as a ring of column pieces, the
 * waves of a workgroup synchronised by progress words in LDS instead of barriers: csrc/smm_ring.hpp), 0 (default) the
 * chunk kernel.  Results are identical (bit for bit under SMM_EXACT); the ring is the slower of the two on MI355X
 *  and is kept as a tested alternative.  Also: env SMM_S2_RING=1 when the context is created. */
int  smm_ctx_tune_stage2(smm_ctx *ctx, int ring);
/* B's packed payload for the CSR product's piece walk: 1 = 1.5-byte columns ("pack12") where that is smaller (default),
   0 = 16-bit columns always, 2 = pack12 wherever the four-entries-per-lane walk applies.  Results never depend on it. */
int  smm_ctx_tune_pack(smm_ctx *ctx, int mode);
/* Where pack12 is chosen: its pieces at a fixed stride (the longest piece's size, a multiple of 128 bytes), addressed by
   (tile, row) with a 2-byte length table instead of the 8-byte descriptors.  1 = where the strided payload is at most 1.5
   times the compact one (default), 0 = never, 2 = wherever pack12 is chosen and the payload stays below 2^31 units.
   Results never depend on it.  Also: env SMM_PACK_STRIDE when the context is created. */
int  smm_ctx_tune_pack_stride(smm_ctx *ctx, int mode);
/* Run-time guard of SMM_EXACT.  The exact walk adds the products of one wave-instruction that fall on the same
 * accumulator in ascending lane order (the reference's order, src/sparsework.cpp:59-76) -- a property of
 * gfx950's ds_add_f64 that was measured, not one the ISA promises.  This runs a sub-millisecond kernel that
 * checks exactly that (random groupings of lanes on addresses, values of many magnitudes, compared bit for
 * bit with the sum taken lane by lane) and fails with SMM_ERR_UNSUPPORTED where it does not hold.  Every
 * context runs it by itself before its first SMM_EXACT product; inject_fault != 0 makes the check compare
 * against the DESCENDING lane order instead, i.e. exercises the failure path (tests). */
int  smm_ctx_exact_selftest(smm_ctx *ctx, int inject_fault);

/* ------------------------------------------------------------------ operands
 * Replaces create_sparsemat + the three memmoves of csr_to_sparsemat
 * (matrix_ops.py:187-202; src/memfunctions.cpp:117-131).  indptr/indices are int32 as in
 * the reference (`int* rowPtr, colInd`, include/matrix_def.h:21-22); nnz < 2^31.
 * The CSR is validated on the device (monotone indptr, indices in range); a malformed
 * operand is rejected with SMM_ERR_INVALID instead of faulting a kernel. */
int  smm_csr_from_host(smm_ctx *ctx, int64_t rows, int64_t cols, int64_t nnz,
                       const int32_t *indptr, const int32_t *indices, const double *data,
                       smm_csr **out);
/* Borrow arrays already in HBM (no copy; they must outlive the handle). */
int  smm_csr_from_device(smm_ctx *ctx, int64_t rows, int64_t cols, int64_t nnz,
                         const int32_t *d_indptr, const int32_t *d_indices, const double *d_data,
                         smm_csr **out);
void smm_csr_destroy(smm_csr *m);
int64_t smm_csr_rows(const smm_csr *m);
int64_t smm_csr_cols(const smm_csr *m);
int64_t smm_csr_nnz(const smm_csr *m);
/* Values-only update of an operand whose sparsity pattern stays (the reference re-marshals all three arrays
 * on every call, matrix_ops.py:187-202,339-340; the README's use case -- covariance products, README.md:5,13 --
 * repeats one pattern with new values).  `data`: nnz doubles in HOST memory, copied over the operand's values
 * in HBM; every cached copy that holds values (packed tile payload, slab-major copy, sliced-ELL copy of H) is
 * refreshed in place, so plans made on this operand stay valid and smm_spgemm_numeric can simply be run
 * again on them: a product with an unchanged pattern costs the numeric phase only.
 * _device: the new values are already in HBM at d_data (copied, for operands made by smm_csr_from_host), or
 * d_data is NULL / the operand's own borrowed array, which the caller has rewritten in place (operands made
 * by smm_csr_from_device): only the cached copies are refreshed.  The stream rule of smm_csr_from_device applies to the
 * values: the refresh is queued on the context's stream without a wait of the host, so they must be complete on that
 * stream, or the caller synchronises first. */
int  smm_csr_update_values(smm_ctx *ctx, smm_csr *m, const double *data);
int  smm_csr_update_values_device(smm_ctx *ctx, smm_csr *m, const double *d_data);
/* A^T as a new operand owned by the caller (smm_csr_destroy), built on the device: its arrays are exactly those of
 * scipy's a.tocsc() -- row j of A^T holds A's entries of column j in ascending source-row order, entries of one source
 * row in their stored order; repeated columns stay repeated, values are copied bit for bit.  Any column length. */
int  smm_csr_transpose(smm_ctx *ctx, const smm_csr *a, smm_csr **out);
/* Host copy of an operand's own arrays: indptr (rows+1 int32), indices (nnz int32), data (nnz float64). */
int  smm_csr_download(smm_ctx *ctx, const smm_csr *m, int32_t *indptr, int32_t *indices, double *data);
/* The same three arrays copied into caller-owned DEVICE buffers of those sizes (a NULL destination is skipped): the
 * pattern of a library-owned operand for a caller that keeps its results in HBM.  Synchronises the context's stream. */
int  smm_csr_copy_device(smm_ctx *ctx, const smm_csr *m, int32_t *d_indptr, int32_t *d_indices, double *d_data);
/* HBM held by the handle: its arrays (when owned) plus every cached copy. */
int64_t smm_csr_device_bytes(const smm_csr *m);
/* 64-bit content hash of a HOST buffer (no GPU involved): a chain of bijective mixing steps, so changing any
 * one 8-byte word always changes the result; large buffers are hashed by several threads.  matrix_ops.py keys
 * its operand cache on it -- a full-content check, so an operand edited in place is never served stale. */
uint64_t smm_host_hash64(const void *p, int64_t bytes);
/* 1 when every row has strictly increasing column indices (scipy "canonical" CSR). */
int  smm_csr_is_canonical(smm_ctx *ctx, smm_csr *m);
/* products[i] = sum over nonzeros (i,r) of A of nnz(B[r,:]) -- the work measure used to
 * balance contiguous row shards across GPUs (replaces limits(), src/workdivision.cpp:16-89,
 * which balances row counts).  Host output, a.rows entries. */
int  smm_row_products(smm_ctx *ctx, const smm_csr *a, const smm_csr *b, int64_t *products_host);

/* ------------------------------------------------------------------ CSR x CSR -> CSR
 * Replaces sparse_nosym / sparse_sym (src/sparse_sparse_sparse.cpp:172-299 / :41-155) and
 * the row kernels sparsework_nosym / sparsework_sym (src/sparsework.cpp:12-149 / :156-300).
 * Two phases, as the reference's count-then-stitch driver: symbolic produces per-row counts
 * and the first-touch-ordered column lists and returns nnz(C); the caller allocates
 * c_indices / c_data (device) of that size; numeric fills indptr (int64, a.rows+1),
 * indices (int32, reference order) and data.
 * a_row_offset: global index of A's row 0 when A is one contiguous row shard of a larger
 * matrix (only the SMM_SYMMETRIC filter i <= col looks at it).
 * The stream rule of smm_csr_from_device applies to the output buffers of smm_spgemm_numeric: it fills them on the
 * context's stream and may return before they are complete, so nothing on another stream may still use them when it is
 * called, and the caller orders its reads behind that stream (smm_ctx_synchronize, which also reports a plan error). */
int  smm_spgemm_symbolic(smm_ctx *ctx, smm_csr *a, smm_csr *b, int flags, int64_t a_row_offset,
                         smm_plan **plan, int64_t *nnz_out);
int  smm_spgemm_numeric(smm_ctx *ctx, smm_plan *plan,
                        int64_t *d_c_indptr, int32_t *d_c_indices, double *d_c_data);
/* Same, results copied into host buffers (numpy arrays owned by the caller). */
int  smm_spgemm_numeric_host(smm_ctx *ctx, smm_plan *plan,
                             int64_t *c_indptr, int32_t *c_indices, double *c_data);
/* The same with int64 column indices in the host array (widened while the chunks are copied out): for
 * results with nnz >= 2^31, where a scipy CSR needs indptr and indices of one (64-bit) dtype -- which
 * the reference's int32 structs cannot represent at all. */
int  smm_spgemm_numeric_host_i64(smm_ctx *ctx, smm_plan *plan,
                                 int64_t *c_indptr, int64_t *c_indices, double *c_data);
/* Only the int64 row pointer of the planned product (device->host, a.rows+1 entries). */
int  smm_plan_indptr_host(smm_ctx *ctx, smm_plan *plan, int64_t *c_indptr);
/* Verify every invariant of the plan that the numeric phase relies on (list capacities non-negative and not
 * overlapping, row counts = row pointer, start slots monotone, list entries in range, sub-run tables consistent with
 * the lists, tile by tile) on the device.  SMM_OK, or SMM_ERR_INTERNAL with the first offending row in
 * smm_last_error().  The numeric kernels additionally clamp everything they read from a plan, always: a table that
 * slipped through can cost a row its values, never a store outside the row, a hang or a fault. */
int  smm_plan_check(smm_ctx *ctx, smm_plan *plan);
/* TEST HOOK: damage one piece of the plan's metadata in HBM (kind 1..8: reversed / out-of-row sub-run, tail
 * descriptor, row count, list entry, slab sub-run, start slot, negative capacity) so that the error path above can
 * be exercised; the plan is to be destroyed afterwards. */
int  smm_plan_inject_fault(smm_ctx *ctx, smm_plan *plan, int kind);
int64_t smm_plan_nnz(const smm_plan *plan);
int64_t smm_plan_device_bytes(const smm_plan *plan);   /* HBM scratch the plan holds (lists, sub-run table, ...) */
void smm_plan_destroy(smm_plan *plan);

/* CSR mirror epilogue (not in the reference, opt-in): callers of symmetric=True get only i <= col
 * (src/sparsework.cpp:217).  These two calls turn such an n x n upper-triangle CSR, resident in HBM, into the full
 * symmetric matrix, in HBM: _symbolic writes the full row pointer (n+1 entries) and returns the full nnz, the
 * caller allocates, _fill writes indices and values.  Order inside row i of the full matrix: first the mirrored
 * entries (columns j < i) in ascending column order, then the row's own entries in the order the input holds them
 * (the reference's first-touch order).  Any row length: mirrored segments of up to 8192 entries are sorted in LDS,
 * longer ones (results as full as the BASELINE configs') are placed by rank -- the columns of a segment are distinct,
 * so an entry's sorted position is the number of set bits below its column in a bitmap of the segment.  Entries left
 * of the diagonal in the input are refused with SMM_ERR_INVALID.
 * An input without entries: _symbolic reads d_indices only through the row pointer, so it may be NULL there; it writes
 * n+1 zeros and returns nnz_full = 0, and that row pointer IS the result.  _fill has nothing to do then and is not to be
 * called: for n > 0 it refuses a NULL d_indices, d_data, d_full_indices or d_full_data with SMM_ERR_INVALID ("NULL CSR
 * array") whatever the row pointers say, without reading them.  A caller whose buffers of zero elements have no address
 * (Context.spgemm_mirrored_torch) returns the zero row pointer and two empty arrays itself. */
int  smm_csr_mirror_symbolic(smm_ctx *ctx, int64_t n, const int64_t *d_indptr, const int32_t *d_indices,
                             int64_t *d_full_indptr, int64_t *nnz_full);
int  smm_csr_mirror_fill(smm_ctx *ctx, int64_t n, const int64_t *d_indptr, const int32_t *d_indices, const double *d_data,
                         const int64_t *d_full_indptr, int32_t *d_full_indices, double *d_full_data);

/* ------------------------------------------------------------------ CSR x CSR -> dense
 * Replaces dense_nosym / dense_sym (src/sparse_sparse_dense.cpp:79-131 / :13-74).
 * d_c: a.rows x b.cols row-major float64 in HBM; every element is written (cells the
 * reference leaves at calloc's 0.0 are written as 0.0). */
int  smm_spgemm_dense(smm_ctx *ctx, smm_csr *a, smm_csr *b, int flags, int64_t a_row_offset,
                      double *d_c);
int  smm_spgemm_dense_host(smm_ctx *ctx, smm_csr *a, smm_csr *b, int flags, int64_t a_row_offset,
                           double *c);

/* ------------------------------------------------------------------ H * Q * H^T
 * Replaces triple_product (src/sparse_sparse_dense.cpp:141-249).  Rows
 * [row_begin,row_end) of the n x n result are computed; d_c points at row row_begin of a
 * row-major buffer with leading dimension n.  Without SMM_FULL_MATRIX only k >= i is
 * computed and the rest of each row is written as 0.0.  With SMM_FULL_MATRIX the whole
 * range must be [0,n) and the reference's behaviour is reproduced exactly: every
 * off-diagonal cell holds S[i,k] + S[k,i]. */
int  smm_triple_product(smm_ctx *ctx, smm_csr *h, smm_csr *q, int flags,
                        int64_t row_begin, int64_t row_end, double *d_c);
int  smm_triple_product_host(smm_ctx *ctx, smm_csr *h, smm_csr *q, int flags,
                             int64_t row_begin, int64_t row_end, double *c);

/* ------------------------------------------------------------------ H * Q * H^T, sparse output
 * The triple product as a CSR held in HBM by the library (not in the reference, whose triple product is dense only:
 * an n x n array caps n near 1e5 on one device).  Rows [row_begin,row_end) of S = H * Q * H^T; each row holds the
 * columns k >= i only, in strictly ascending order (canonical CSR).
 *   Pattern (structural, never value-based): (i,k) is stored iff some j is stored both in row i of T = H * Q (the
 *   SpGEMM pattern of smm_spgemm_symbolic) and in row k of H.  Entries that cancel to 0.0 are stored.
 *   Values with SMM_EXACT: bit-identical to what smm_triple_product (dense, without SMM_FULL_MATRIX) writes at (i,k) --
 *   the reference's loop sum = 0.0; sum += T[i, H.col[jp]] * H.val[jp] over row k of H in stored order
 *   (sparse_sparse_dense.cpp:201-211), T's unstored entries read as +0.0 -- for any legal H (unsorted rows, repeated
 *   columns).  Without it: within 1e-10 relative of those numbers (fused multiply-adds).
 *   SMM_FULL_MATRIX (whole range [0,n) only): the full symmetric matrix, the upper triangle mirrored by
 *   smm_csr_mirror_symbolic / _fill -- deliberately NOT the reference's compute_full_matrix=1 (S[i,k] + S[k,i] off the
 *   diagonal), which smm_triple_product keeps reproducing.  Rows stay ascending.  SMM_MIRROR is refused.
 * Nothing of size n x n or n x K is allocated: H is taken in row blocks whose T fits smm_ctx_tune_triple_sparse's
 * budget, so nnz(H * Q) beyond 2^31 in total is fine.  Peak HBM: the operands, H^T (cached on H's handle, built by
 * smm_csr_transpose; it depends on the pattern only, so smm_csr_update_values does not invalidate it), one block's
 * T and its stage-2 scratch, and the result. */
typedef struct smm_result smm_result;   /* a CSR result held in HBM by the library; belongs to the context */
int  smm_triple_product_sparse(smm_ctx *ctx, smm_csr *h, smm_csr *q, int flags, int64_t row_begin, int64_t row_end,
                               smm_result **out);
int64_t smm_result_nnz(const smm_result *r);
int64_t smm_result_rows(const smm_result *r);           /* row_end - row_begin of the call that made it */
/* Host copy: indptr (rows+1 int64), indices (int32 with index_bytes 4, int64 with 8 -- what a scipy CSR with
 * nnz >= 2^31 needs), data (nnz float64). */
int  smm_result_download(smm_ctx *ctx, smm_result *r, int64_t *indptr, void *indices, int index_bytes, double *data);
/* Device copy into caller-owned HBM buffers of the same sizes (int32 indices). */
int  smm_result_copy_device(smm_ctx *ctx, smm_result *r, int64_t *d_indptr, int32_t *d_indices, double *d_data);
void smm_result_destroy(smm_result *r);
/* Row-block budget of smm_triple_product_sparse: entries of T = H[b] * Q per block, counted as products (an upper
 * bound of them); 0 = the default, 2^27.  A block holds at least one row.  Results do not depend on it, bit for bit. */
int  smm_ctx_tune_triple_sparse(smm_ctx *ctx, int64_t max_t_nnz);
/* The sparse triple product on a given pattern: rows [row_begin,row_end) of S = H * Q * H^T at the positions of the
 * mask L (n x n, canonical: rows strictly ascending, else SMM_ERR_INVALID -- see smm_csr_is_canonical) with k >= i.
 * L's values are ignored; a position with no structural contribution holds +0.0.  Values as smm_triple_product_sparse
 * (SMM_EXACT: bit-identical to smm_triple_product at (i,k)).  SMM_FULL_MATRIX (whole range only) mirrors the upper part;
 * L's entries below the diagonal are ignored.  Stage 1 (T_b = H[b] * Q) and the row-block budget are those of
 * smm_triple_product_sparse; the stage-2 pattern is L's rows, so H^T is neither built nor used. */
int  smm_triple_product_sparse_masked(smm_ctx *ctx, smm_csr *h, smm_csr *q, smm_csr *mask, int flags, int64_t row_begin,
                                      int64_t row_end, smm_result **out);

/* ------------------------------------------------------------------ masked SpGEMM (A * B on a given pattern)
 * Writes nnz(mask) values, in the mask's order, of C = A * B at the positions of mask (A.rows x B.cols, canonical, else
 * SMM_ERR_INVALID; its values are ignored, explicitly stored zeros are positions) into caller-owned device memory.
 * A position that no product A[i,k] * B[k,j] reaches holds +0.0.  A pair (k,j) that row i of A does not store is never
 * multiplied (an inf in B cannot reach C through a missing A[i,k]).
 *   SMM_EXACT (the only flag accepted): at every position that smm_spgemm_* stores, bit-identical to its SMM_EXACT value
 *   (the reference's order), for any legal A and B.  Without it: within 1e-10 relative to (|A| |B|)[i,j].
 * Two evaluation paths, chosen per row (smm_ctx_tune_masked): the dot path sums row j of B^T against a table of A_i
 * (cost nnz(A_i) + sum over the mask row of nnz(B^T_j); canonical A only) and the row path walks A_i * B filtered by a
 * table of the mask row (cost: the row's products).  B^T with values is built on the device and cached on B's handle;
 * smm_csr_update_values[_device] on B drops it. */
int  smm_spgemm_masked(smm_ctx *ctx, smm_csr *a, smm_csr *b, smm_csr *mask, int flags, double *d_c_data);
int  smm_spgemm_masked_host(smm_ctx *ctx, smm_csr *a, smm_csr *b, smm_csr *mask, int flags, double *c_data);
/* Path of the masked SpGEMM: 0 = per-row cost model (default), 1 = dot path, 2 = row path.  A that is not canonical
 * always takes the row path.  Results do not depend on it (bit for bit under SMM_EXACT). */
int  smm_ctx_tune_masked(smm_ctx *ctx, int mode);

/* ------------------------------------------------------------------ sparse x dense: Y = op(A) * X
 * op(A) (m x K) is A, or A^T with SMM_TRANSPOSE (the transpose is built on the device on first use and cached on A's
 * handle; smm_csr_update_values[_device] drops it).  X: K x k, Y: m x k, both row-major float64
 * with leading dimensions ldx, ldy >= k; every element of Y's k columns is written, its padding columns are not.
 * 64-bit offsets: rows * ld may exceed 2^31.  k = 0 is valid and does nothing.
 *   SMM_EXACT: Y[i,j] starts at +0.0 and adds A[i,p] * X[col_p, j] for p in row i's stored order, one product at a time
 *   (scipy's csr_matvec / csr_matvecs loop; for A^T the rows of scipy's A.tocsc()): bit-identical to scipy's A @ X and
 *   A.T @ X for any legal CSR.  Without it: fused multiply-adds and long rows split across waves, within 1e-10 of
 *   (|A| |X|)[i,j] of the exact value.  No float atomics: results are bitwise reproducible in both modes.
 *   A pair that row i does not store is never multiplied (an inf in X[c,:] reaches Y[i,:] only through A[i,c]).
 * Accepted flags: SMM_EXACT | SMM_TRANSPOSE; anything else, ldx < k, ldy < k, NULL buffers that should hold data and
 * overlapping device ranges of X and Y are SMM_ERR_INVALID. */
int  smm_spmm(smm_ctx *ctx, smm_csr *a, int flags, int64_t k, const double *d_x, int64_t ldx, double *d_y, int64_t ldy);
/* Same with host X and Y (uploaded / downloaded through pool temporaries). */
int  smm_spmm_host(smm_ctx *ctx, smm_csr *a, int flags, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy);
/* Y = H * (Q * (H^T * X)) = S X with S = H Q H^T never formed: three sparse x dense products with device intermediates
 * (H: n x K, Q: K x K, need not be symmetric; X, Y: n x k).  H^T comes from H's cached transpose.  X is taken in column
 * blocks whose two K x block intermediates fit the context's apply budget (smm_ctx_tune_spmm).  SMM_EXACT (the only flag):
 * bit-identical to scipy's H @ (Q @ (H.T @ X)). */
int  smm_triple_apply(smm_ctx *ctx, smm_csr *h, smm_csr *q, int flags, int64_t k, const double *d_x, int64_t ldx,
                      double *d_y, int64_t ldy);
int  smm_triple_apply_host(smm_ctx *ctx, smm_csr *h, smm_csr *q, int flags, int64_t k, const double *x, int64_t ldx,
                           double *y, int64_t ldy);
/* Kernel classes of the sparse x dense product: mode 0 = rows binned by length (default), 1 / 2 / 3 = every row in the
 * tiny / group / long class (tests).  apply_budget_bytes: bytes of smm_triple_apply's two intermediates per column block,
 * 0 = the default, 1 GiB.  The result's shape and values never depend on either (bit for bit under SMM_EXACT). */
int  smm_ctx_tune_spmm(smm_ctx *ctx, int mode, int64_t apply_budget_bytes);

/* ------------------------------------------------------------------ sampled dense product: (X Y^T) on a pattern
 * Writes nnz(mask) values, in the mask's stored order, of C[p] = X[i,:] . Y[j,:] for every stored entry p = (i, j) of mask
 * (m x n) into caller-owned memory -- SDDMM with dense operands, the dense counterpart of smm_spgemm_masked.  mask may be
 * any legal CSR: rows may be unsorted and may repeat columns (a repeated position yields a repeated value); its values
 * are read only with SMM_SCALE_BY_MASK.  X: m x k, Y: n x k, both row-major float64 with leading dimensions ldx, ldy >= k
 * (one row = one state variable's ensemble members); 64-bit offsets.  d_y == d_x with ldy == ldx is the covariance case
 * X X^T.  The call allocates no pattern, runs no symbolic phase and builds no transpose.
 *   SMM_EXACT: s = +0.0; s = s + X[i,e] * Y[j,e] for e = 0 .. k-1, every product rounded before its add: bit-identical to
 *   that loop for any legal mask, any k, any ld, aligned or unaligned bases.
 *   Without it, with NP = 2 G and G = ceil(k / 2) rounded up to a power of two in [4, 64] (so NP depends on k alone):
 *   partial q of NP starts at +0.0 and takes s[q] = fma(X[i,e], Y[j,e], s[q]) for e = q, q + NP, q + 2 NP, ... in ascending
 *   e; then s[q] = s[q] + s[q + h] for every q that is a multiple of 2 h, for h = 1, 2, 4, ..., NP / 2; the result is s[0].
 *   The order does not depend on the mask, on a row's length, on the entry's place in its row, on the alignment of the
 *   operands or on smm_ctx_tune_sddmm: two runs agree bit for bit, and so does one (i, j) in two different masks.
 *   Within 1e-10 (|X| |Y|^T)[i,j] (times |w| when scaled) of the exact value.  No float atomics.
 *   SMM_SCALE_BY_MASK: C[p] = mask.data[p] * s, the multiply always carried out (0 * inf = NaN); without it C[p] = s.
 *   k = 0 writes +0.0 (w * +0.0 when scaled).
 * X[i,:] and Y[j,:] are read only for the entries that name them: an inf or NaN in row j of Y reaches exactly the entries
 * of column j, and rows that no entry names are never loaded.
 * Flags other than SMM_EXACT | SMM_SCALE_BY_MASK, k < 0, ldx < k, ldy < k, NULL buffers that should hold data and an
 * output range that overlaps X or Y are SMM_ERR_INVALID, before any launch. */
int  smm_sddmm(smm_ctx *ctx, smm_csr *mask, int flags, int64_t k, const double *d_x, int64_t ldx, const double *d_y, int64_t ldy,
               double *d_c_data);
/* Same with host X, Y and c_data (uploaded / downloaded through pool temporaries). */
int  smm_sddmm_host(smm_ctx *ctx, smm_csr *mask, int flags, int64_t k, const double *x, int64_t ldx, const double *y, int64_t ldy,
                    double *c_data);
/* Kernel classes of the sampled dense product: mode 0 = chosen from nnz(mask) (default), 1 = neighbouring lane groups take
 * neighbouring entries, 2 = every lane group walks a run of consecutive entries and keeps X[i,:] in registers (tests).
 * Results never depend on it, bit for bit, in either mode. */
int  smm_ctx_tune_sddmm(smm_ctx *ctx, int mode);

/* ------------------------------------------------------------------ localisation taper from point coordinates
 * L[i,j] = w(|a_i - b_j|) for every pair of points closer than `cutoff`, as a new operand (na x nb) owned by the caller
 * (smm_csr_destroy), as smm_csr_transpose returns one -- the mask / weight matrix L of smm_triple_product_sparse_masked,
 * smm_spgemm_masked and smm_sddmm, built where it is used instead of on the host.  a: na x dim, b: nb x dim, both
 * row-major float64 with leading dimensions lda, ldb >= dim; dim is 1, 2 or 3; 64-bit offsets.  d_b may be d_a's own
 * buffer: the square, symmetric case.  Distances are Euclidean: for points on a sphere pass unit-sphere xyz and a chord
 * cutoff.  No periodic domains.
 *   Distance    d2 = +0.0; for t = 0 .. dim-1: df = a[i,t] - b[j,t]; d2 = d2 + df * df, every product rounded before its
 *               add.  The sign of df cannot matter, so the square case is symmetric bit for bit.
 *   Membership  (i, j) is stored iff d2 < cutoff * cutoff: a strict comparison against a right-hand side rounded once.
 *               Nothing else decides the pattern; the cell search that finds the candidates never loses a pair that
 *               passes this test (csrc/smm_taper.hpp has the argument).  Columns are strictly ascending in every row, so
 *               smm_csr_is_canonical holds; pairs at distance 0 (and i == j of the square case) are stored.
 *   Value       SMM_TAPER_BOXCAR: 1.0.
 *               SMM_TAPER_GASPARI_COHN: Gaspari & Cohn (1999), eq. 4.10, with half-width c = 0.5 * cutoff and
 *               z = sqrt(d2) / c (IEEE square root and division), every multiply rounded before its add:
 *                 z <= 1:    p = -0.25 * z + 0.5;  p = p * z + 0.625;  p = p * z - (5.0 / 3.0);  p = p * z;  p = p * z + 1.0
 *                 otherwise: p = (1.0 / 12.0) * z - 0.5;  p = p * z + 0.625;  p = p * z + (5.0 / 3.0);  p = p * z - 5.0;
 *                            p = p * z + 4.0;  p = p - 2.0 / (3.0 * z)
 *                 w = p < 0.0 ? +0.0 : p          (this order gives down to -1.6e-15 just inside z = 2; exactly 1.0 at z = 0)
 *   One mode: there is no SMM_EXACT flag and no other order -- a dozen flops per 12-byte entry.  Pattern and values are
 *   bit-identical to that recipe carried out in IEEE double, and two calls give the same bits.  No float atomics.
 * The candidates come from a uniform grid over b's bounding box with cell edge cutoff * (1 + 2^-20), grown by factors of
 * 1.25 while the box would hold more than max(4096, 2 nb) cells (at most 2^30); a point x has cell coordinate
 * trunc((x - lo) * (1 / edge)), clamped to the grid, in every dimension.
 * SMM_ERR_INVALID, before any launch that depends on the value: dim outside 1..3, unknown kind, cutoff not finite or
 * <= 0, lda or ldb < dim, a NULL buffer with rows > 0, na or nb < 0 or >= 2^31 - 1 (an operand's dimension); also a
 * coordinate that is NaN or +-inf (counted in the pass that takes the bounding box).  More than 2^31 - 2 entries:
 * SMM_ERR_OVERFLOW (operand row pointers are int32).  na == 0 or nb == 0: an operand without entries, no launch. */
enum smm_taper_kind { SMM_TAPER_BOXCAR = 0, SMM_TAPER_GASPARI_COHN = 1 };
int  smm_taper_build(smm_ctx *ctx, int dim, int kind, double cutoff, int64_t na, const double *d_a, int64_t lda,
                     int64_t nb, const double *d_b, int64_t ldb, smm_csr **out);
/* Same with a and b in host memory (uploaded through pool temporaries; b == a with ldb == lda and nb == na once). */
int  smm_taper_build_host(smm_ctx *ctx, int dim, int kind, double cutoff, int64_t na, const double *a, int64_t lda,
                          int64_t nb, const double *b, int64_t ldb, smm_csr **out);

/* ------------------------------------------------------------------ parametric covariance on a given pattern
 * For every stored entry p = (i, j) of `pattern` (na x nb; any legal CSR of this context: rows may be unsorted, repeat
 * columns, be empty) a covariance value variance * c(h) and / or its derivative with respect to a correlation length,
 * from the coordinates a_i and b_j, written at position p of the caller-owned arrays d_val / d_dval (nnz(pattern) float64
 * each, in the pattern's stored order; either may be NULL, not both).  The pattern comes from an operand the library can
 * already build -- a taper (smm_taper_build), Q's pattern, or H's for cross-covariances; this call searches nothing and
 * writes neither the pattern operand nor anything cached for it.  a: na x dim, b: nb x dim, row-major float64 with leading
 * dimensions lda, ldb >= dim; dim is 1, 2 or 3; 64-bit offsets; d_b may be d_a's own buffer.  length: dim doubles in HOST
 * memory, the correlation length of every coordinate.  Distances are Euclidean in the scaled coordinates.
 * Every product is rounded before its add; there is one mode, no SMM_EXACT flag and no other order.
 *   Distance    u_t = (a[i,t] - b[j,t]) / length[t] (IEEE division); h2 = +0.0; h2 = h2 + u_t * u_t for t = 0 .. dim-1;
 *               h = sqrt(h2) (IEEE square root).  The sign of u_t cannot matter: the square case on a symmetric pattern
 *               is symmetric bit for bit.
 *   Models      c = the correlation, g = -dc/dh; e = exp(x) is the device library's double exp.
 *               SMM_COV_SPHERICAL    h < 1: c = ((0.5 * h) * h - 1.5) * h + 1.0, g = 1.5 - 1.5 * (h * h); h >= 1: both +0.0
 *               SMM_COV_EXPONENTIAL  e = exp(-h);  c = e;  g = e
 *               SMM_COV_GAUSSIAN     e = exp(-h2); c = e;  g = (2.0 * h) * e
 *               SMM_COV_MATERN32     s = sqrt3 * h (sqrt3 = 1.7320508075688772, the nearest double); e = exp(-s);
 *                                    c = (1.0 + s) * e;  g = (3.0 * h) * e
 *               SMM_COV_MATERN52     s = sqrt5 * h (sqrt5 = 2.23606797749979); e = exp(-s);
 *                                    c = ((1.0 + s) + (5.0 / 3.0) * h2) * e;  g = (((5.0 / 3.0) * h) * (1.0 + s)) * e
 *   Value       val[p] = variance * c: exactly variance at h = 0 in every model.
 *   Derivative  wrt = t in 0 .. dim-1, d/d length[t]: +0.0 when h == 0, else ((variance * g) * (u_t * u_t)) / (h * length[t]).
 *               wrt = SMM_COV_WRT_ALL, d/d of one common length: +0.0 when h == 0, else ((variance * g) * h) / length[0];
 *               accepted only when all dim lengths are the same double.  wrt = SMM_COV_WRT_NONE: no derivative.
 *   SMM_COV_SCALE_BY_PATTERN (the only flag): each output is multiplied last by the pattern's stored value w[p], the
 *               multiply always carried out (0 * inf = NaN).  With w a Gaspari-Cohn taper this is Q = L o C, compactly
 *               supported and still positive semidefinite; the taper does not depend on the length, so dQ takes the same factor.
 *   The spherical model is bit-identical to that recipe in IEEE double; the others are within the device exp's error (a
 *   few ulp) of it; two calls give the same bits.  No float atomics.
 * Coordinates are not screened: an infinite one gives what the recipe gives (inf - inf = NaN), a NaN gives NaN at its
 * entries in every model (the spherical one included: neither h < 1 nor h >= 1 holds).
 * SMM_ERR_INVALID, before any launch: an unknown flag or model, dim outside 1..3, a length that is not finite or <= 0, a
 * variance that is not finite (0 is allowed), wrt outside {SMM_COV_WRT_NONE, 0 .. dim-1, SMM_COV_WRT_ALL}, SMM_COV_WRT_ALL
 * with unequal lengths, d_dval without wrt or wrt without d_dval, both outputs NULL, lda or ldb < dim, a NULL coordinate
 * buffer with rows > 0, na or nb other than the pattern's rows and columns, SMM_COV_SCALE_BY_PATTERN on a pattern without
 * values, an output that overlaps the other output or the coordinates.  nnz(pattern) == 0: no launch, SMM_OK.  A column
 * outside [0, nb) (reachable only through smm_csr_from_device) is skipped and reported as SMM_ERR_INTERNAL. */
enum smm_cov_model { SMM_COV_SPHERICAL = 0, SMM_COV_EXPONENTIAL = 1, SMM_COV_GAUSSIAN = 2, SMM_COV_MATERN32 = 3, SMM_COV_MATERN52 = 4 };
enum smm_cov_wrt { SMM_COV_WRT_NONE = -1, SMM_COV_WRT_ALL = 3 };
enum smm_cov_flags { SMM_COV_SCALE_BY_PATTERN = 32 };
int  smm_cov_eval(smm_ctx *ctx, smm_csr *pattern, int flags, int model, int dim, const double *length, double variance, int wrt,
                  int64_t na, const double *d_a, int64_t lda, int64_t nb, const double *d_b, int64_t ldb, double *d_val, double *d_dval);
/* Same with a, b, val and dval in host memory (through pool temporaries; b == a with ldb == lda is uploaded once). */
int  smm_cov_eval_host(smm_ctx *ctx, smm_csr *pattern, int flags, int model, int dim, const double *length, double variance, int wrt,
                       int64_t na, const double *a, int64_t lda, int64_t nb, const double *b, int64_t ldb, double *val, double *dval);

/* ------------------------------------------------------------------ empirical variogram on a given pattern
 * The look at the data that comes before a model and a first length are chosen: over the stored entries e = (i, j) of
 * `pattern` (n x n; any legal CSR of this context: rows may be unsorted, repeat columns, be empty -- a taper from
 * smm_taper_build is the usual one; this call searches nothing), binned by the distance of the points a_i and a_j, per bin
 * the number of pairs, the sum of their distances and the sum of their squared increments of the values y.  a: n x dim,
 * row-major float64, leading dimension lda >= dim, dim 1, 2 or 3; y: n x k, row-major float64, ldy >= k (k variables, or k
 * realisations of one); 64-bit offsets.  edges: nb + 1 doubles in HOST memory, the bins [edges[b], edges[b+1]).  The three
 * outputs are in HOST memory for both entries -- count: nb x int64, sum_h and sum_sq: nb doubles each -- and the call
 * returns synchronised.  lag[b] = sum_h[b] / count[b] and gamma[b] = sum_sq[b] / (2 k count[b]) are the caller's divisions.
 * The call writes neither the pattern operand nor anything cached for it.  Every product is rounded before its add; there
 * is one mode, no SMM_EXACT flag, no other order and no float atomics.  For each stored entry e = (i, j), e its position in
 * the pattern's stored order:
 *   Distance    d2 = +0.0; for t = 0 .. dim-1: df = a[i,t] - a[j,t]; d2 = d2 + df * df; h = sqrt(d2) (IEEE square root): the
 *               recipe of smm_taper_build, so an entry of a taper has h < cutoff exactly as the taper decided it.
 *   Increment   s = +0.0; for c = 0 .. k-1: dv = y[i,c] - y[j,c]; s = s + dv * dv.  k = 0 gives +0.0.
 *   Bin         the entry takes part iff edges[0] <= h < edges[nb] and, by default, j > i -- so each pair of a symmetric
 *               pattern counts once and the diagonal never.  SMM_VG_ALL_ENTRIES (the only flag) drops the condition on j:
 *               every stored entry takes part, the diagonal included.  Its bin is b = the number of q in 1 .. nb with
 *               edges[q] <= h: comparisons only, so h == edges[b] lies in bin b and a NaN distance in no bin.  Values are
 *               not screened: a NaN or an infinity in y reaches exactly sum_sq of the bins its pairs fall in, never count
 *               or sum_h.
 *   Slot        with T = SMM_VG_SLOTS and W = T / 64: run = e / SMM_VG_RUN, slot t = (run mod W) * 64 + (e mod 64) -- the
 *               lane map of smm_cov_eval on a grid of exactly T lanes: waves take runs of SMM_VG_RUN consecutive entries
 *               round robin.  For every bin b, slot (t, b) starts at +0.0 and adds h (for sum_h) and s (for sum_sq) of
 *               its entries in ascending e.
 *   Tree        for every bin: p[t] = p[t] + p[t + g] for every t that is a multiple of 2 g, for g = 1, 2, 4, ..., T / 2;
 *               the result is p[0].  Adjacent pairs, as in smm_sddmm's default order (not the halving tree of the CG's
 *               dot products): the steps inside a wave come first, and the result does not depend on the workgroup size.
 *   count       exact integer counting.
 * sum_h, sum_sq and count are bit-identical to that recipe carried out in IEEE double whatever the pattern's row
 * structure, and two calls give the same bits.  Every term is >= 0, so each sum is within (ceil(nnz / T) + 17) * 2^-53
 * relative of the exact sum of its rounded terms.  SMM_VG_SLOTS and SMM_VG_RUN are part of the contract.
 * SMM_ERR_INVALID, before any launch or allocation: an unknown flag, dim outside 1..3, nb outside 1..SMM_VG_MAX_BINS, an edge
 * that is not finite, edges[0] < 0, edges not strictly ascending, a pattern that is not square, k < 0, lda < dim, ldy < k,
 * a NULL buffer that should hold data (edges, the three outputs; a with n > 0; y with n > 0 and k > 0).  nnz(pattern) == 0:
 * no launch, counts 0 and sums +0.0.  An entry that its row's range does not contain, or a column outside [0, n)
 * (reachable only through smm_csr_from_device), is skipped and reported as SMM_ERR_INTERNAL. */
enum smm_vg_constants { SMM_VG_RUN = 256, SMM_VG_SLOTS = 65536, SMM_VG_MAX_BINS = 32 };
enum smm_vg_flags { SMM_VG_ALL_ENTRIES = 64 };
int  smm_variogram(smm_ctx *ctx, smm_csr *pattern, int flags, int dim, const double *d_a, int64_t lda, int64_t k, const double *d_y,
                   int64_t ldy, int nb, const double *edges, int64_t *count, double *sum_h, double *sum_sq);
/* Same with a and y in host memory (uploaded through pool temporaries). */
int  smm_variogram_host(smm_ctx *ctx, smm_csr *pattern, int flags, int dim, const double *a, int64_t lda, int64_t k, const double *y,
                        int64_t ldy, int nb, const double *edges, int64_t *count, double *sum_h, double *sum_sq);

/* ------------------------------------------------------------------ observation operator from point coordinates
 * H (n x K): the matrix that interpolates a field on a rectilinear grid to n points, as a new operand owned by the caller
 * (smm_csr_destroy), as smm_taper_build returns one -- the H of smm_triple_apply, smm_innovation_solve and their _kron forms,
 * built where it is used instead of on the host.
 *   Grid        dim is 1 to 4.  Axis t has m_t >= 2 nodes x_t[0] < x_t[1] < ... (finite, strictly ascending, float64; the
 *               spacing may vary).  K = prod m_t < 2^31 - 1.  Node (j_0, ..., j_{dim-1}) is column (j_0 m_1 + j_1) m_2 + ...:
 *               row-major, axis 0 slowest, stride_t = prod of m_u over u > t.  With time as axis 0 the columns are those of
 *               the Kronecker operand below (t r + j).
 *   Cell        for point i and axis t with coordinate x: c = (number of nodes <= x) - 1, clamped to [0, m_t - 2] (only
 *               comparisons: any search gives the same c), and f = (x - x_t[c]) / (x_t[c+1] - x_t[c]), one IEEE
 *               subtraction each and one IEEE division.  For x inside [x_t[0], x_t[m_t-1]] this gives 0 <= f <= 1, and
 *               f = 1.0 exactly on the last node.
 *   SMM_INTERP_LINEAR   row i holds 2^dim entries; entry e (bit b_t of e, axis 0 the most significant bit) is at column
 *               sum (c_t + b_t) stride_t with value ((w_0 * w_1) * w_2) * w_3, taken left to right, every product rounded,
 *               w_t = f_t if b_t is set and 1.0 - f_t otherwise.  Columns ascend strictly with e (stride_t >= 2 stride_{t+1}),
 *               so smm_csr_is_canonical holds; explicit zeros stay entries, as in smm_kron_build.  The row pointer is the
 *               closed form ptr[i] = i 2^dim: no count pass, no scan.
 *   SMM_INTERP_NEAREST  one entry per row, at node c_t + (f_t > 0.5 ? 1 : 0) in every axis (a tie goes to the lower node),
 *               with value 1.0; ptr[i] = i.
 *   Outside     a point is outside if x < x_t[0] or x > x_t[m_t-1] in any axis.
 *               SMM_INTERP_REJECT: the call returns SMM_ERR_INVALID with the number of outside points in the message; no
 *               operand is returned and no pool block stays handed out (an integer count, taken before the operand is
 *               allocated).  SMM_INTERP_CLAMP: f_t is replaced by 0.0 below the first node and 1.0 above the last --
 *               constant extrapolation.  SMM_INTERP_ZERO: the columns of CLAMP, and every value of the row is +0.0: the
 *               observation sees nothing and the closed-form row pointer survives.
 *               A coordinate that is NaN or +-inf is SMM_ERR_INVALID under every policy, with the count in the message.
 *   One mode: there is no SMM_EXACT flag and no other order.  Pattern and values are bit-identical to that recipe carried
 *   out in IEEE double.  No float atomics: two calls give the same bits.
 * axis_len (dim entries) and axes (the nodes of axis 0, 1, ... one after the other: sum m_t doubles) are HOST arrays in both
 * forms and go up through a pool temporary.  The points are n x dim row-major float64 with leading dimension ldp >= dim,
 * 64-bit offsets, used where they are.
 * SMM_ERR_INVALID before any launch: dim outside 1..4, unknown method or policy, an axis shorter than 2, not strictly
 * ascending or not finite, K >= 2^31 - 1, n < 0 or n >= 2^31 - 1, ldp < dim, a NULL buffer with n > 0.  More than 2^31 - 2
 * entries (n 2^dim, or n): SMM_ERR_OVERFLOW.  n == 0: an operand without entries, no launch. */
enum smm_interp_method { SMM_INTERP_LINEAR = 0, SMM_INTERP_NEAREST = 1 };
enum smm_interp_outside { SMM_INTERP_REJECT = 0, SMM_INTERP_CLAMP = 1, SMM_INTERP_ZERO = 2 };
int  smm_interp_build(smm_ctx *ctx, int dim, const int64_t *axis_len, const double *axes, int method, int outside,
                      int64_t n, const double *d_pts, int64_t ldp, smm_csr **out);
/* Same with the points in host memory (uploaded through a pool temporary). */
int  smm_interp_build_host(smm_ctx *ctx, int dim, const int64_t *axis_len, const double *axes, int method, int outside,
                           int64_t n, const double *pts, int64_t ldp, smm_csr **out);

/* ------------------------------------------------------------------ conjugate gradients on (H Q H^T + R) Z = D
 * S = H Q H^T is never formed (H: n x K, Q: K x K, R: n x n sparse or NULL for S alone; the system is expected to be
 * symmetric positive definite).  B (the right-hand sides D) and X (the solution Z) are n x k row-major float64 with
 * leading dimensions ldb, ldx >= k.  Every column is its own CG with x0 = 0; the columns share each sparse x dense
 * product.  Nothing but one count of live columns per iteration comes to the host between B and X.  Per column:
 *     r = d;  p = r;  rho = dot(r, r);  rhs_sq = rho;  thr = (tol * tol) * rhs_sq
 *     rho <= thr: converged, 0 iterations (a zero column gives x = 0)
 *     for it = 1 .. maxiter:
 *         w = H (Q (H^T p)) + R p              one add per element; without R, w = S p
 *         pw = dot(p, w);  not (pw > 0): status 2, iterations = it - 1, frozen   (pw <= 0 and NaN)
 *         alpha = rho / pw;  x = x + alpha p;  r = r - alpha w;  rho_new = dot(r, r)
 *         rho_new <= thr: status 0, iterations = it, frozen
 *         beta = rho_new / rho;  p = r + beta p;  rho = rho_new
 *     still live after maxiter: status 1, iterations = maxiter
 * A frozen column's x, residual_sq and iterations never change again; columns cannot influence each other.  The test is
 * on squared norms of the recurrence's residual (no square root); alpha and beta are IEEE divisions done on the device.
 * dot(u, v), for T = SMM_CG_LANES: partial t starts at +0.0 and adds u[i] v[i] for i = t, t + T, t + 2T, ... in
 * ascending i; then s[t] = s[t] + s[t + h] for h = T/2, T/4, ..., 1; the result is s[0].
 *   SMM_EXACT (the only flag): the three products are the exact sparse x dense product above, every multiply in a dot
 *   or a vector update is rounded before its add, and X and the four outputs are bit-identical to that recipe carried
 *   out in IEEE double, for any legal CSR operands.  Without it: fused multiply-adds and the default sparse x dense
 *   kernels; no float atomics, so two runs give the same bits.
 * The right-hand sides are solved in column blocks when five n x block vectors and two K x block intermediates exceed the
 * apply budget (smm_ctx_tune_spmm); blocking changes no bit under SMM_EXACT (default mode: as long as no block is a single
 * column).  The rows of H^T, Q, H and R are binned once per column block, not per iteration.
 * Outputs, host arrays of k entries each: iterations, status (0 converged, 1 iteration limit, 2 breakdown),
 * residual_sq (the recurrence's dot(r, r) when the column froze or the solve ended) and rhs_sq (dot(d, d)).
 * Non-convergence is reported there, not as an error.  k < 0, ldb < k, ldx < k, tol not finite and positive, maxiter < 0,
 * NULL buffers that should hold data, overlapping ranges of B and X and shapes that do not fit are SMM_ERR_INVALID. */
#define SMM_CG_LANES 2048
int  smm_innovation_solve(smm_ctx *ctx, smm_csr *h, smm_csr *q, smm_csr *r, int flags, int64_t k, const double *d_b,
                          int64_t ldb, double *d_x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                          double *residual_sq, double *rhs_sq);
/* Same with host B and X (uploaded / downloaded through pool temporaries). */
int  smm_innovation_solve_host(smm_ctx *ctx, smm_csr *h, smm_csr *q, smm_csr *r, int flags, int64_t k, const double *b,
                               int64_t ldb, double *x, int64_t ldx, double tol, int64_t maxiter, int *iterations,
                               int *status, double *residual_sq, double *rhs_sq);

/* ------------------------------------------------------------------ Kronecker operand Q = D (x) E
 * The prior covariance of a space-time inverse problem: a temporal factor D (p x p') times a spatial factor E (r x r').
 * D (x) E is (p r) x (p' r'); row t r + j is the pair (t, j), column t' r' + j' the pair (t', j').  Both factors may be any
 * legal CSR (unsorted rows, repeated columns, empty rows).  p r and p' r' must be < 2^31 - 1 (SMM_ERR_INVALID) in every call
 * of this section.
 *
 * smm_kron_build: the explicit matrix as a new operand owned by the caller (smm_csr_destroy), as smm_taper_build returns one.
 *   Row (t, j) holds, for a over row t of D in stored order and b over row j of E in stored order, column
 *   D.idx[a] r' + E.idx[b] with value D.val[a] * E.val[b]: one rounded multiply (inf * 0 is stored as NaN; explicit zeros
 *   stay entries).  One mode: there is no SMM_EXACT flag and no other order.  The row pointer is the closed form
 *   ptr[t r + j] = D.ptr[t] nnz(E) + len_D(t) E.ptr[j]: no count pass, no scan, no atomics.  For canonical D and E the result
 *   is canonical (smm_csr_is_canonical) and its three arrays are those of scipy.sparse.kron(D, E, format="csr"), bit for bit.
 *   Refused before any allocation or launch: a dimension as above (SMM_ERR_INVALID); nnz(D) nnz(E) > 2^31 - 2
 *   (SMM_ERR_OVERFLOW: operand row pointers are int32 -- such a Q is used through its factors, below).  A factor without
 *   entries gives an operand without entries and no launch.
 *
 * smm_kron_apply: Y = (D (x) E) X without forming it.  X: (p' r') x k, Y: (p r) x k, row-major float64 with leading
 *   dimensions ldx, ldy >= k, 64-bit offsets, no overlap of X and Y, every element of Y's k columns written and its padding
 *   not, k = 0 valid -- all as smm_spmm.  The order is part of the contract, E first:
 *       U[(t', j), :] = sum over row j of E, in stored order b, of E.val[b] * X[(t', E.idx[b]), :]      for every t' < p'
 *       Y[(t, j), :]  = sum over row t of D, in stored order a, of D.val[a] * U[(D.idx[a], j), :]
 *   SMM_EXACT (the only flag): every element starts at +0.0 and adds one rounded product at a time -- scipy's
 *   U[t'] = E @ X[t'] followed by D @ U.reshape(p', r k), bit for bit, for any legal CSR factors and any row length.  This
 *   is deliberately NOT the bits of scipy.sparse.kron(D, E) @ X, whose association differs (the two differ in the last bit).
 *   Without it: the same order with fused multiply-adds, within 1e-10 ((|D| (x) |E|) |X|)[i, c] of the exact value.  No float
 *   atomics, and in both kernels a lane owns its elements of U and Y for every k, k = 1 included: two runs give the same
 *   bits, and neither the column blocking below nor k can change a bit, in either mode.
 *   A pair that a factor does not store is never multiplied (an inf in X[(t', j'), :] reaches Y[(t, j), :] only through a
 *   stored D[t, t'] and a stored E[j, j']).
 *   U is a pool temporary of (p' r) x kb: X is taken in blocks of kb columns when U exceeds the apply budget
 *   (smm_ctx_tune_spmm).  There is no transpose flag: (D (x) E)^T = D^T (x) E^T, so callers pass transposed factors.
 *
 * smm_triple_apply_kron / smm_innovation_solve_kron: smm_triple_apply / smm_innovation_solve with Q = D (x) E (D and E square,
 *   p r == H.cols, else SMM_ERR_INVALID) and "Q Z1" replaced by the apply above; everything else -- flags, buffers, the CG
 *   recipe, the outputs -- is that call's contract.  The column block counts three K x kb intermediates (H^T P, U, Q H^T P)
 *   where the CSR form counts two.  The factors' kernels bin no rows and nothing new synchronises with the host inside a CG
 *   iteration.  Under SMM_EXACT blocking changes no bit; in default mode the k = 1 caveat of smm_innovation_solve remains,
 *   through H, H^T and R only. */
int  smm_kron_build(smm_ctx *ctx, smm_csr *d, smm_csr *e, smm_csr **out);
int  smm_kron_apply(smm_ctx *ctx, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *d_x, int64_t ldx, double *d_y, int64_t ldy);
/* Same with host X and Y (uploaded / downloaded through pool temporaries). */
int  smm_kron_apply_host(smm_ctx *ctx, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy);
int  smm_triple_apply_kron(smm_ctx *ctx, smm_csr *h, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *d_x, int64_t ldx,
                           double *d_y, int64_t ldy);
int  smm_triple_apply_kron_host(smm_ctx *ctx, smm_csr *h, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *x, int64_t ldx,
                                double *y, int64_t ldy);
int  smm_innovation_solve_kron(smm_ctx *ctx, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *r, int flags, int64_t k, const double *d_b,
                               int64_t ldb, double *d_x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                               double *residual_sq, double *rhs_sq);
int  smm_innovation_solve_kron_host(smm_ctx *ctx, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *r, int flags, int64_t k, const double *b,
                                    int64_t ldb, double *x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                                    double *residual_sq, double *rhs_sq);

/* ------------------------------------------------------------------ masked products with Q = D (x) E, Q never formed
 * Entries of H (D (x) E) H^T and of A (D (x) E) at the positions of a mask, for a Q that cannot be held (a dense D of 40
 * periods over 25 000 grid points is 2.7e9 entries).  Each entry is its CSR counterpart -- smm_triple_product_sparse_masked,
 * smm_spgemm_masked[_host] -- called with Q = smm_kron_build(d, e): same arguments, flags, result object (smm_result, columns
 * k >= i, SMM_FULL_MATRIX mirrors the upper part, row ranges), +0.0 where nothing reaches, never a product of a pair the
 * operands do not store, within 1e-10 of (|H| |Q| |H|^T)[i,k] resp. (|A| |Q|)[i,c] in default mode.  No Q, no T = H Q and no
 * transpose is allocated: the temporaries are 24 bytes per stored entry of H (A) and the row lists.
 *   Factors: canonical (rows strictly ascending -- their entries are found by bisection; smm_csr_is_canonical), square for the
 *   triple product, p r == H.cols (A.cols), p r and p' r' < 2^31 - 1; else SMM_ERR_INVALID before anything is allocated.  The
 *   mask is canonical, n x n resp. A.rows x p' r'.  H and A may be any legal CSR (unsorted rows, repeated columns).  H, A or a
 *   factor without entries: the pattern filled with +0.0, no value kernel.
 *   SMM_EXACT: bit-identical to the counterpart on the explicit operand.  Written out:
 *     (A Q)[i, c], c = t' r' + j':  over row i of A in stored order a, with (t, j) = divmod(A.idx[a], r), the term
 *       A.val[a] * q, q = D[t,t'] * E[j,j'] rounded once (the value smm_kron_build stores), taken only when both factors
 *       store their entry; the first term lands unchanged, later ones are added one rounded product at a time.
 *     S[i, k]:  T[i, c] as above with A = H, "stored" iff some a reaches it (even if it cancels); then sum = 0.0;
 *       sum += T[i, H.idx[a2]] * H.val[a2] over row k of H in stored order, an unstored T read as +0.0 and still multiplied.
 *   Without SMM_EXACT: the same association with fused multiply-adds (q still rounded once).  No float atomics in either
 *   mode: two runs agree bit for bit, and the value at a position depends on the two rows of H (the row of A) and the
 *   factors only -- not on the mask, the row range or the launch shape. */
int  smm_triple_product_sparse_masked_kron(smm_ctx *ctx, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *mask, int flags,
                                           int64_t row_begin, int64_t row_end, smm_result **out);
int  smm_spgemm_masked_kron(smm_ctx *ctx, smm_csr *a, smm_csr *d, smm_csr *e, smm_csr *mask, int flags, double *d_c_data);
int  smm_spgemm_masked_kron_host(smm_ctx *ctx, smm_csr *a, smm_csr *d, smm_csr *e, smm_csr *mask, int flags, double *c_data);

/* ------------------------------------------------------------------ log det(H Q H^T + R): probes and recorded CG coefficients
 * Stochastic Lanczos quadrature reads ln det Psi, Psi = H Q H^T + R, off the batched CG above: probes z_c with entries +-1,
 * CG on Psi x = z_c, the CG coefficients turned into the Lanczos tridiagonal T_c (m x m for a column with m iterations),
 *     T[j, j] = 1 / alpha_j + beta_{j-1} / alpha_{j-1}  (second term absent for j = 0),   T[j, j+1] = T[j+1, j] = sqrt(beta_j) / alpha_j,
 * and z_c^T ln(Psi) z_c ~ n e_1^T ln(T_c) e_1; the mean over the probes estimates tr ln Psi = ln det Psi.  The device part is
 * the two calls below; the eigen-decomposition of the small tridiagonals is the caller's (the Python package uses LAPACK).
 *
 * smm_probe_fill: X[i, c] = +1.0 or -1.0 for i < n, c < k, into a row-major float64 block with leading dimension ldx >= k;
 *   padding is not written.  The sign is part of the contract.  With 64-bit wrap-around arithmetic,
 *       z = seed + c * 0xD1B54A32D192ED03 + (i + 1) * 0x9E3779B97F4A7C15
 *       z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9
 *       z ^= z >> 27;  z *= 0x94D049BB133111EB
 *       z ^= z >> 31
 *   and the entry is -1.0 iff bit 63 of z is set.  The value depends on (seed, i, c) only -- not on k, ldx or the launch
 *   geometry: column c of any call with the same seed is the same probe.  k = 0 or n = 0: no launch.  A NULL buffer with data
 *   to write, ldx < k and negative sizes are SMM_ERR_INVALID.  The call returns with the fill queued on the context's stream.
 *
 * smm_innovation_solve_coef / smm_innovation_solve_coef_kron: smm_innovation_solve / smm_innovation_solve_kron on device B and
 *   X -- the same arguments, recipe, outputs and bits -- with the coefficients of every column kept.  alpha and beta are
 *   host arrays of maxiter x k doubles, row it - 1, column j:
 *       alpha[it - 1, j]  the alpha of iteration it of column j, written where the column does not break down in it
 *       beta[it - 1, j]   the beta of iteration it, written where the column does not converge in it
 *   and every other entry is +0.0 (a frozen column is never written again).  So a column with iterations = m has m alphas;
 *   m - 1 betas when its status is 0, m betas when it is 1 or 2.  On the device the histories are two pool temporaries of
 *   maxiter x kb per column block, zeroed per block and downloaded after the block's loop into the caller's columns: nothing
 *   new synchronises inside the iteration, and column blocking puts every column's coefficients in its own place.  Under
 *   SMM_EXACT alpha and beta are bit-identical to the recipe above carried out in IEEE double, for any blocking; in default
 *   mode two runs agree bit for bit.  maxiter sizes the histories: 1 <= maxiter <= 65536, else SMM_ERR_INVALID, as are NULL
 *   alpha or beta (k > 0) and a NULL d_x. */
int  smm_probe_fill(smm_ctx *ctx, int64_t n, int64_t k, uint64_t seed, double *d_x, int64_t ldx);
int  smm_innovation_solve_coef(smm_ctx *ctx, smm_csr *h, smm_csr *q, smm_csr *r, int flags, int64_t k, const double *d_b,
                               int64_t ldb, double *d_x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                               double *residual_sq, double *rhs_sq, double *alpha, double *beta);
int  smm_innovation_solve_coef_kron(smm_ctx *ctx, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *r, int flags, int64_t k,
                                    const double *d_b, int64_t ldb, double *d_x, int64_t ldx, double tol, int64_t maxiter,
                                    int *iterations, int *status, double *residual_sq, double *rhs_sq, double *alpha, double *beta);

/* ------------------------------------------------------------------ device memory helpers
 * (so that hosts without torch can still hold results in HBM) */
int  smm_device_malloc(smm_ctx *ctx, int64_t bytes, void **d_ptr);
int  smm_device_free(smm_ctx *ctx, void *d_ptr);
int  smm_memcpy_d2h(smm_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes);
int  smm_memcpy_h2d(smm_ctx *ctx, void *dst_dev, const void *src_host, int64_t bytes);

/* ================================================================== LEGACY ABI
 * Binary drop-in for the library the reference's unmodified matrix_ops.py loads
 * (lib/libsparse*.so, matrix_ops.py:118-136).  Layouts as that file declares them. */
struct sparsemat {                 /* matrix_ops.py:26-33 */
    int nzmax, rows, cols;
    int *rowPtr;
    int *colInd;
    double *values;
};
struct darray {                    /* matrix_ops.py:44-48 */
    double *array;
    int rows, cols;
};
struct iarray {                    /* include/matrix_def.h:34-38 with int dims */
    int *array;
    int rows, cols;
};

struct sparsemat *create_sparsemat(int rows, int cols, int nzmax);   /* memfunctions.cpp:117-131 */
struct darray    *create_darray(int rows, int cols);                 /* memfunctions.cpp:143-154 */
void destroy_sparsemat(struct sparsemat *m);                         /* memfunctions.cpp:22-33   */
void destroy_darray(struct darray *m);                               /* memfunctions.cpp:51-57   */
void destroy_iarray(struct iarray *m);                               /* memfunctions.cpp:37-43   */
void modifyalloc(struct sparsemat *m, int new_size);                 /* memfunctions.cpp:77-103  */
void limits(int tcov_rows, int numprocs, struct iarray *result);     /* workdivision.cpp:16-89   */
/* imemSize is the reference's CPU scratch hint (sparse_sparse_sparse.cpp:204-217); it has
 * no meaning on the GPU and is accepted and ignored.  On failure the output struct is left
 * with nzmax==0 / NULL arrays and a message goes to stderr, as the reference does. */
void sparse_nosym(const struct sparsemat *a, const struct sparsemat *b, struct sparsemat *c, int imemSize);
void sparse_sym(const struct sparsemat *a, const struct sparsemat *b, struct sparsemat *c, int imemSize);
void sparsework_nosym(const struct sparsemat *a, const struct sparsemat *b, struct sparsemat *c,
                      int startIndex, int endIndex, int memIncrease);   /* sparsework.cpp:12-149  */
void sparsework_sym(const struct sparsemat *a, const struct sparsemat *b, struct sparsemat *c,
                    int startIndex, int endIndex, int memIncrease);     /* sparsework.cpp:156-300 */
void dense_nosym(const struct sparsemat *a, const struct sparsemat *b, struct darray *c);
void dense_sym(const struct sparsemat *a, const struct sparsemat *b, struct darray *c);
void triple_product(struct sparsemat *h, struct sparsemat *q, struct darray *c, int compute_full_matrix);

#ifdef __cplusplus
}
#endif
#endif /* SMM_HIP_H */
