// smm_api.hip -- host side of libsmm_hip.so: the v2 C ABI declared in include/smm_hip.h.
// Owns the device context (stream, pooled workspace, per-kernel timing) and sequences the
// kernels of smm_kernels.hpp.  There is deliberately no CPU compute path in this file: with
// no device every entry point fails with SMM_ERR_NO_DEVICE.
#include "smm_kernels.hpp"
#include "smm_slab.hpp"
#include "smm_ring.hpp"
#include "smm_triple_sparse.hpp"
#include "smm_masked.hpp"
#include "smm_spmm.hpp"
#include "smm_kron.hpp"
#include "smm_kron_masked.hpp"
#include "smm_cg.hpp"
#include "smm_slq.hpp"
#include "smm_sddmm.hpp"
#include "smm_taper.hpp"
#include "smm_interp.hpp"
#include "smm_cov.hpp"
#include "smm_variogram.hpp"
#include "../../include/smm_hip.h"

#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace smm;

// ------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(SMM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                \
    } while (0)
#define CHK(expr)                      \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != SMM_OK) return rc_; \
    } while (0)

extern "C" const char *smm_last_error(void) { return g_err; }

extern "C" int smm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

// ------------------------------------------------------------------------------ context
struct PoolBlock { void *p; size_t bytes; };
struct TimedLaunch { std::string name; hipEvent_t t0, t1; };

struct smm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool timing = false;
    int sym_wide = 1;        // symbolic phase on 16-bit columns: chunks of 128 entries (env SMM_SYM_WIDE=0: 64)
    int sym_ccs = 1;         // symbolic phase over the chunk-padded column stream (smm_symbolic_ccs; env SMM_SYM_CCS=0: smm_symbolic)
    int piece_walk = 1;      // default mode: one piece of B per wave iteration where every piece has <= 256 entries (env SMM_PIECE_WALK=0: chunk walk)
    int pack12 = 1;          // pack12 payload of B (1.5-byte columns, smm_pack12_*) for the CSR product's four-entries-per-lane piece walk: 1 = where it is
                             // smaller than the 16-bit payload, 0 never, 2 wherever that walk applies (env SMM_PACK12, smm_ctx_tune_pack)
    int pack_stride = 1;     // pack12 pieces at a fixed stride, addressed by row (no descriptor gather in the walk): 1 = where the stride costs at most
                             // half the compact payload again, 0 never, 2 wherever pack12 is chosen (env SMM_PACK_STRIDE, smm_ctx_tune_pack_stride)
    int sym_max_ws = 0;      // widest column slab of that walk (0 = CCS_MAX_WS); B with more columns is walked slab by slab
                             // (smm_ctx_tune_symbolic; tests set it small to reach the slab path with small matrices)
    int sym_dense = 1;       // symbolic walk over operands with dense runs of columns: 0 never, 1 chosen from B (>= 80 % of the neighbouring
                             // entries share a bitmap word), 2 always (tests) -- env SMM_SYM_DENSE, smm_ctx_tune_dense_runs
    int numeric_persist = 1; // smm_numeric: persistent workgroups fed by a unit counter (env SMM_NUMERIC_PERSIST: 0 never, 1 CSR output without triangle, 2 always)
    int s2_ring = 0;         // triple stage 2: 1 = the ring kernel of round 4 (smm_ring.hpp: correct, measured 60-63 ms against 51 at
                             // BASELINE configs[3] -- kept as an alternative, env SMM_S2_RING=1 / smm_ctx_tune_stage2); 0 = the chunk kernel
    int s2_group = 5;        // triple stage 2: k-groups whose blocks follow each other on one XCD and share a tile of T
                             // through its L2 (env SMM_S2_GROUP; at BASELINE configs[3] 1: 58.2, 2: 56.3, 4: 60.1, 5: 54.8,
                             // 7: 54.9, 8: 58.9, 10: 54.8 ms -- powers of two lose, profiles/r2_s2_sweeps.txt)
    int lds_cols = 18000;    // SMM_EXACT walk: accumulator columns per workgroup (x8 B of LDS; 1.5 KB of
    int waves = 8;           // scratch per wave sit behind them) and waves per workgroup (each owns 1/waves)
    int lds_cols_shared = 20000;   // default (shared-tile) walk: tile columns and waves per workgroup
    int waves_shared = 16;
    int hash_small = 256;    // rows of C with <= hash_small nonzeros: one wave per row, LDS hash (0 = off)
    int hash_medium = 2048;  // ... <= hash_medium: one workgroup per row, LDS hash; above: dense LDS tiles
    int tiny_max = TINY_G;   // rows with <= 16 products from <= 16 entries of A: smm_*_tiny, four rows per wave (env SMM_TINY=0: off)
    // row block x column slab kernels (smm_slab.hpp): mode 0 = where they pay, 1 = never, 2 = wherever
    // they can run; ws = slab width (0 = sized so that one slab of B is ~3 MB, L2-resident);
    // rows per wave 2 or 4 (8 waves per workgroup: 16 or 32 rows per block)
    int slab_mode = 0, slab_ws = 0, slab_rw = 4;
    int narrow_idx = 1;      // 1: operands with < 65535 columns go through the symbolic phase as uint16 (column stream and lists)
    int64_t t3_max_t = (int64_t)1 << 27;   // sparse triple product: products of H[b] * Q (an upper bound of nnz(T_b)) per row block
    int masked_mode = 0;                   // masked SpGEMM: 0 per-row cost model, 1 dot path (canonical A only), 2 row path
    int spmm_mode = 0;                     // sparse x dense: 0 rows binned by length, 1 / 2 / 3 every row in the tiny / group / long class
    int64_t apply_budget = (int64_t)1 << 30;   // smm_triple_apply: bytes of the two intermediates of one column block
    int sddmm_mode = 0;                    // sampled dense product: 0 chosen from nnz(mask), 1 interleaved entries, 2 runs of entries
    int interp_stage = 1;                  // smm_interp_fill: 1 = axes of at most IP_STAGE_NODES nodes are searched in LDS, 0 = always through L2 (env SMM_INTERP_STAGE)
    int n_cu = 256;
    std::vector<PoolBlock> pool;          // free blocks
    std::map<void *, size_t> live;        // blocks handed out
    std::vector<TimedLaunch> launches;
    std::map<std::string, std::pair<double, int64_t>> totals;
    // result download (download() below): ring of pinned bounce buffers, allocated on first use
    static constexpr int PIN_SLOTS = 8;
    static constexpr size_t PIN_BYTES = (size_t)32 << 20;
    void *pin[PIN_SLOTS] = {nullptr};
    hipEvent_t pin_ev[PIN_SLOTS] = {nullptr};
    int *cg_live = nullptr;          // smm_innovation_solve: two pinned words for the count of live columns, with their events
    hipEvent_t cg_ev[2] = {nullptr, nullptr};
    int exact_checked = 0;           // SMM_EXACT guard (smm_ctx_exact_selftest): 0 not run yet, 1 passed, -1 failed
    int check = 0;                   // 1: every symbolic phase ends with the plan checker (env SMM_CHECK, smm_ctx_set_check)
    int inject_alloc_nth = 0;        // test hook: the n-th dev_malloc from now fails (its first attempt, or both: _hard)
    bool inject_alloc_hard = false;
    int64_t alloc_retries = 0;       // allocations that needed the pool flushed
    unsigned *d_flags = nullptr;     // [0] validation flags; +64: int -1 and +128: double 0 read by idle lanes
    unsigned *d_err = nullptr;       // plan error word: [0] PLAN_ERR_* bits, [1] lowest row that tripped one (kernels' always-on clamps, plan checker)
    std::recursive_mutex mu;         // every entry point that touches the context takes it: calls from
                                     // several host threads on one context serialise (one stream anyway)
};
#define CTX_LOCK(c) std::lock_guard<std::recursive_mutex> ctx_lock_((c)->mu)

// Return every free block of the context's pool to the device (blocks handed out stay).  hipFree waits for the
// device, so work still queued on blocks that went back to the pool has finished by then.
static void pool_flush(smm_ctx *c)
{
    for (auto &b : c->pool) (void)hipFree(b.p);
    c->pool.clear();
}
// hipMalloc for everything that is not pooled (operands and their cached copies).  An allocation that fails is
// retried once after the pool's free blocks -- the multi-GB lists of closed plans live there -- went back to the
// device; a failure never leaves HIP's sticky last error behind (the next LAUNCH_CHECK would report it).
// Test hook (smm_ctx_inject_alloc_failure): the n-th call from now fails its first attempt -- or both.
static hipError_t dev_malloc(smm_ctx *c, void **p, size_t bytes)
{
    bool fail_first = false, fail_both = false;
    if (c->inject_alloc_nth > 0 && --c->inject_alloc_nth == 0) { fail_first = true; fail_both = c->inject_alloc_hard; }
    hipError_t e = fail_first ? hipErrorOutOfMemory : hipMalloc(p, bytes);
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
    pool_flush(c);
    ++c->alloc_retries;
    e = fail_both ? hipErrorOutOfMemory : hipMalloc(p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; }
    return e;
}

static int pool_alloc(smm_ctx *c, size_t bytes, void **out)
{
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 255) & ~(size_t)255;
    int best = -1;
    for (int i = 0; i < (int)c->pool.size(); ++i)
        if (c->pool[i].bytes >= bytes && c->pool[i].bytes <= bytes + bytes / 4 + (1 << 20) &&
            (best < 0 || c->pool[i].bytes < c->pool[best].bytes))
            best = i;
    if (best >= 0) {
        *out = c->pool[best].p;
        c->live[*out] = c->pool[best].bytes;
        c->pool.erase(c->pool.begin() + best);
        return SMM_OK;
    }
    void *p = nullptr;
    hipError_t e = dev_malloc(c, &p, bytes);           // (drops the pool's free blocks and retries once)
    if (e != hipSuccess) return fail(SMM_ERR_ALLOC, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    c->live[p] = bytes;
    *out = p;
    return SMM_OK;
}
static void pool_free(smm_ctx *c, void *p)
{
    if (!p) return;
    auto it = c->live.find(p);
    if (it == c->live.end()) return;
    c->pool.push_back({p, it->second});
    c->live.erase(it);
}
template <typename T> static int pool_get(smm_ctx *c, size_t count, T **out)
{
    void *p = nullptr;
    int rc = pool_alloc(c, count * sizeof(T), &p);
    *out = (T *)p;
    return rc;
}

// Owner of one pool block: reset() and the destructor hand it back to the pool.  Neither synchronises, and neither
// needs to: the context has one stream, so the pool hands a block out again only to work queued behind everything
// that used it, and pool_flush returns blocks to the device through hipFree, which waits for the device.
template <typename T> struct PoolBuf {
    smm_ctx *c;
    T *p = nullptr;
    explicit PoolBuf(smm_ctx *ctx) : c(ctx) {}
    PoolBuf(PoolBuf &&o) noexcept : c(o.c), p(o.release()) {}
    PoolBuf &operator=(PoolBuf &&o) noexcept { if (this != &o) { reset(); c = o.c; p = o.release(); } return *this; }
    ~PoolBuf() { reset(); }
    int alloc(size_t count) { reset(); return pool_get(c, count, &p); }
    void reset() { pool_free(c, p); p = nullptr; }
    T *release() { T *q = p; p = nullptr; return q; }
    operator T *() const { return p; }
};
// Owner of a dev_malloc'd array, and the record of its size: an operand's own arrays and every cached copy are held
// by one of these for their whole life (smm_csr_device_bytes sums `bytes`).  An empty one never calls into the runtime:
// the row views of csr_row_view die on the stack, possibly on a thread that has no device set.
template <typename T> struct DevBuf {
    T *p = nullptr;
    int64_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); std::swap(p, o.p); std::swap(bytes, o.bytes); } return *this; }
    ~DevBuf() { reset(); }
    hipError_t alloc(smm_ctx *c, size_t count)
    {
        reset();
        const hipError_t e = dev_malloc(c, (void **)&p, count * sizeof(T));
        if (e == hipSuccess) bytes = (int64_t)(count * sizeof(T));
        return e;
    }
    void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    operator T *() const { return p; }
};
// unique_ptr deleter that calls one of the ABI's destroy functions (plans and results under construction)
template <auto Destroy> struct Destroyer {
    template <typename T> void operator()(T *x) const { Destroy(x); }
};

struct LaunchTimer {
    smm_ctx *c; const char *name; hipEvent_t t0 = nullptr, t1 = nullptr;
    LaunchTimer(smm_ctx *ctx, const char *n) : c(ctx), name(n)
    {
        if (c->timing) {
            (void)hipEventCreate(&t0); (void)hipEventCreate(&t1);
            (void)hipEventRecord(t0, c->stream);
        }
    }
    ~LaunchTimer()
    {
        if (c->timing) {
            (void)hipEventRecord(t1, c->stream);
            c->launches.push_back({name, t0, t1});
        }
    }
};
#define LAUNCH(ctx, name, kern, grid, block, lds, ...)                                         \
    do {                                                                                       \
        LaunchTimer lt_(ctx, name);                                                            \
        hipLaunchKernelGGL(kern, dim3((unsigned)(grid)), dim3((unsigned)(block)), (size_t)(lds), \
                           (ctx)->stream, __VA_ARGS__);                                        \
    } while (0)
#define LAUNCH_CHECK() HIPCHK(hipGetLastError())

extern "C" int smm_ctx_create(int device, void *hip_stream, smm_ctx **out)
{
    if (!out) return fail(SMM_ERR_INVALID, "smm_ctx_create: out is NULL");
    *out = nullptr;
    int n = smm_device_count();
    if (n <= 0) return fail(SMM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(SMM_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SMM_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device,
                    prop.gcnArchName);
    smm_ctx *c = new smm_ctx();
    c->device = device;
    if (const char *e = getenv("SMM_NARROW_IDX")) c->narrow_idx = atoi(e) != 0;     // A/B switch (scripts/ab_env.sh)
    if (const char *e = getenv("SMM_S2_GROUP")) c->s2_group = std::max(1, atoi(e));
    if (const char *e = getenv("SMM_S2_RING")) c->s2_ring = atoi(e) != 0;
    if (const char *e = getenv("SMM_NUMERIC_PERSIST")) c->numeric_persist = atoi(e);
    if (const char *e = getenv("SMM_TINY")) c->tiny_max = atoi(e) != 0 ? TINY_G : 0;
    if (const char *e = getenv("SMM_SYM_DENSE")) c->sym_dense = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("SMM_SYM_WIDE")) c->sym_wide = atoi(e) != 0;
    if (const char *e = getenv("SMM_SYM_CCS")) c->sym_ccs = atoi(e) != 0;
    if (const char *e = getenv("SMM_PIECE_WALK")) c->piece_walk = atoi(e);
    if (const char *e = getenv("SMM_PACK12")) c->pack12 = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("SMM_PACK_STRIDE")) c->pack_stride = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("SMM_SYM_MAX_WS")) c->sym_max_ws = std::max(0, std::min(atoi(e), (int)CCS_MAX_WS));
    if (const char *e = getenv("SMM_CHECK")) c->check = atoi(e) != 0;
    if (const char *e = getenv("SMM_INTERP_STAGE")) c->interp_stage = atoi(e) != 0;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hip_stream == SMM_STREAM_DEFAULT) { c->stream = nullptr; c->own_stream = false; }   // the device's null stream
    else if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
    else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return fail(SMM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
        c->own_stream = true;
    }
    if (hipMalloc((void **)&c->d_flags, 512) != hipSuccess) { delete c; return fail(SMM_ERR_ALLOC, "hipMalloc flags"); }    // (+256: bin counts, +288 / +320: row counters)
    {
        unsigned char init[256];
        memset(init, 0, sizeof(init));
        const int neg1 = -1;
        memcpy(init + 64, &neg1, sizeof(neg1));
        if (hipMemcpy(c->d_flags, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(c->d_flags); delete c;
            return fail(SMM_ERR_HIP, "hipMemcpy of the context constants failed");
        }
    }
    {
        const unsigned clean[2] = {0u, 0xffffffffu};
        if (hipMalloc((void **)&c->d_err, 64) != hipSuccess || hipMemcpy(c->d_err, clean, sizeof(clean), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(c->d_err); (void)hipFree(c->d_flags); delete c;
            return fail(SMM_ERR_ALLOC, "hipMalloc of the context's error word failed");
        }
    }
    *out = c;
    return SMM_OK;
}

extern "C" void smm_ctx_destroy(smm_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &l : c->launches) { (void)hipEventDestroy(l.t0); (void)hipEventDestroy(l.t1); }
    for (auto &b : c->pool) (void)hipFree(b.p);
    for (auto &kv : c->live) (void)hipFree(kv.first);
    (void)hipFree(c->d_flags);
    (void)hipFree(c->d_err);
    for (int i = 0; i < smm_ctx::PIN_SLOTS; ++i) {
        if (c->pin[i]) (void)hipHostFree(c->pin[i]);
        if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]);
    }
    if (c->cg_live) (void)hipHostFree(c->cg_live);
    for (hipEvent_t e : c->cg_ev) if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Fetch-and-clear the context's plan error word (what the kernels' always-on clamps and the plan checker record);
// synchronises the stream.  A non-zero word means plan metadata was inconsistent: the result of the product that
// tripped it is not to be trusted, and the caller gets SMM_ERR_INTERNAL -- never a hang or a fault.
static int take_plan_error(smm_ctx *c, const char *where)
{
    unsigned h[16] = {0u};
    HIPCHK(hipMemcpyAsync(h, c->d_err, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!h[0]) return SMM_OK;
    if ((h[0] & PLAN_ERR_RING) && getenv("SMM_DEBUG"))
        fprintf(stderr, "[smm] ring wait ran out: need %u fmin %d pmin %d fp %u step %d wave %u row block %u T_w %u\n", h[8] >> 16, (int)(short)(h[8] & 0xffff),
                (int)h[9] >> 16, h[9] & 0xffff, (int)h[10], h[11] & 0xff, h[11] >> 8, h[12]);
    const unsigned clean[2] = {0u, 0xffffffffu};
    HIPCHK(hipMemcpyAsync(c->d_err, clean, sizeof(clean), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    static const char *names[] = {"sub-run bounds", "tail descriptor", "slab sub-run table", "start slots", "hash look-up",
                                  "list capacity", "row counts", "list entries", "ring schedule / progress words of triple-product stage 2",
                                  "piece lengths of the strided payload"};
    std::string what;
    for (int b = 0; b < 10; ++b)
        if (h[0] & (1u << b)) { if (!what.empty()) what += ", "; what += names[b]; }
    return fail(SMM_ERR_INTERNAL, "%s: inconsistent plan metadata (%s; first at row %u of A) -- the result of this product is not valid; "
                                  "please report this with the operands (SMM_CHECK=1 verifies every plan)", where, what.c_str(), h[1]);
}

extern "C" int smm_ctx_synchronize(smm_ctx *c)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    return take_plan_error(c, "smm_ctx_synchronize");       // (synchronises the stream)
}

extern "C" int smm_ctx_release_pool(smm_ctx *c)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    pool_flush(c);
    return SMM_OK;
}
extern "C" int64_t smm_ctx_pool_bytes(smm_ctx *c)
{
    if (!c) return -1;
    CTX_LOCK(c);
    int64_t t = 0;
    for (auto &b : c->pool) t += (int64_t)b.bytes;
    return t;
}
extern "C" int64_t smm_ctx_live_bytes(smm_ctx *c)
{
    if (!c) return -1;
    CTX_LOCK(c);
    int64_t t = 0;
    for (auto &kv : c->live) t += (int64_t)kv.second;
    return t;
}
extern "C" int smm_ctx_inject_alloc_failure(smm_ctx *c, int nth, int hard)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    c->inject_alloc_nth = nth > 0 ? nth : 0;
    c->inject_alloc_hard = hard != 0;
    return SMM_OK;
}
extern "C" int64_t smm_ctx_alloc_retries(smm_ctx *c)
{
    if (!c) return -1;
    CTX_LOCK(c);
    return c->alloc_retries;
}

extern "C" int smm_ctx_set_check(smm_ctx *c, int enable)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    c->check = enable != 0;
    return SMM_OK;
}

static int drain_timers(smm_ctx *c)
{
    if (c->launches.empty()) return SMM_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &l : c->launches) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, l.t0, l.t1);
        auto &t = c->totals[l.name];
        t.first += ms; t.second += 1;
        (void)hipEventDestroy(l.t0); (void)hipEventDestroy(l.t1);
    }
    c->launches.clear();
    return SMM_OK;
}
extern "C" int smm_ctx_timing(smm_ctx *c, int enable)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(drain_timers(c));
    c->timing = enable != 0;
    return SMM_OK;
}
extern "C" int smm_ctx_timing_reset(smm_ctx *c)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(drain_timers(c));
    c->totals.clear();
    return SMM_OK;
}
extern "C" int smm_ctx_kernel_time(smm_ctx *c, const char *kernel, double *ms_total, int64_t *launches)
{
    if (!c || !kernel) return fail(SMM_ERR_INVALID, "smm_ctx_kernel_time: NULL argument");
    CTX_LOCK(c);
    CHK(drain_timers(c));
    auto it = c->totals.find(kernel);
    if (ms_total) *ms_total = it == c->totals.end() ? 0.0 : it->second.first;
    if (launches) *launches = it == c->totals.end() ? 0 : it->second.second;
    return SMM_OK;
}
extern "C" int smm_ctx_tune(smm_ctx *c, int lds_cols, int waves)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (lds_cols) {
        if (lds_cols < 64 || lds_cols > 20000) return fail(SMM_ERR_INVALID, "lds_cols must be in [64,20000]");
        c->lds_cols = lds_cols;
    }
    if (waves) {
        if (waves != 1 && waves != 2 && waves != 4 && waves != 8 && waves != 16)
            return fail(SMM_ERR_INVALID, "waves must be 1, 2, 4, 8 or 16");
        c->waves = waves;
    }
    return SMM_OK;
}
extern "C" int smm_ctx_tune_hash(smm_ctx *c, int small_max, int medium_max)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (small_max < 0 || small_max > 256 || medium_max < 0 || medium_max > 2048)
        return fail(SMM_ERR_INVALID, "hash thresholds must be in [0,256] and [0,2048]");
    c->hash_small = small_max;
    c->hash_medium = std::max(medium_max, small_max);
    return SMM_OK;
}
extern "C" int smm_ctx_tune_slab(smm_ctx *c, int mode, int ws, int rows_per_wave)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (mode < 0 || mode > 2) return fail(SMM_ERR_INVALID, "slab mode must be 0 (auto), 1 (off) or 2 (force)");
    if (ws < 0 || ws > 32766) return fail(SMM_ERR_INVALID, "slab width must be in [0,32766]");
    if (rows_per_wave != 0 && rows_per_wave != 2 && rows_per_wave != 4)
        return fail(SMM_ERR_INVALID, "rows per wave must be 0 (keep), 2 or 4");
    c->slab_mode = mode;
    c->slab_ws = ws;
    if (rows_per_wave) c->slab_rw = rows_per_wave;
    return SMM_OK;
}
extern "C" int smm_ctx_tune_narrow(smm_ctx *c, int enable)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    c->narrow_idx = enable != 0;
    return SMM_OK;
}
extern "C" int smm_ctx_tune_symbolic(smm_ctx *c, int max_slab_cols)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (max_slab_cols < 0 || max_slab_cols > CCS_MAX_WS) return fail(SMM_ERR_INVALID, "slab width must be in [0,%d]", CCS_MAX_WS);
    c->sym_max_ws = max_slab_cols;
    return SMM_OK;
}
extern "C" int smm_ctx_tune_dense_runs(smm_ctx *c, int mode)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (mode < 0 || mode > 2) return fail(SMM_ERR_INVALID, "mode must be 0 (never), 1 (chosen from the operand) or 2 (always)");
    c->sym_dense = mode;
    return SMM_OK;
}
extern "C" int smm_ctx_tune_stage2(smm_ctx *c, int ring)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    c->s2_ring = ring != 0;
    return SMM_OK;
}
extern "C" int smm_ctx_tune_pack(smm_ctx *c, int mode)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (mode < 0 || mode > 2) return fail(SMM_ERR_INVALID, "mode must be 0 (never), 1 (where smaller) or 2 (wherever the walk applies)");
    c->pack12 = mode;
    return SMM_OK;
}
extern "C" int smm_ctx_tune_pack_stride(smm_ctx *c, int mode)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (mode < 0 || mode > 2) return fail(SMM_ERR_INVALID, "mode must be 0 (never), 1 (where the stride fits the capacity rule) or 2 (wherever pack12 is chosen)");
    c->pack_stride = mode;
    return SMM_OK;
}
extern "C" int smm_ctx_tune_shared(smm_ctx *c, int lds_cols, int waves)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (lds_cols) {
        if (lds_cols < 64 || lds_cols > 20000) return fail(SMM_ERR_INVALID, "lds_cols must be in [64,20000]");
        c->lds_cols_shared = lds_cols;
    }
    if (waves) {
        if (waves != 4 && waves != 8 && waves != 16) return fail(SMM_ERR_INVALID, "waves must be 4, 8 or 16");
        c->waves_shared = waves;
    }
    return SMM_OK;
}

// ------------------------------------------------------------------------------ SMM_EXACT guard
extern "C" int smm_ctx_exact_selftest(smm_ctx *c, int inject_fault)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    unsigned *d_bad = (unsigned *)((char *)c->d_flags + 240);
    HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(unsigned), c->stream));
    constexpr int NTRIAL = 16384;
    LAUNCH(c, "smm_lds_order_selftest", smm_lds_order_selftest, 512, 64, 0, NTRIAL, inject_fault ? 1 : 0, d_bad);
    LAUNCH_CHECK();
    unsigned bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad)
        return fail(SMM_ERR_UNSUPPORTED,
                    "SMM_EXACT self-test failed: %u of %d accumulators differ from the lane-ordered sum%s -- this device does not "
                    "apply the lanes of one ds_add_f64 in ascending lane order, so reference-order (bit-exact) accumulation is "
                    "not available; run without SMM_EXACT (values agree to rounding)",
                    bad, NTRIAL * 32, inject_fault ? " (fault injected)" : "");
    return SMM_OK;
}
// every SMM_EXACT product goes through this first; the kernel runs once per context
static int exact_guard(smm_ctx *c, int flags)
{
    if (!(flags & SMM_EXACT) || c->exact_checked > 0) return SMM_OK;
    if (c->exact_checked == 0) {
        const char *e = getenv("SMM_EXACT_INJECT_FAULT");
        const int rc = smm_ctx_exact_selftest(c, e && *e && strcmp(e, "0") != 0);
        if (rc != SMM_OK && rc != SMM_ERR_UNSUPPORTED) return rc;      // could not run: try again next time
        c->exact_checked = rc == SMM_OK ? 1 : -1;
        if (rc != SMM_OK) return rc;
        return SMM_OK;
    }
    return fail(SMM_ERR_UNSUPPORTED, "SMM_EXACT is not available on this device (its self-test failed earlier on this context)");
}

// ------------------------------------------------------------------------------ host-side content hash
// h' = rotl(h ^ w, 27) * P is a bijection of h for a fixed word and of the word for a fixed h: a buffer that
// differs from another in one 8-byte word gives a different lane state from there on, whatever follows.
// Blocks of 4 MB are hashed independently (four interleaved lanes each; by several threads when the buffer
// is large) and their hashes are chained in order by the same step.
static inline uint64_t hash_step(uint64_t h, uint64_t w)
{
    h ^= w;
    h = (h << 27) | (h >> 37);
    return h * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
}
static inline uint64_t hash_final(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
static uint64_t hash_block(const unsigned char *p, size_t bytes)
{
    uint64_t h0 = 0x243F6A8885A308D3ull, h1 = 0x13198A2E03707344ull, h2 = 0xA4093822299F31D0ull, h3 = 0x082EFA98EC4E6C89ull;
    size_t i = 0;
    for (; i + 32 <= bytes; i += 32) {
        uint64_t w0, w1, w2, w3;
        memcpy(&w0, p + i, 8); memcpy(&w1, p + i + 8, 8); memcpy(&w2, p + i + 16, 8); memcpy(&w3, p + i + 24, 8);
        h0 = hash_step(h0, w0); h1 = hash_step(h1, w1); h2 = hash_step(h2, w2); h3 = hash_step(h3, w3);
    }
    for (; i < bytes; i += 8) {                         // tail: whole words, the last one zero-padded
        uint64_t w = 0;
        memcpy(&w, p + i, std::min<size_t>(8, bytes - i));
        h0 = hash_step(h0, w);
    }
    uint64_t h = hash_step(hash_step(hash_step(hash_step(0x452821E638D01377ull, h0), h1), h2), h3);
    return hash_step(h, (uint64_t)bytes);
}
extern "C" uint64_t smm_host_hash64(const void *ptr, int64_t nbytes)
{
    if (!ptr || nbytes <= 0) return hash_final(0x9E3779B97F4A7C15ull);
    const unsigned char *p = (const unsigned char *)ptr;
    const size_t bytes = (size_t)nbytes;
    constexpr size_t BLK = (size_t)4 << 20;
    const size_t nblk = (bytes + BLK - 1) / BLK;
    std::vector<uint64_t> hb(nblk);
    auto run = [&](size_t b0, size_t stride) {
        for (size_t b = b0; b < nblk; b += stride) hb[b] = hash_block(p + b * BLK, std::min(BLK, bytes - b * BLK));
    };
    unsigned nt = 1;
    if (nblk >= 4) {
        unsigned hw = std::thread::hardware_concurrency();
        if (const char *e = getenv("SMM_HASH_THREADS")) hw = (unsigned)std::max(1, atoi(e));
        nt = (unsigned)std::min<size_t>(std::min<unsigned>(hw ? hw : 1, 8), nblk);
    }
    if (nt <= 1) run(0, 1);
    else {
        // (a thread that cannot be started -- resource limits -- must not throw across the C ABI: its blocks are
        // hashed by this thread instead; the result does not depend on who hashes which block)
        std::vector<std::thread> th;
        std::vector<unsigned> inline_lanes;
        for (unsigned t = 1; t < nt; ++t) {
            try { th.emplace_back(run, (size_t)t, (size_t)nt); }
            catch (...) { inline_lanes.push_back(t); }
        }
        run(0, nt);
        for (unsigned t : inline_lanes) run(t, nt);
        for (auto &t : th) t.join();
    }
    uint64_t h = 0x3F84D5B5B5470917ull;
    for (size_t b = 0; b < nblk; ++b) h = hash_step(h, hb[b]);
    return hash_final(hash_step(h, (uint64_t)bytes));
}

// ------------------------------------------------------------------------------ result download
// Device -> host copy of a result into the caller's (pageable, usually freshly allocated) array
// (reference: sparsemat_to_csr / darray_to_numpy copy the result out, matrix_ops.py:205-240).  One big
// hipMemcpy into such memory runs at the speed of ONE thread taking page faults 4 KB at a time.  Here:
//  * the destination is first advised to use transparent huge pages (512x fewer faults where the kernel
//    allows it; harmless where it does not);
//  * chunks of 32 MB travel by DMA into a ring of pinned buffers on the context's stream, and a few host
//    threads copy finished chunks into the destination in parallel -- so the faults are taken by several
//    threads and overlap with the DMA of the following chunks.
// Small results take the plain copy (measured: at 118 MB the pipeline's start-up still cost 5 ms more than it
// saved, at 265 MB it was ahead).
// widen: the source holds int32, the destination receives int64 (CSR column indices of a result whose nnz
// does not fit int32: scipy wants indptr and indices of one dtype); `bytes` counts SOURCE bytes.
static int download(smm_ctx *c, void *dst, const void *src_dev, size_t bytes, bool widen = false)
{
    if (bytes == 0) return SMM_OK;
    static const bool plain = getenv("SMM_DOWNLOAD_PLAIN") != nullptr;      // A/B switch for scripts/api_e2e.py
    if ((bytes < ((size_t)256 << 20) || plain) && !widen) {
        HIPCHK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    }
    constexpr int R = smm_ctx::PIN_SLOTS;
    constexpr size_t CH = smm_ctx::PIN_BYTES;
    for (int i = 0; i < R; ++i) {
        if (!c->pin[i]) {
            if (hipHostMalloc(&c->pin[i], CH, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                c->pin[i] = nullptr;
                if (widen) return fail(SMM_ERR_ALLOC, "hipHostMalloc of the download ring failed");
                HIPCHK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));   // no pinned memory: plain copy
                HIPCHK(hipStreamSynchronize(c->stream));
                return SMM_OK;
            }
            HIPCHK(hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
        }
    }
    {   // huge pages for the page-aligned interior of the destination
        const size_t pg = (size_t)2 << 20;
        const size_t dbytes = widen ? 2 * bytes : bytes;
        const uintptr_t lo = ((uintptr_t)dst + pg - 1) & ~(uintptr_t)(pg - 1), hi = ((uintptr_t)dst + dbytes) & ~(uintptr_t)(pg - 1);
        if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
    }
    const size_t nchunks = (bytes + CH - 1) / CH;
    const int W = (int)std::min<size_t>(4, nchunks);
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> issued(nchunks, 0), copied(nchunks, 0);
    hipError_t worker_err = hipSuccess;
    auto worker = [&](int w) {
        (void)hipSetDevice(c->device);
        for (size_t i = (size_t)w; i < nchunks; i += (size_t)W) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return issued[i] != 0; });
                if (issued[i] == 2) return;                         // the issuing side failed: stop
            }
            const hipError_t e = hipEventSynchronize(c->pin_ev[i % R]);
            const size_t off = i * CH, len = std::min(CH, bytes - off);
            if (e == hipSuccess) {
                if (!widen) memcpy((char *)dst + off, c->pin[i % R], len);
                else {
                    const int32_t *sp = (const int32_t *)c->pin[i % R];
                    int64_t *dp = (int64_t *)dst + off / sizeof(int32_t);
                    for (size_t k = 0; k < len / sizeof(int32_t); ++k) dp[k] = sp[k];
                }
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                if (e != hipSuccess) worker_err = e;
                copied[i] = 1;
            }
            cv.notify_all();
        }
    };
    std::vector<std::thread> threads;
    bool spawned = true;
    try {
        for (int w = 0; w < W; ++w) threads.emplace_back(worker, w);
    } catch (...) {                                     // (resource limits: nothing may throw across the C ABI)
        spawned = false;
    }
    if (!spawned) {
        // the workers that did start are told to stop; this thread moves the chunks alone, one at a time
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t k = 0; k < nchunks; ++k) issued[k] = 2;
        }
        cv.notify_all();
        for (auto &t : threads) t.join();
        for (size_t i = 0; i < nchunks; ++i) {
            const size_t off = i * CH, len = std::min(CH, bytes - off);
            HIPCHK(hipMemcpyAsync(c->pin[0], (const char *)src_dev + off, len, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (!widen) memcpy((char *)dst + off, c->pin[0], len);
            else {
                const int32_t *sp = (const int32_t *)c->pin[0];
                int64_t *dp = (int64_t *)dst + off / sizeof(int32_t);
                for (size_t k = 0; k < len / sizeof(int32_t); ++k) dp[k] = sp[k];
            }
        }
        return SMM_OK;
    }
    hipError_t err = hipSuccess;
    for (size_t i = 0; i < nchunks; ++i) {
        if (i >= (size_t)R) {                                       // the slot's previous chunk must have left it
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return copied[i - R] != 0; });
        }
        const size_t off = i * CH, len = std::min(CH, bytes - off);
        if (err == hipSuccess) err = hipMemcpyAsync(c->pin[i % R], (const char *)src_dev + off, len, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipEventRecord(c->pin_ev[i % R], c->stream);
        {
            std::lock_guard<std::mutex> lk(mu);
            issued[i] = err == hipSuccess ? 1 : 2;
            if (err != hipSuccess)
                for (size_t k = i; k < nchunks; ++k) issued[k] = 2;
        }
        cv.notify_all();
        if (err != hipSuccess) break;
    }
    for (auto &t : threads) t.join();
    if (err == hipSuccess) err = worker_err;
    if (err != hipSuccess) { (void)hipGetLastError(); return fail(SMM_ERR_HIP, "result download: %s", hipGetErrorString(err)); }
    return SMM_OK;
}

// ------------------------------------------------------------------------------ operands
using CsrPtr = std::unique_ptr<smm_csr, Destroyer<smm_csr_destroy>>;
struct smm_csr {
    smm_ctx *ctx = nullptr;
    int64_t rows = 0, cols = 0, nnz = 0;
    const int *ptr = nullptr, *idx = nullptr;    // what everything reads: own_* below, or the caller's arrays (smm_csr_from_device)
    const double *val = nullptr;
    DevBuf<int> own_ptr, own_idx; DevBuf<double> own_val;    // empty for a borrowed operand
    bool owned() const { return own_ptr.p != nullptr; }
    bool validated = false;
    unsigned vflags = 0;
    // Cached copies.  Every entry owns its arrays; plans and launch code get plain values (a raw pointer, or a *View),
    // never a pointer into a vector here, which may grow.  The device arrays themselves never move once built.
    // cached tile indices (sorted operands only), one per tile geometry that has been asked for:
    // plans keep the pointer of theirs, so a later product with another geometry (SMM_EXACT vs
    // default, another tuning, the ELL chunks of the triple product) never invalidates it
    struct SegCache { int wf, n_ft; DevBuf<int> seg; };
    struct LocCache { int wc; DevBuf<short> loc; };   // tile-local columns for coarse width wc
    // slab-major copy (smm_slab.hpp); seg: the tile index it was built from (one of segs), as in the entries below
    struct SlabView { int ws, n_slabs; int *soff; short *scol; double *sval; };
    struct SlabCache {
        int ws, n_slabs; const int *seg; DevBuf<int> soff; DevBuf<short> scol; DevBuf<double> sval;
        SlabView view() const { return {ws, n_slabs, soff, scol, sval}; }
    };
    // packed tile-major payload (smm_pack_*), one entry per (tile geometry, format); maxlen: longest piece (fmt 0: entries;
    // PACK_FMT_12: slots n).  A pack12 entry always holds the counts it was judged by (units16 / units12: the operand as
    // either format, in 8-byte units) and its arrays only once a product chose it.  It can hold its pieces twice: back to
    // back behind descriptors (desc / pay) and at a fixed stride behind a length table (len16 / spay, stride in units;
    // see smm_pack12_len16) -- each built when a product first chooses it, so both only after SMM_PACK_STRIDE changed.
    struct PackView { int wc, nct; int2 *desc; double *pay; int maxlen; int fmt; unsigned short *len16 = nullptr; int stride = 0; };
    struct PackCache {
        int wc, nct; const int *seg; DevBuf<int2> desc; DevBuf<double> pay; int maxlen; int fmt; int64_t units16, units12;
        DevBuf<unsigned short> len16; DevBuf<double> spay; int stride = 0;
        PackView view(bool strided = false) const
        {
            if (strided) return {wc, nct, nullptr, spay, maxlen, fmt, len16, stride};
            return {wc, nct, desc, pay, maxlen, fmt, nullptr, 0};
        }
    };
    // chunk-padded 16-bit column stream per column slab (smm_ccs_*): the symbolic phase's gather stream
    // (same_word: share of neighbouring entries in one bitmap word)
    struct CcsView { int ws, n_slabs, bm_words, guard_chunk; int *cptr; unsigned short *stream; double same_word; };
    struct CcsCache {
        int ws, n_slabs, bm_words, guard_chunk; DevBuf<int> cptr; DevBuf<unsigned short> stream; double same_word;
        CcsView view() const { return {ws, n_slabs, bm_words, guard_chunk, cptr, stream, same_word}; }
    };
    // sliced-ELL copy for triple-product stage 2 (chunk width `chunk`); built = val holds an array
    struct EllCopy { int chunk = 0, nchunks = 0; bool spread = false; const int *seg = nullptr; DevBuf<int64_t> off; DevBuf<short> col; DevBuf<double> val; };
    // scheduled streams for the ring kernel of triple-product stage 2 (smm_ring.hpp), one per (k-group, wave)
    struct RingCopy { int npieces = 0; bool spread = false; DevBuf<int64_t> off; DevBuf<short> col; DevBuf<double> val; DevBuf<unsigned> hdr; };
    std::vector<SegCache> segs;
    std::vector<LocCache> locs;
    std::vector<SlabCache> slabs;
    std::vector<PackCache> packs;
    std::vector<CcsCache> ccs;
    DevBuf<unsigned short> idx16;                // 16-bit copy of idx (cols < 65535): the symbolic phase's gather stream
    DevBuf<int> idx_pad;                         // borrowed operands with >= 65535 columns: a copy of idx with two ints of slack (wide symbolic walk)
    EllCopy ell;
    RingCopy ring;
    CsrPtr tr;                                   // H^T for the sparse triple product (pattern only: update_values leaves it)
    CsrPtr trv;                                  // A^T with values: the masked SpGEMM's dot path (B^T), the transposed sparse x dense
                                                 // product and H^T of smm_triple_apply; built on first use, update_values drops it
};

// Rows [r0, r0 + nr) of a validated h as a borrowed operand without any of h's caches.  The row pointer is not rebased:
// kernels use ptr[row] and ptr[row + 1] only as absolute positions in idx / val.
static smm_csr csr_row_view(const smm_csr *h, int64_t r0, int64_t nr)
{
    smm_csr v;
    v.ctx = h->ctx; v.rows = nr; v.cols = h->cols; v.nnz = h->nnz;
    v.ptr = h->ptr + r0; v.idx = h->idx; v.val = h->val;
    v.validated = h->validated; v.vflags = h->vflags;
    return v;
}

static int validate(smm_ctx *c, smm_csr *m)
{
    if (m->validated) return (m->vflags & CSR_BAD) ? fail(SMM_ERR_INVALID, "malformed CSR operand") : SMM_OK;
    HIPCHK(hipMemsetAsync(c->d_flags, 0, sizeof(unsigned), c->stream));
    const int grid = (int)std::min<int64_t>(std::max<int64_t>((m->rows + 3) / 4, 1), 8192);
    LAUNCH(c, "smm_validate", smm_validate, grid, 256, 0, (int)m->rows, (int)m->cols, (int)m->nnz, m->ptr, m->idx,
           c->d_flags);
    LAUNCH_CHECK();
    unsigned f = 0;
    HIPCHK(hipMemcpyAsync(&f, c->d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    m->vflags = f;
    m->validated = true;
    if (f & CSR_BAD)
        return fail(SMM_ERR_INVALID, "malformed CSR operand (non-monotone indptr or column index out of range)");
    return SMM_OK;
}

static int csr_common(smm_ctx *c, int64_t rows, int64_t cols, int64_t nnz)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    if (rows < 0 || cols < 0 || nnz < 0) return fail(SMM_ERR_INVALID, "negative dimension");
    if (rows >= INT32_MAX || cols >= INT32_MAX || nnz >= INT32_MAX)
        return fail(SMM_ERR_INVALID, "operand dimensions/nnz must be < 2^31 (int32 indices, as the reference)");
    HIPCHK(hipSetDevice(c->device));
    return SMM_OK;
}

static CsrPtr new_csr(smm_ctx *c, int64_t rows, int64_t cols, int64_t nnz)
{
    CsrPtr m(new smm_csr());
    m->ctx = c; m->rows = rows; m->cols = cols; m->nnz = nnz;
    return m;
}
// The three arrays of an operand that owns them (idx with 2 ints of slack: the wide symbolic walk reads columns in pairs).
static int alloc_owned(smm_ctx *c, smm_csr *m, const char *what)
{
    const size_t n = (size_t)std::max<int64_t>(m->nnz, 1);
    if (m->own_ptr.alloc(c, (size_t)m->rows + 1) != hipSuccess || m->own_idx.alloc(c, n + 2) != hipSuccess || m->own_val.alloc(c, n) != hipSuccess)
        return fail(SMM_ERR_ALLOC, "hipMalloc of %s failed", what);
    m->ptr = m->own_ptr; m->idx = m->own_idx; m->val = m->own_val;
    return SMM_OK;
}

extern "C" int smm_csr_from_host(smm_ctx *c, int64_t rows, int64_t cols, int64_t nnz, const int32_t *indptr,
                                 const int32_t *indices, const double *data, smm_csr **out)
{
    if (!out) return fail(SMM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    CHK(csr_common(c, rows, cols, nnz));
    CTX_LOCK(c);
    if (!indptr || (nnz > 0 && (!indices || !data))) return fail(SMM_ERR_INVALID, "NULL CSR array");
    CsrPtr m = new_csr(c, rows, cols, nnz);
    CHK(alloc_owned(c, m.get(), "a CSR operand"));
    HIPCHK(hipMemcpyAsync(m->own_ptr, indptr, (rows + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(m->own_idx, indices, nnz * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(m->own_val, data, nnz * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    CHK(validate(c, m.get()));
    *out = m.release();
    return SMM_OK;
}

extern "C" int smm_csr_from_device(smm_ctx *c, int64_t rows, int64_t cols, int64_t nnz, const int32_t *d_indptr,
                                   const int32_t *d_indices, const double *d_data, smm_csr **out)
{
    if (!out) return fail(SMM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    CHK(csr_common(c, rows, cols, nnz));
    CTX_LOCK(c);
    if (!d_indptr || (nnz > 0 && (!d_indices || !d_data))) return fail(SMM_ERR_INVALID, "NULL CSR array");
    CsrPtr m = new_csr(c, rows, cols, nnz);
    m->ptr = d_indptr; m->idx = d_indices; m->val = d_data;
    CHK(validate(c, m.get()));
    *out = m.release();
    return SMM_OK;
}

// (every array the handle owns, and its transposes, go with it: the members' destructors)
extern "C" void smm_csr_destroy(smm_csr *m)
{
    if (!m) return;
    CTX_LOCK(m->ctx);
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    delete m;
}
extern "C" int64_t smm_csr_rows(const smm_csr *m) { return m ? m->rows : -1; }
extern "C" int64_t smm_csr_cols(const smm_csr *m) { return m ? m->cols : -1; }
extern "C" int64_t smm_csr_nnz(const smm_csr *m) { return m ? m->nnz : -1; }
extern "C" int smm_csr_is_canonical(smm_ctx *c, smm_csr *m)
{
    if (!c || !m) return fail(SMM_ERR_INVALID, "NULL argument");
    CTX_LOCK(c);
    CHK(validate(c, m));
    return (m->vflags & (CSR_UNSORTED | CSR_HAS_EQUAL)) ? 0 : 1;
}

extern "C" int64_t smm_csr_device_bytes(const smm_csr *m)
{
    if (!m) return -1;
    CTX_LOCK(m->ctx);
    // HBM of everything the handle owns: what each array's owner recorded when it allocated it
    int64_t total = m->own_ptr.bytes + m->own_idx.bytes + m->own_val.bytes + m->idx16.bytes + m->idx_pad.bytes;
    for (auto &e : m->segs) total += e.seg.bytes;
    for (auto &e : m->locs) total += e.loc.bytes;
    for (auto &e : m->slabs) total += e.soff.bytes + e.scol.bytes + e.sval.bytes;
    for (auto &e : m->packs) total += e.desc.bytes + e.pay.bytes + e.len16.bytes + e.spay.bytes;
    for (auto &e : m->ccs) total += e.cptr.bytes + e.stream.bytes;
    total += m->ell.off.bytes + m->ell.col.bytes + m->ell.val.bytes;
    total += m->ring.off.bytes + m->ring.col.bytes + m->ring.val.bytes + m->ring.hdr.bytes;
    return total + (m->tr ? smm_csr_device_bytes(m->tr.get()) : 0) + (m->trv ? smm_csr_device_bytes(m->trv.get()) : 0);
}

// Tile geometry: nct coarse tiles of wc = nw*wf columns; fine tile t covers [t*wf,(t+1)*wf).
struct Geom { int nct, wc, wf, n_ft, nw; };
// n tiles of width w, one wave: the tile index behind a packed payload, a slab copy, a column stream, the ELL chunks
static Geom tiles_geom(int n, int w) { return Geom{n, w, w, n, 1}; }
static Geom make_geom(const smm_ctx *c, int64_t ncols, const smm_csr *b, bool exact)
{
    Geom g;
    if (!exact) {
        // shared-tile walk: one coarse tile per workgroup, waves split the chunks; the tile
        // index has one entry per coarse tile
        g.nw = c->waves_shared;
        const int64_t cols = std::max<int64_t>(ncols, 1);
        g.nct = (int)((cols + c->lds_cols_shared - 1) / c->lds_cols_shared);
        g.wc = (int)((cols + g.nct - 1) / g.nct);
        g.wf = g.wc;
        g.n_ft = g.nct;
        return g;
    }
    // exact walk: wave w of the workgroup owns fine tile w of the coarse tile; LDS also holds
    // sizeof(ExactScratch) per wave behind the accumulators
    g.nw = c->waves;
    const int64_t cols = std::max<int64_t>(ncols, 1);
    const int64_t lds_max = ((int64_t)160 * 1024 - (int64_t)g.nw * (int64_t)sizeof(ExactScratch) - 64 * 8) / 8 - 2;
    const int64_t wc_max = std::max<int64_t>(std::min<int64_t>(c->lds_cols, lds_max), g.nw);
    g.nct = (int)((cols + wc_max - 1) / wc_max);
    const int64_t per = (cols + g.nct - 1) / g.nct;
    g.wf = (int)((per + g.nw - 1) / g.nw);
    g.wc = g.wf * g.nw;
    if (g.wc > wc_max) {                      // rounding up to a multiple of nw overshot the LDS budget
        g.nct += 1;
        g.wf = (int)(((cols + g.nct - 1) / g.nct + g.nw - 1) / g.nw);
        g.wc = g.wf * g.nw;
    }
    g.n_ft = g.nct * g.nw;
    return g;
}

static int ensure_seg(smm_ctx *c, smm_csr *b, const Geom &g, const int **out)
{
    for (auto &e : b->segs)
        if (e.wf == g.wf && e.n_ft == g.n_ft) { *out = e.seg; return SMM_OK; }
    const int64_t total = b->rows * (int64_t)(g.n_ft + 1);
    DevBuf<int> seg;
    if (seg.alloc(c, std::max<int64_t>(total, 1)) != hipSuccess) return fail(SMM_ERR_ALLOC, "hipMalloc of the tile index failed");
    if (total > 0) {
        LAUNCH(c, "smm_segptr", smm_segptr, (total + 255) / 256, 256, 0, (int)b->rows, g.n_ft, g.wf, b->ptr, b->idx, seg);
        LAUNCH_CHECK();
    }
    *out = seg;
    b->segs.push_back({g.wf, g.n_ft, std::move(seg)});
    return SMM_OK;
}

static int ensure_idx16(smm_ctx *c, smm_csr *b)
{
    if (b->idx16) return SMM_OK;
    if (b->cols >= 65535) return fail(SMM_ERR_INVALID, "16-bit column copy needs < 65535 columns");
    // + 2 entries of slack: the wide symbolic walk reads columns in pairs
    DevBuf<unsigned short> idx16;
    if (idx16.alloc(c, std::max<int64_t>(b->nnz, 1) + 2) != hipSuccess) return fail(SMM_ERR_ALLOC, "hipMalloc of the 16-bit column copy failed");
    if (b->nnz > 0) {
        LAUNCH(c, "smm_idx16", smm_idx16, std::min<int64_t>((b->nnz + 255) / 256, 65536), 256, 0, (int)b->nnz, b->idx, idx16);
        LAUNCH_CHECK();
    }
    b->idx16 = std::move(idx16);
    return SMM_OK;
}

// The wide 32-bit symbolic walk loads columns in pairs, so the pair of a row's last, odd entry reaches one int
// past the array.  Arrays this library allocated carry that slack; a BORROWED array (smm_csr_from_device) ends
// where the caller's allocation may end, so the walk reads a padded copy of it instead (made once per handle).
static int idx_with_slack(smm_ctx *c, smm_csr *b, const int **out)
{
    if (b->owned()) { *out = b->idx; return SMM_OK; }
    if (!b->idx_pad) {
        const size_t n = (size_t)std::max<int64_t>(b->nnz, 1) + 2;
        DevBuf<int> pad;
        if (pad.alloc(c, n) != hipSuccess) return fail(SMM_ERR_ALLOC, "hipMalloc of the padded column copy failed");
        HIPCHK(hipMemsetAsync(pad + (n - 2), 0, 2 * sizeof(int), c->stream));
        if (b->nnz > 0) HIPCHK(hipMemcpyAsync(pad, b->idx, (size_t)b->nnz * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        b->idx_pad = std::move(pad);
    }
    *out = b->idx_pad;
    return SMM_OK;
}

static int ensure_loc(smm_ctx *c, smm_csr *b, const Geom &g, const short **out)
{
    for (auto &e : b->locs)
        if (e.wc == g.wc) { *out = e.loc; return SMM_OK; }
    if (g.wc > 32767) return fail(SMM_ERR_INVALID, "coarse tile wider than 32767 columns");
    DevBuf<short> loc;
    if (loc.alloc(c, std::max<int64_t>(b->nnz, 1)) != hipSuccess) return fail(SMM_ERR_ALLOC, "hipMalloc of the tile-local column array failed");
    if (b->nnz > 0) {
        LAUNCH(c, "smm_loc16", smm_loc16, std::min<int64_t>((b->nnz + 255) / 256, 65536), 256, 0, (int)b->nnz, g.wc, b->idx, loc);
        LAUNCH_CHECK();
    }
    *out = loc;
    b->locs.push_back({g.wc, std::move(loc)});
    return SMM_OK;
}

// Sliced-ELL re-layout of H for triple-product stage 2 (see smm_triple_stage2); one copy is cached per
// handle, for one chunk width and one order of the steps (spread = any order inside a segment, the default
// mode's; otherwise stored order with idle steps, SMM_EXACT's -- smm_ell_fill).
static EllArgs ell_args(const smm_csr *h, const smm_csr::EllCopy &e)
{
    EllArgs E{};
    E.n = (int)h->rows; E.nchunks = e.nchunks; E.chunk = e.chunk; E.nslices = (int)((h->rows + WAVE - 1) / WAVE);
    E.h_ptr = h->ptr; E.h_idx = h->idx; E.h_val = h->val; E.hseg = e.seg;
    E.off = e.off; E.col = e.col; E.val = e.val;
    return E;
}
// The payload of e from h's current values (one wave per (chunk, slice)); queued, not checked.
static void ell_fill(smm_ctx *c, const smm_csr *h, const smm_csr::EllCopy &e)
{
    const EllArgs E = ell_args(h, e);
    const int64_t items = (int64_t)E.nchunks * E.nslices;
    auto kern = e.spread ? smm_ell_fill<1> : smm_ell_fill<2>;
    if (items > 0) LAUNCH(c, "smm_ell_fill", kern, (int)((items + 3) / 4), 256, 0, E);
}
static int ensure_ell(smm_ctx *c, smm_csr *h, int nchunks, int chunk, bool spread)
{
    if (h->ell.val && h->ell.chunk == chunk && h->ell.nchunks == nchunks && h->ell.spread == spread) return SMM_OK;
    smm_csr::EllCopy e;                                 // built here, then put in the old copy's place
    e.chunk = chunk; e.nchunks = nchunks; e.spread = spread;
    CHK(ensure_seg(c, h, tiles_geom(nchunks, chunk), &e.seg));
    const int64_t items = (int64_t)nchunks * ((h->rows + WAVE - 1) / WAVE);
    if (items >= 0x7fffffff) return fail(SMM_ERR_INVALID, "H too large for the sliced-ELL index (%lld blocks)", (long long)items);
    PoolBuf<int64_t> cnt(c);
    CHK(cnt.alloc((size_t)items));
    if (e.off.alloc(c, (size_t)items + 1) != hipSuccess) return fail(SMM_ERR_ALLOC, "hipMalloc of the ELL index failed");
    EllArgs E = ell_args(h, e);
    E.cnt = cnt;
    LAUNCH(c, "smm_ell_count", smm_ell_count, (int)((items + 3) / 4), 256, 0, E);
    LAUNCH(c, "smm_scan", smm_scan<int64_t>, 1, 1024, 0, (int)items, (const int64_t *)cnt, e.off.p);
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, e.off + items, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    cnt.reset();
    // + one wave of slack: stage 2 requests step 0 of a block before it knows the block is empty
    if (e.col.alloc(c, total + WAVE) != hipSuccess || e.val.alloc(c, total + WAVE) != hipSuccess)
        return fail(SMM_ERR_ALLOC, "hipMalloc of the ELL payload (%lld entries) failed", (long long)total);
    ell_fill(c, h, e);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));            // nothing queued reads the old copy any more
    h->ell = std::move(e);
    return SMM_OK;
}

// Scheduled streams of H for the ring kernel of triple-product stage 2 (smm_ring.hpp); one copy cached per handle and
// order (spread = default mode: a lane picks among its next 8 entries; otherwise stored order, SMM_EXACT).
static RingBuildArgs ring_args(smm_ctx *c, const smm_csr *h, const smm_csr::RingCopy &e)
{
    RingBuildArgs B{};
    B.n = (int)h->rows; B.K = (int)h->cols; B.npieces = e.npieces; B.nkg = (int)((h->rows + 16 * WAVE - 1) / (16 * WAVE));
    B.h_ptr = h->ptr; B.h_idx = h->idx; B.h_val = h->val;
    B.off = e.off; B.col = e.col; B.val = e.val; B.hdr = e.hdr; B.err = c->d_err;
    return B;
}
// The streams of e from h's current values (the build kernel's second pass); queued, not checked.
static void ring_fill(smm_ctx *c, const smm_csr *h, const smm_csr::RingCopy &e)
{
    const RingBuildArgs B = ring_args(c, h, e);
    auto kern = e.spread ? smm_ring_build<8, true> : smm_ring_build<1, true>;
    LAUNCH(c, "smm_ring_build", kern, B.nkg, 1024, 0, B);
}
static int ensure_ring(smm_ctx *c, smm_csr *h, bool spread)
{
    const int npieces = (int)((h->cols + RING_PW - 1) / RING_PW);
    if (h->ring.val && h->ring.npieces == npieces && h->ring.spread == spread) return SMM_OK;
    smm_csr::RingCopy e;                                // built here, then put in the old copy's place
    e.npieces = npieces; e.spread = spread;
    PoolBuf<int64_t> cnt(c);
    RingBuildArgs B = ring_args(c, h, e);
    const int64_t streams = (int64_t)B.nkg * 16;
    CHK(cnt.alloc((size_t)streams));
    if (e.off.alloc(c, (size_t)streams + 1) != hipSuccess) return fail(SMM_ERR_ALLOC, "hipMalloc of the ring stream index failed");
    B.cnt = cnt; B.off = e.off;
    auto count = spread ? smm_ring_build<8, false> : smm_ring_build<1, false>;
    LAUNCH(c, "smm_ring_build", count, B.nkg, 1024, 0, B);
    LAUNCH(c, "smm_scan", smm_scan<int64_t>, 1, 1024, 0, (int)streams, (const int64_t *)cnt, e.off.p);
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, e.off + streams, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    cnt.reset();
    if (e.col.alloc(c, (size_t)(total + 1) * WAVE) != hipSuccess || e.val.alloc(c, (size_t)(total + 1) * WAVE) != hipSuccess ||
        e.hdr.alloc(c, (size_t)(total + streams + 64)) != hipSuccess)
        return fail(SMM_ERR_ALLOC, "hipMalloc of the ring streams (%lld steps) failed", (long long)total);
    ring_fill(c, h, e);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));            // nothing queued reads the old copy any more
    h->ring = std::move(e);
    return take_plan_error(c, "smm_ring_build");
}

static int check_pair(smm_ctx *c, smm_csr *a, smm_csr *b)
{
    if (!c || !a || !b) return fail(SMM_ERR_INVALID, "NULL argument");
    if (a->ctx != c || b->ctx != c) return fail(SMM_ERR_INVALID, "operand belongs to another context");
    if (a->cols != b->rows)       /* matrix_ops.py:312-313, sparse_sparse_dense.cpp:83-86 */
        return fail(SMM_ERR_INVALID, "Matrix dimensions are incompatible for multiplication (%lld x %lld times %lld x %lld)",
                    (long long)a->rows, (long long)a->cols, (long long)b->rows, (long long)b->cols);
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, a));
    CHK(validate(c, b));
    return SMM_OK;
}

extern "C" int smm_row_products(smm_ctx *c, const smm_csr *a, const smm_csr *b, int64_t *products_host)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(check_pair(c, (smm_csr *)a, (smm_csr *)b));
    if (!products_host) return fail(SMM_ERR_INVALID, "products_host is NULL");
    if (a->rows == 0) return SMM_OK;
    PoolBuf<int64_t> d(c);
    CHK(d.alloc((size_t)a->rows));
    const int grid = (int)std::min<int64_t>((a->rows + 3) / 4, 16384);
    LAUNCH(c, "smm_row_work", smm_row_work, grid, 256, 0, (int)a->rows, (int)b->cols, (int64_t)0, 0, a->ptr, a->idx,
           b->ptr, d, (int64_t *)nullptr);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(products_host, d, a->rows * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

// ------------------------------------------------------------------------------ numeric dispatch
template <int OUT, bool SYM, int NW, bool EXACT, bool SCR = false, bool L16 = false, bool SLAB = false>
static int launch_numeric_t(smm_ctx *c, NumericArgs &args)
{
    if constexpr (OUT == OUT_SPARSE && !L16) {
        if (args.list16) return launch_numeric_t<OUT, SYM, NW, EXACT, SCR, true>(c, args);
    }
    if constexpr (OUT == OUT_SPARSE && L16 && !SCR && !SLAB) {
        if (args.runs2) return launch_numeric_t<OUT, SYM, NW, EXACT, false, true, true>(c, args);
    }
    // accumulator tile (+ the exact walk's per-wave scratch behind it)
    // accumulators (+ the exact walk's per-wave scratch and the workgroup's 64-slot sink behind them)
    const size_t lds = (size_t)(((args.wc + 1) & ~1) + 2) * sizeof(double) + (EXACT ? (size_t)NW * sizeof(ExactScratch) + 64 * sizeof(double) : 0);
    auto kern = smm_numeric<OUT, SYM, NW, EXACT, SCR, L16, SLAB>;
    if (lds > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int64_t grid = (int64_t)args.m * args.nct;
    if (grid > 0x7fffffff) return fail(SMM_ERR_INVALID, "too many (row, tile) units for one launch");
    args.unit_counter = nullptr; args.n_units = (unsigned)grid;
    // Persistent workgroups where every unit is real work (CSR output, no triangle): -0.3 ms at configs[1], -0.9 ms on a
    // configs[4] share, -0.6 ms under SMM_EXACT.  Dense output measured neutral (configs[2]) and, with the trivial units
    // below the diagonal, slower (stage 1 of configs[3]: 19.2 against 18.4 ms) -- those keep one unit per workgroup
    // unless SMM_NUMERIC_PERSIST=2 (profiles/r4_numeric_persist.txt).
    const bool persist = c->numeric_persist == 2 || (c->numeric_persist == 1 && OUT == OUT_SPARSE);
    if (persist && grid > c->n_cu) {
        // as many workgroups as are resident at once (more would only find the counter spent)
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(32 / NW, (int64_t)(160 * 1024) / (int64_t)(lds + 64)));
        args.unit_counter = (unsigned *)((char *)c->d_flags + 220);
        HIPCHK(hipMemsetAsync(args.unit_counter, 0, sizeof(unsigned), c->stream));
        grid = std::min<int64_t>(grid, per_cu * c->n_cu);
    }
#ifdef SMM_STAMPS
    PoolBuf<unsigned long long> d_st(c);
    CHK(d_st.alloc(4));
    (void)hipMemsetAsync(d_st, 0, 32, c->stream);
    args.stamps = d_st;
#endif
    LAUNCH(c, SCR ? "smm_emit" : OUT == OUT_SPARSE ? "smm_numeric" : "smm_numeric_dense", kern, grid, NW * 64, lds, args);
    hipError_t e = hipGetLastError();
#ifdef SMM_STAMPS
    {
        unsigned long long h[4];
        (void)hipMemcpyAsync(h, d_st, 32, hipMemcpyDeviceToHost, c->stream);
        (void)hipStreamSynchronize(c->stream);
        const double tot = (double)(h[0] + h[1] + h[2]);
        fprintf(stderr, "[SMM_STAMPS] units=%lld NW=%d wc=%d nct=%d exact=%d  init %.1f%%  accumulate %.1f%%  epilogue %.1f%%  (sum %.3g cycles)\n",
                (long long)grid, NW, args.wc, args.nct, (int)EXACT, 100 * h[0] / tot, 100 * h[1] / tot, 100 * h[2] / tot, tot);
        d_st.reset();
    }
#endif
    if (e != hipSuccess) return fail(SMM_ERR_HIP, "smm_numeric launch: %s", hipGetErrorString(e));
    return SMM_OK;
}
template <int OUT>
static int launch_numeric(smm_ctx *c, NumericArgs &args, bool sym, int nw, bool exact)
{
    if (args.m <= 0) return SMM_OK;
    args.dummy_idx = (const int *)((const char *)c->d_flags + 64);
    args.dummy_val = (const double *)((const char *)c->d_flags + 128);
    args.err = c->d_err;
#define SMM_CASE(S, N, X) \
    if (sym == S && nw == N && exact == X) return launch_numeric_t<OUT, S, N, X>(c, args);
    SMM_CASE(false, 1, true) SMM_CASE(true, 1, true) SMM_CASE(false, 2, true) SMM_CASE(true, 2, true)
    SMM_CASE(false, 4, true) SMM_CASE(true, 4, true) SMM_CASE(false, 8, true) SMM_CASE(true, 8, true)
    SMM_CASE(false, 16, true) SMM_CASE(true, 16, true)
    SMM_CASE(false, 4, false) SMM_CASE(true, 4, false) SMM_CASE(false, 8, false) SMM_CASE(true, 8, false)
    SMM_CASE(false, 16, false) SMM_CASE(true, 16, false)
#undef SMM_CASE
    return fail(SMM_ERR_INVALID, "unsupported numeric configuration");
}

constexpr size_t LIST_SLACK = (size_t)1 << 17;      // entries behind the ordered lists (see smm_spgemm_symbolic)
#ifndef SMM_CCS_UNROLL
#define SMM_CCS_UNROLL 8        // chunk loads in flight per wave of smm_symbolic_ccs (configs[1]: 2: 6.7, 4: 5.5, 8: 5.2 ms)
#endif
// the instantiation of the chunked symbolic walk: triangle, dense runs of columns in B, units per counter round trip
using ccs_kernel_t = decltype(&smm_symbolic_ccs<false, SMM_CCS_UNROLL>);
static ccs_kernel_t ccs_kernel(bool sym, bool dr, bool batch)
{
#define CCS_K(S, D, B) smm_symbolic_ccs<S, SMM_CCS_UNROLL, D, B>
    if (batch) return dr ? (sym ? CCS_K(true, true, 16) : CCS_K(false, true, 16)) : (sym ? CCS_K(true, false, 16) : CCS_K(false, false, 16));
    return dr ? (sym ? CCS_K(true, true, 1) : CCS_K(false, true, 1)) : (sym ? CCS_K(true, false, 1) : CCS_K(false, false, 1));
#undef CCS_K
}
// ------------------------------------------------------------------------------ CSR x CSR -> CSR
struct SlabGeom { int ws, n_slabs, rw; };
constexpr int SLAB_NW = 8;                       // waves per workgroup of smm_dense_slab
struct smm_plan {
    smm_ctx *ctx = nullptr;
    smm_csr *a = nullptr, *b = nullptr;
    int flags = 0;
    int64_t row_offset = 0;
    int64_t m = 0, ncols = 0, nnz = 0;
    bool b_sorted = true;
    Geom g{};
    int64_t *d_ub_off = nullptr;   // m+1
    void *d_tmp = nullptr;         // capacity-strided ordered column lists (int32, or uint16 when list16)
    bool list16 = false;
    unsigned *d_P = nullptr;       // nnz(A)
    unsigned *d_runs = nullptr;    // nnz(A) x (nct+1)
    int2 *d_tail = nullptr;        // m: where the tail of every row starts (smm_runs)
    // column slabs (B wider than one chunked-stream slab): slab-local lists, per-(slab,row) counts, smm_runs_slab's tables
    int n_slabs = 1, tps = 0, ws = 0;
    int *d_scnt = nullptr;         // n_slabs x m
    unsigned *d_dst0 = nullptr;    // nnz(A)
    uint2 *d_runs2 = nullptr;      // nct x nnz(A)
    unsigned char *d_tflag = nullptr;   // nct x m: which (tile, row) units hold entries of C
    const int *seg = nullptr;      // B's tile index and tile-local columns for geometry g (owned by b)
    const short *loc = nullptr;
    smm_csr::PackView pack{0, 0, nullptr, nullptr, 0, 0}; // default mode: packed payload of B for geometry g
    bool use_slab = false;         // dense-bin rows: smm_dense_slab -> scratch -> emission, instead of the tile kernel
    SlabGeom sg{};
    smm_csr::SlabView slab{0, 0, nullptr, nullptr, nullptr};
    int *d_rowcnt = nullptr;       // m
    int64_t total_cap = 0;         // sum of the list capacities (= d_ub_off's last entry)
    int *d_lists = nullptr;        // 5 x m: rows of the small / medium / dense / tiny (16) / tiny (32) bins
    int n_bin[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t *d_cptr = nullptr;     // m+1
};

extern "C" void smm_plan_destroy(smm_plan *p)
{
    if (!p) return;
    smm_ctx *c = p->ctx;
    CTX_LOCK(c);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    pool_free(c, p->d_ub_off); pool_free(c, p->d_tmp); pool_free(c, p->d_P); pool_free(c, p->d_runs);
    pool_free(c, p->d_rowcnt); pool_free(c, p->d_cptr); pool_free(c, p->d_lists); pool_free(c, p->d_tail);
    pool_free(c, p->d_scnt); pool_free(c, p->d_dst0); pool_free(c, p->d_runs2); pool_free(c, p->d_tflag);
    delete p;
}
using PlanPtr = std::unique_ptr<smm_plan, Destroyer<smm_plan_destroy>>;
extern "C" int64_t smm_plan_nnz(const smm_plan *p) { return p ? p->nnz : -1; }
extern "C" int64_t smm_plan_device_bytes(const smm_plan *p)
{
    if (!p) return -1;
    smm_ctx *c = p->ctx;
    CTX_LOCK(c);
    int64_t total = 0;
    const void *blocks[] = {p->d_ub_off, p->d_tmp, p->d_P, p->d_runs, p->d_rowcnt, p->d_cptr, p->d_lists, p->d_tail,
                            p->d_scnt, p->d_dst0, p->d_runs2, p->d_tflag};
    for (const void *b : blocks) {
        auto it = c->live.find((void *)b);
        if (b && it != c->live.end()) total += (int64_t)it->second;
    }
    return total;
}

// exclusive scan of n values into out[0..n] (out[n] = total)
template <typename T>
static int scan_launch(smm_ctx *c, int64_t n, const T *in, int64_t *out)
{
    if (n <= 8 * SCAN_TILE) {
        LAUNCH(c, "smm_scan", smm_scan<T>, 1, 1024, 0, (int)n, in, out);
        LAUNCH_CHECK();
        return SMM_OK;
    }
    const int tiles = (int)((n + SCAN_TILE - 1) / SCAN_TILE);
    PoolBuf<int64_t> sums(c);
    CHK(sums.alloc((size_t)2 * tiles + 1));
    LAUNCH(c, "smm_scan", smm_scan_tile_sums<T>, tiles, 1024, 0, (int)n, in, sums);
    LAUNCH(c, "smm_scan", smm_scan<int64_t>, 1, 1024, 0, tiles, (const int64_t *)sums, sums + tiles);
    LAUNCH(c, "smm_scan", smm_scan_tiles<T>, tiles, 1024, 0, (int)n, in, (const int64_t *)(sums + tiles), out);
    LAUNCH_CHECK();
    return SMM_OK;
}

// Packed tile-major payload of B for the shared-tile walk (smm_pack_* / smm_pack12_* in smm_kernels.hpp), cached per
// (geometry, format).
// pack_fill: the payload of e from b's current values (pack12: +0.0 into the mid-piece pads as well); queued, not checked.
// which: an entry that holds its pieces both back to back and strided re-fills both on a value update, a build fills its own.
enum { FILL_COMPACT = 1, FILL_STRIDED = 2, FILL_ALL = 3 };
static void pack_fill(smm_ctx *c, const smm_csr *b, const smm_csr::PackCache &e, int which = FILL_ALL)
{
    const int64_t cells = (int64_t)e.nct * b->rows;
    if (cells <= 0) return;
    if (e.fmt == PACK_FMT_12 && e.spay && (which & FILL_STRIDED))
        LAUNCH(c, "smm_pack12_fill", smm_pack12_fill, std::min<int64_t>((cells + 3) / 4, 65536), 256, 0, (int)b->rows, e.nct, e.wc, b->idx, b->val, e.seg,
               (const int2 *)nullptr, e.spay.p, e.stride, (const unsigned short *)e.len16);
    if (!e.pay || !(which & FILL_COMPACT)) return;
    if (e.fmt == PACK_FMT_12)
        LAUNCH(c, "smm_pack12_fill", smm_pack12_fill, std::min<int64_t>((cells + 3) / 4, 65536), 256, 0, (int)b->rows, e.nct, e.wc, b->idx, b->val, e.seg,
               (const int2 *)e.desc, e.pay.p, 0, (const unsigned short *)nullptr);
    else
        LAUNCH(c, "smm_pack_fill", smm_pack_fill, std::min<int64_t>((b->rows + 3) / 4, 65536), 256, 0, (int)b->rows, e.nct, e.wc, b->ptr,
               b->idx, b->val, e.seg, (const int2 *)e.desc, e.pay.p);
}
// The pack12 rule: the walk that reads it runs four entries per lane (longest n in (128, 256]) and, unless forced
// (mode 2), the operand is smaller that way.
static bool pack12_chosen(const smm_ctx *c, const smm_csr::PackCache &e)
{
    if (c->pack12 == 0 || !c->piece_walk || e.maxlen <= 128 || e.maxlen > 256) return false;
    return c->pack12 == 2 || e.units12 < e.units16;
}
// The stride rule: pack12 is chosen, the strided payload (the longest piece's units for every piece) stays below 2^31
// units and, unless forced (mode 2), it is at most 1.5 times the compact one -- a condition on capacity, not a tuned
// number: one very long row must not multiply the operand's footprint.
static int64_t stride_units(const smm_csr::PackCache &e, int64_t rows) { return (int64_t)pack12_units(e.maxlen) * rows * e.nct; }
static bool stride_chosen(const smm_ctx *c, const smm_csr::PackCache &e, int64_t rows)
{
    if (c->pack_stride == 0 || !pack12_chosen(c, e)) return false;
    const int64_t total = stride_units(e, rows);
    if (total + PACK12_STRIDE_SLACK >= INT32_MAX) return false;
    return c->pack_stride == 2 || 2 * total <= 3 * e.units12;
}
// Count b's pieces as pack12 into e (a new entry, or one that lacks the arrays the rules choose now) and build them.
static int pack12_prepare(smm_ctx *c, smm_csr *b, smm_csr::PackCache &e)
{
    const int64_t cells = (int64_t)e.nct * b->rows;
    if (cells + 1 >= INT32_MAX) return fail(SMM_ERR_INVALID, "too many (tile, row) pieces");
    PoolBuf<int> units(c), n12(c);
    PoolBuf<int64_t> off64(c);
    PoolBuf<unsigned long long> d_stat(c);
    CHK(units.alloc((size_t)std::max<int64_t>(cells, 1)));
    CHK(n12.alloc((size_t)std::max<int64_t>(cells, 1)));
    CHK(off64.alloc((size_t)cells + 1));
    CHK(d_stat.alloc(4));
    HIPCHK(hipMemsetAsync(d_stat, 0, 4 * sizeof(unsigned long long), c->stream));
    if (cells > 0)
        LAUNCH(c, "smm_pack12_count", smm_pack12_count, (cells + 255) / 256, 256, 0, (int)b->rows, e.nct, e.wc, b->idx, e.seg, units.p, n12.p, d_stat.p);
    LAUNCH_CHECK();
    unsigned long long stat[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(stat, d_stat, sizeof(stat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    e.maxlen = (int)stat[0]; e.units16 = (int64_t)stat[1]; e.units12 = (int64_t)stat[2];
    if (stride_chosen(c, e, b->rows)) {
        if (!e.spay) {
            e.stride = pack12_units(e.maxlen);
            if (e.len16.alloc(c, (size_t)std::max<int64_t>(cells, 1)) != hipSuccess || e.spay.alloc(c, (size_t)(stride_units(e, b->rows) + PACK12_STRIDE_SLACK)) != hipSuccess) {
                e.len16.reset(); e.spay.reset();
                return fail(SMM_ERR_ALLOC, "hipMalloc of the packed payload failed");
            }
            LAUNCH(c, "smm_pack12_len16", smm_pack12_len16, (cells + 255) / 256, 256, 0, cells, (const int *)n12, e.len16.p);
            pack_fill(c, b, e, FILL_STRIDED);
            LAUNCH_CHECK();
        }
    } else if (pack12_chosen(c, e) && !e.pay) {
        if (e.units12 >= INT32_MAX) return fail(SMM_ERR_INVALID, "operand too large for the packed payload");
        CHK(scan_launch<int>(c, cells, units, off64));
        // (+ 4 units of slack, as for the 16-bit payload)
        if (e.desc.alloc(c, (size_t)std::max<int64_t>(cells, 1)) != hipSuccess || e.pay.alloc(c, (size_t)(std::max<int64_t>(e.units12, 1) + 4)) != hipSuccess)
            return fail(SMM_ERR_ALLOC, "hipMalloc of the packed payload failed");
        LAUNCH(c, "smm_pack12_desc", smm_pack12_desc, (cells + 255) / 256, 256, 0, cells, (const int64_t *)off64, (const int *)n12, e.desc.p);
        pack_fill(c, b, e, FILL_COMPACT);
        LAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(c->stream));            // units / n12 / off64 go back to the pool
    units.reset(); n12.reset(); off64.reset(); d_stat.reset();
    return SMM_OK;
}
// fmt: what the caller's walk can read -- PACK_FMT_12 asks for pack12 where the rule chooses it and gets the 16-bit
// payload otherwise (out->fmt says which).
// (descriptors are handed out BY VALUE: a plan must not point into the operand's vector, which may grow)
static int ensure_pack(smm_ctx *c, smm_csr *b, const Geom &g, int fmt, smm_csr::PackView *out)
{
    if (g.wc > 32767) return fail(SMM_ERR_INVALID, "coarse tile wider than 32767 columns");
    if (fmt == PACK_FMT_12 && c->pack12 != 0 && c->piece_walk) {
        size_t at = b->packs.size();
        for (size_t i = 0; i < b->packs.size(); ++i)
            if (b->packs[i].wc == g.wc && b->packs[i].nct == g.nct && b->packs[i].fmt == PACK_FMT_12) at = i;
        if (at == b->packs.size()) {
            smm_csr::PackCache e{g.wc, g.nct, nullptr, {}, {}, 0, PACK_FMT_12, 0, 0};
            CHK(ensure_seg(c, b, tiles_geom(g.nct, g.wc), &e.seg));
            CHK(pack12_prepare(c, b, e));
            b->packs.push_back(std::move(e));
        } else if (pack12_chosen(c, b->packs[at]) && (stride_chosen(c, b->packs[at], b->rows) ? !b->packs[at].spay : !b->packs[at].pay)) {
            CHK(pack12_prepare(c, b, b->packs[at]));       // (judged under another SMM_PACK12 / SMM_PACK_STRIDE mode before)
        }
        if (pack12_chosen(c, b->packs[at])) {
            const bool strided = stride_chosen(c, b->packs[at], b->rows);
            if (strided ? (bool)b->packs[at].spay : (bool)b->packs[at].pay) { *out = b->packs[at].view(strided); return SMM_OK; }
        }
    }
    for (auto &e : b->packs)
        if (e.wc == g.wc && e.nct == g.nct && e.fmt == PACK_FMT_16) { *out = e.view(); return SMM_OK; }
    smm_csr::PackCache e{g.wc, g.nct, nullptr, {}, {}, 0, PACK_FMT_16, 0, 0};
    CHK(ensure_seg(c, b, tiles_geom(g.nct, g.wc), &e.seg));   // the coarse-tile index (shared walk: one entry per coarse tile)
    const int64_t cells = (int64_t)g.nct * b->rows;
    if (cells + 1 >= INT32_MAX) return fail(SMM_ERR_INVALID, "too many (tile, row) pieces");
    PoolBuf<int> units(c);
    PoolBuf<int64_t> off64(c);
    CHK(units.alloc((size_t)std::max<int64_t>(cells, 1)));
    CHK(off64.alloc((size_t)cells + 1));
    int *d_maxlen = (int *)((char *)c->d_flags + 244);
    (void)hipMemsetAsync(d_maxlen, 0, sizeof(int), c->stream);
    if (cells > 0) LAUNCH(c, "smm_pack_count", smm_pack_count, (cells + 255) / 256, 256, 0, (int)b->rows, g.nct, e.seg, units, d_maxlen);
    CHK(scan_launch<int>(c, cells, units, off64));
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, off64 + cells, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&e.maxlen, d_maxlen, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total >= INT32_MAX) return fail(SMM_ERR_INVALID, "operand too large for the packed payload");
    e.units16 = total;
    // (+ 4 units of slack: the piece walk's last lane reads up to three 8-byte units past a very short last piece)
    if (e.desc.alloc(c, (size_t)std::max<int64_t>(cells, 1)) != hipSuccess || e.pay.alloc(c, (size_t)(std::max<int64_t>(total, 1) + 4)) != hipSuccess)
        return fail(SMM_ERR_ALLOC, "hipMalloc of the packed payload failed");
    if (cells > 0) {
        LAUNCH(c, "smm_pack_desc", smm_pack_desc, (cells + 255) / 256, 256, 0, (int)b->rows, g.nct, e.seg, (const int64_t *)off64, e.desc.p);
        pack_fill(c, b, e);
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(c->stream));        // units / off64 go back to the pool
    }
    units.reset(); off64.reset();
    *out = e.view();
    b->packs.push_back(std::move(e));
    return SMM_OK;
}

// Chunk-padded 16-bit column stream of B for the symbolic walk (smm_ccs_* / smm_symbolic_ccs), cached per slab
// geometry.  (Handed out BY VALUE, like the packed payload: the operand's vector may grow.)
static int ensure_ccs(smm_ctx *c, smm_csr *b, int ws, int n_slabs, smm_csr::CcsView *out)
{
    for (auto &e : b->ccs)
        if (e.ws == ws && e.n_slabs == n_slabs) { *out = e.view(); return SMM_OK; }
    if (ws > CCS_MAX_WS) return fail(SMM_ERR_INVALID, "column slab wider than %d columns", CCS_MAX_WS);
    const int *seg = nullptr;
    CHK(ensure_seg(c, b, tiles_geom(n_slabs, ws), &seg));
    const int64_t cells = (int64_t)n_slabs * b->rows;
    if (cells + n_slabs + 1 >= INT32_MAX) return fail(SMM_ERR_INVALID, "too many (slab, row) pieces");
    PoolBuf<int> chunks(c);
    PoolBuf<int64_t> off64(c);
    CHK(chunks.alloc((size_t)std::max<int64_t>(cells, 1)));
    CHK(off64.alloc((size_t)cells + 1));
    if (cells > 0) LAUNCH(c, "smm_ccs_count", smm_ccs_count, (cells + 255) / 256, 256, 0, (int)b->rows, n_slabs, seg, chunks);
    CHK(scan_launch<int>(c, cells, chunks, off64));
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, off64 + cells, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total + 1 >= (INT32_MAX / CCS_CHUNK)) return fail(SMM_ERR_INVALID, "operand too large for the chunked column stream");
    PoolBuf<unsigned long long> d_stat(c);
    CHK(d_stat.alloc(2));
    HIPCHK(hipMemsetAsync(d_stat, 0, 2 * sizeof(unsigned long long), c->stream));
    const int64_t ptr_entries = (int64_t)n_slabs * (b->rows + 1);
    DevBuf<int> cptr; DevBuf<unsigned short> stream;
    if (cptr.alloc(c, (size_t)ptr_entries) != hipSuccess || stream.alloc(c, (size_t)(total + 1) * CCS_CHUNK) != hipSuccess)
        return fail(SMM_ERR_ALLOC, "hipMalloc of the chunked column stream failed");
    const int bm_words = (ws + 31) / 32;
    LAUNCH(c, "smm_ccs_ptr", smm_ccs_ptr, (ptr_entries + 255) / 256, 256, 0, (int)b->rows, n_slabs, (const int64_t *)off64, cptr);
    LAUNCH(c, "smm_ccs_fill", smm_ccs_fill, std::min<int64_t>(std::max<int64_t>((cells + 3) / 4, 1), 65536), 256, 0, (int)b->rows, n_slabs, ws,
           bm_words, b->idx, seg, (const int *)cptr, stream, d_stat);
    LAUNCH_CHECK();
    unsigned long long stat[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(stat, d_stat, sizeof(stat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));        // chunks / off64 go back to the pool
    chunks.reset(); off64.reset(); d_stat.reset();
    b->ccs.push_back({ws, n_slabs, bm_words, (int)total, std::move(cptr), std::move(stream), stat[1] ? (double)stat[0] / (double)stat[1] : 0.0});
    *out = b->ccs.back().view();
    return SMM_OK;
}

// ------------------------------------------------------------------------------ row block x column slab path

// Slab width: the slab's share of B's payload (10 bytes per entry) should sit in one XCD's 4 MiB L2 next
// to the streams that pass through it, and R rows of it must fit the LDS.  Returns false when the
// slab kernels cannot run for this operand.
static bool slab_geometry(const smm_ctx *c, const smm_csr *b, int64_t ncols, SlabGeom *g)
{
    if ((b->vflags & CSR_UNSORTED) || ncols <= 0 || b->nnz <= 0) return false;
    const int rw = c->slab_rw;
    const int R = SLAB_NW * rw;
    const int64_t lds_doubles = ((int64_t)160 * 1024 - (int64_t)SLAB_NW * (int64_t)sizeof(SlabScratch) - (int64_t)sizeof(SlabShared)) / 8;
    int64_t ws_lds = (lds_doubles / R) & ~(int64_t)1;
    int64_t ws = c->slab_ws;
    if (ws <= 0) {
        const double l2_bytes = 3.0e6;
        ws = (int64_t)(l2_bytes * (double)ncols / (10.0 * (double)b->nnz));
        if (ws < 64) ws = 64;
    }
    ws = std::min<int64_t>(std::min<int64_t>(ws, ws_lds), std::min<int64_t>(ncols, 32766));
    if (ws < 1) return false;
    int64_t ns = (ncols + ws - 1) / ws;
    if (ns >= 8 && c->slab_ws <= 0) ns = (ns + 7) & ~(int64_t)7;       // whole slabs per XCD
    ws = (ncols + ns - 1) / ns;
    ws = (ws + 1) & ~(int64_t)1;
    if (ws > ws_lds) ws = ws_lds;
    ns = (ncols + ws - 1) / ws;
    if (ns * b->rows + 1 >= INT32_MAX) return false;
    g->ws = (int)ws; g->n_slabs = (int)ns; g->rw = rw;
    return true;
}

// The columns and values of e from b's current arrays; queued, not checked.
static void slab_fill(smm_ctx *c, const smm_csr *b, const smm_csr::SlabCache &e)
{
    if (b->rows > 0)
        LAUNCH(c, "smm_slab_fill", smm_slab_fill, std::min<int64_t>((b->rows + 3) / 4, 65536), 256, 0, (int)b->rows, e.n_slabs, e.ws,
               b->ptr, b->idx, b->val, e.seg, (const int *)e.soff, e.scol.p, e.sval.p);
}
static int ensure_slab(smm_ctx *c, smm_csr *b, const SlabGeom &g, smm_csr::SlabView *out)
{
    for (auto &e : b->slabs)
        if (e.ws == g.ws && e.n_slabs == g.n_slabs) { *out = e.view(); return SMM_OK; }
    smm_csr::SlabCache e{g.ws, g.n_slabs, nullptr, {}, {}, {}};
    CHK(ensure_seg(c, b, tiles_geom(g.n_slabs, g.ws), &e.seg));
    const int64_t cells = (int64_t)g.n_slabs * b->rows;
    PoolBuf<int> cnt(c);
    PoolBuf<int64_t> off64(c);
    CHK(cnt.alloc((size_t)std::max<int64_t>(cells, 1)));
    CHK(off64.alloc((size_t)cells + 1));
    if (e.soff.alloc(c, (size_t)(cells + 1)) != hipSuccess || e.scol.alloc(c, (size_t)std::max<int64_t>(b->nnz, 1)) != hipSuccess ||
        e.sval.alloc(c, (size_t)std::max<int64_t>(b->nnz, 1)) != hipSuccess)
        return fail(SMM_ERR_ALLOC, "hipMalloc of the slab-major copy of B failed");
    if (cells > 0) LAUNCH(c, "smm_slab_count", smm_slab_count, (cells + 255) / 256, 256, 0, (int)b->rows, g.n_slabs, e.seg, cnt);
    CHK(scan_launch<int>(c, cells, cnt, off64));
    LAUNCH(c, "smm_narrow32", smm_narrow32, std::min<int64_t>((cells + 256) / 256, 65536), 256, 0, cells + 1, (const int64_t *)off64, e.soff.p);
    slab_fill(c, b, e);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));        // cnt / off64 go back to the pool
    cnt.reset(); off64.reset();
    *out = e.view();
    b->slabs.push_back(std::move(e));
    return SMM_OK;
}

// ------------------------------------------------------------------------------ values-only update
// New values on an unchanged pattern: the operand's value array is overwritten in place and every cached
// copy that carries values is re-filled in place by the kernel that built it (same pattern -> same
// positions), so the pointers plans hold stay valid.  Everything is queued on the context's stream, behind
// whatever product is still running there.
static int refresh_value_copies(smm_ctx *c, smm_csr *m)
{
    m->trv.reset();                                     // (rebuilt by the next product that needs it)
    for (auto &e : m->packs) pack_fill(c, m, e);
    for (auto &e : m->slabs) slab_fill(c, m, e);
    if (m->ring.val) ring_fill(c, m, m->ring);
    if (m->ell.val) ell_fill(c, m, m->ell);
    LAUNCH_CHECK();
    return SMM_OK;
}

extern "C" int smm_csr_update_values(smm_ctx *c, smm_csr *m, const double *data)
{
    if (!c || !m) return fail(SMM_ERR_INVALID, "NULL argument");
    if (m->ctx != c) return fail(SMM_ERR_INVALID, "operand belongs to another context");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    if (!m->owned()) return fail(SMM_ERR_INVALID, "smm_csr_update_values: the operand borrows its arrays (smm_csr_from_device); "
                                                "rewrite them and call smm_csr_update_values_device");
    if (m->nnz == 0) return SMM_OK;
    if (!data) return fail(SMM_ERR_INVALID, "data is NULL");
    HIPCHK(hipMemcpyAsync((void *)m->val, data, (size_t)m->nnz * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));          // the caller's host array may change as soon as this returns
    return refresh_value_copies(c, m);
}

extern "C" int smm_csr_update_values_device(smm_ctx *c, smm_csr *m, const double *d_data)
{
    if (!c || !m) return fail(SMM_ERR_INVALID, "NULL argument");
    if (m->ctx != c) return fail(SMM_ERR_INVALID, "operand belongs to another context");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    if (m->nnz == 0) return SMM_OK;
    if (d_data && d_data != m->val) {
        if (!m->owned()) return fail(SMM_ERR_INVALID, "smm_csr_update_values_device: a borrowed operand is updated by rewriting its "
                                                    "own array (pass NULL or that array)");
        HIPCHK(hipMemcpyAsync((void *)m->val, d_data, (size_t)m->nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    return refresh_value_copies(c, m);
}

// rows (a row list, or rows 0..m-1 of A) x all slabs -> `out`, rows of the launch ldo apart, column order
template <bool NEGZERO>
static int launch_slab(smm_ctx *c, const smm_csr *a, const smm_csr *b, const smm_csr::SlabView &sl, int rw, int m,
                       const int *rowlist, bool sym, int64_t row_offset, double *out, int64_t ldo)
{
    if (m <= 0) return SMM_OK;
    SlabArgs S{};
    const int R = SLAB_NW * rw;
    S.m = m; S.ncols = (int)b->cols; S.ws = sl.ws; S.n_slabs = sl.n_slabs; S.n_rb = (m + R - 1) / R; S.rowsB = (int)b->rows;
    S.row_offset = row_offset; S.rowlist = rowlist;
    S.kmax = (int)std::max<int64_t>(b->nnz - 1, 0);
    S.a_ptr = a->ptr; S.a_idx = a->idx; S.a_val = a->val;
    S.soff = sl.soff; S.scol = sl.scol; S.sval = sl.sval;
    S.dummy_idx = (const int *)((const char *)c->d_flags + 64);
    S.dummy_val = (const double *)((const char *)c->d_flags + 128);
    S.out = out; S.ldo = ldo;
    const int64_t units = (int64_t)S.n_rb * S.n_slabs;
    S.cpx = (int)((units + 7) / 8);
    const int64_t grid = (int64_t)S.cpx * 8;
    if (grid > 0x7fffffff) return fail(SMM_ERR_INVALID, "too many (row block, slab) units for one launch");
    const size_t lds = (size_t)R * ((sl.ws + 1) & ~1) * sizeof(double) + (size_t)SLAB_NW * sizeof(SlabScratch) + sizeof(SlabShared);
#define SLAB_CASE(S_, RW_)                                                                                       \
    if (sym == S_ && rw == RW_) {                                                                                \
        auto kern = smm_dense_slab<S_, SLAB_NW, RW_, NEGZERO>;                                                   \
        if (lds > 64 * 1024)                                                                                     \
            HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        LAUNCH(c, "smm_dense_slab", kern, grid, SLAB_NW * 64, lds, S);                                           \
        LAUNCH_CHECK();                                                                                          \
        return SMM_OK;                                                                                           \
    }
    SLAB_CASE(false, 2) SLAB_CASE(true, 2) SLAB_CASE(false, 4) SLAB_CASE(true, 4)
#undef SLAB_CASE
    return fail(SMM_ERR_INVALID, "unsupported slab configuration");
}

// Does the slab path pay?  It moves A's metadata once per slab and, for CSR output, the dense scratch
// twice; the tile kernel moves 10 bytes per product through the fabric.  `cells` = rows x columns of the
// launch, `products` their multiply-adds (an estimate is enough), `nnz_c` < 0 for dense output.
static bool slab_pays(const smm_ctx *c, const smm_csr *a, const SlabGeom &g, double cells, double products, double nnz_c,
                      double b_nnz_per_row, double ncols)
{
    if (c->slab_mode == 1) return false;
    if (c->slab_mode == 2) return true;
    if (cells <= 0) return false;
    // Measured (profiles/r2_c_slab_sweep.txt): with pieces of B's rows of 6-13 entries (50k x 50k, d = 0.01,
    // slabs of 570-1100 columns) the kernel is bound by the L1's line look-ups -- every piece is its own
    // 128-byte line, ~26 look-ups per 64-lane chunk against ~5 for the tile kernel -- and loses 1.4-1.8x.
    // It is therefore chosen only where a slab-sized piece of a row of B is long.
    const double piece = (double)b_nnz_per_row * g.ws / std::max<double>(1.0, ncols);
    if (piece < 24.0) return false;
    const double tile_bytes = 10.0 * products;
    double slab_bytes = 12.0 * (double)a->nnz * g.n_slabs + 8.0 * (double)a->nnz * g.n_slabs   /* A and soff per slab */
                        + 2.5 * products;                                                          /* ~3/4 of the gather hits L2 */
    if (nnz_c >= 0) slab_bytes += 16.0 * cells;                                                    /* scratch out and back */
    return slab_bytes < 0.7 * tile_bytes && products > 1e7;
}

template <bool SYM, bool SAFE, int MARK, int UNROLL, bool I16>
static int launch_symbolic_w(smm_ctx *c, smm_plan *p, int words, unsigned *gbm, int grid, int wpb, const int *rowlist,
                             const int *d_nrows, int *d_row_counter, int rbatch);
template <bool SYM, bool SAFE, int MARK, int UNROLL = 16>
static int launch_symbolic_t(smm_ctx *c, smm_plan *p, int words, unsigned *gbm, int grid, int wpb, const int *rowlist,
                             const int *d_nrows, int *d_row_counter, int rbatch = 1)
{
    return p->list16 ? launch_symbolic_w<SYM, SAFE, MARK, UNROLL, true>(c, p, words, gbm, grid, wpb, rowlist, d_nrows, d_row_counter, rbatch)
                     : launch_symbolic_w<SYM, SAFE, MARK, UNROLL, false>(c, p, words, gbm, grid, wpb, rowlist, d_nrows, d_row_counter, rbatch);
}
template <bool SYM, bool SAFE, int MARK, int UNROLL, bool I16>
static int launch_symbolic_w(smm_ctx *c, smm_plan *p, int words, unsigned *gbm, int grid, int wpb, const int *rowlist,
                             const int *d_nrows, int *d_row_counter, int rbatch)
{
    // LDS per wave: bitmap words + the guard word, or the hash slots
    const size_t lds = MARK == MARK_GLOBAL_BITMAP ? 0 : (size_t)(words + (MARK == MARK_LDS_HASH ? 0 : 1)) * wpb * sizeof(unsigned);
    auto kern = smm_symbolic<SYM, SAFE, MARK, UNROLL, I16>;
    const int *b_idx32 = p->b->idx;
#ifndef SMM_SYMW_UNROLL
#define SMM_SYMW_UNROLL 4
#endif
#ifndef SMM_SYMW_DEEP
#define SMM_SYMW_DEEP 16
#endif
    if constexpr (!SAFE && MARK != MARK_LDS_HASH) {
        // chunks of 128 entries, two columns per lane (16-bit columns: the idle column must fit 16 bits)
        // The pair of an odd chunk's last entry reaches one column past the row: the 16-bit copy and the 32-bit
        // arrays this library allocates have slack for that, a borrowed 32-bit array is read through a padded copy.
        if (c->sym_wide && (!I16 || words * 32 + 31 <= 65535)) {
            kern = smm_symbolic<SYM, false, MARK, (UNROLL == 16 ? SMM_SYMW_UNROLL : SMM_SYMW_DEEP), I16, true>;
            if (!I16) CHK(idx_with_slack(c, p->b, &b_idx32));
        }
    }
    if (lds > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    LAUNCH(c, MARK == MARK_LDS_HASH ? "smm_symbolic_hash" : "smm_symbolic", kern, grid, wpb * 64, lds, (int)p->m, rowlist,
           d_nrows, p->row_offset, words, p->a->ptr, p->a->idx, p->b->ptr,
           I16 ? (const void *)p->b->idx16.p : (const void *)b_idx32, p->d_ub_off, p->d_tmp, p->d_P,
           p->d_rowcnt, gbm, d_row_counter, rbatch);
    LAUNCH_CHECK();
    return SMM_OK;
}

// The plan checker (smm_plan_check_* in smm_kernels.hpp): every invariant the numeric phase relies on, verified on the
// device; violations come back as SMM_ERR_INTERNAL through the context's error word.
static int plan_check(smm_ctx *c, smm_plan *p)
{
    const int64_t m = p->m;
    if (m == 0 || !p->d_ub_off || !p->d_rowcnt) return take_plan_error(c, "smm_plan_check");      // zero operand: nothing was planned
    const smm_csr *a = p->a;
    const int grid = (int)std::min<int64_t>((m + 3) / 4, 16384);
    const bool slabs = p->d_scnt != nullptr;
    const int ns = slabs ? p->n_slabs : 1;
    const int *cnt = slabs ? p->d_scnt : p->d_rowcnt;
    if (p->list16)
        LAUNCH(c, "smm_plan_check", smm_plan_check_rows<unsigned short>, grid, 256, 0, (int)m, ns, slabs ? p->ws : (int)p->ncols, (int)p->ncols,
               (int64_t)a->nnz, p->total_cap, a->ptr, (const int64_t *)p->d_ub_off, cnt, (const int *)p->d_rowcnt, (const int64_t *)p->d_cptr,
               (const unsigned *)p->d_P, (const unsigned short *)p->d_tmp, c->d_err);
    else
        LAUNCH(c, "smm_plan_check", smm_plan_check_rows<int>, grid, 256, 0, (int)m, ns, (int)p->ncols, (int)p->ncols,
               (int64_t)a->nnz, p->total_cap, a->ptr, (const int64_t *)p->d_ub_off, cnt, (const int *)p->d_rowcnt, (const int64_t *)p->d_cptr,
               (const unsigned *)p->d_P, (const int *)p->d_tmp, c->d_err);
    LAUNCH_CHECK();
    CHK(take_plan_error(c, "smm_plan_check"));          // the table checks below walk the lists through what was just verified
    const int nd = p->n_bin[2];
    if (nd > 0 && p->d_lists) {
        const int *rows = p->d_lists + 2 * m;
        const int rgrid = (int)std::min<int64_t>((nd + 3) / 4, 16384);
        if (p->d_runs2)
            LAUNCH(c, "smm_plan_check", smm_plan_check_runs2, rgrid, 256, 0, nd, (int)m, p->n_slabs, p->tps, p->g.nct, p->g.wc, (int64_t)a->nnz, rows,
                   a->ptr, (const int64_t *)p->d_ub_off, (const int *)p->d_scnt, (const int64_t *)p->d_cptr, (const unsigned *)p->d_P,
                   (const unsigned short *)p->d_tmp, (const uint2 *)p->d_runs2, c->d_err);
        else if (p->d_runs && p->list16)
            LAUNCH(c, "smm_plan_check", smm_plan_check_runs<unsigned short>, rgrid, 256, 0, nd, p->g.nct, p->g.wc, rows, a->ptr,
                   (const int64_t *)p->d_ub_off, (const int *)p->d_rowcnt, (const unsigned *)p->d_P, (const unsigned short *)p->d_tmp,
                   (const unsigned *)p->d_runs, (const int2 *)p->d_tail, c->d_err);
        else if (p->d_runs)
            LAUNCH(c, "smm_plan_check", smm_plan_check_runs<int>, rgrid, 256, 0, nd, p->g.nct, p->g.wc, rows, a->ptr,
                   (const int64_t *)p->d_ub_off, (const int *)p->d_rowcnt, (const unsigned *)p->d_P, (const int *)p->d_tmp,
                   (const unsigned *)p->d_runs, (const int2 *)p->d_tail, c->d_err);
        LAUNCH_CHECK();
    }
    if (p->pack.stride > 0 && p->pack.len16 && p->b) {
        const int64_t cells = (int64_t)p->pack.nct * p->b->rows;
        if (cells > 0)
            LAUNCH(c, "smm_plan_check", smm_plan_check_len16, (int)std::min<int64_t>((cells + 255) / 256, 16384), 256, 0, cells, p->pack.maxlen,
                   (const unsigned short *)p->pack.len16, c->d_err);
        LAUNCH_CHECK();
    }
    return take_plan_error(c, "smm_plan_check");
}

extern "C" int smm_plan_check(smm_ctx *c, smm_plan *p)
{
    if (!c || !p || p->ctx != c) return fail(SMM_ERR_INVALID, "bad plan/context");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    return plan_check(c, p);
}

// Test hook: damage one piece of the plan's metadata on the device (kinds: smm_plan_corrupt in smm_kernels.hpp).
extern "C" int smm_plan_inject_fault(smm_ctx *c, smm_plan *p, int kind)
{
    if (!c || !p || p->ctx != c) return fail(SMM_ERR_INVALID, "bad plan/context");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    if (kind < 1 || kind > 8) return fail(SMM_ERR_INVALID, "fault kind must be in [1,8]");
    if (p->nnz == 0 || !p->d_lists) return fail(SMM_ERR_INVALID, "fault injection needs a plan with a non-empty result");
    if ((kind <= 3 && !p->d_runs) || (kind == 6 && !p->d_runs2)) return fail(SMM_ERR_INVALID, "this plan has no such table");
    // the first row of the tile bin (the tables exist for those rows only), else of the medium / small hash bin
    const int bin = p->n_bin[2] > 0 ? 2 : (p->n_bin[1] > 0 ? 1 : 0);
    if (p->n_bin[bin] == 0 || (bin != 2 && (kind <= 3 || kind == 6))) return fail(SMM_ERR_INVALID, "no row to damage for this fault kind");
    int row = 0;
    HIPCHK(hipMemcpyAsync(&row, p->d_lists + (size_t)bin * p->m, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hipLaunchKernelGGL(smm_plan_corrupt, dim3(1), dim3(64), 0, c->stream, kind, row, p->g.nct, (int64_t)p->a->nnz, p->a->ptr, p->d_ub_off,
                       p->d_rowcnt, p->d_P, p->d_tmp, p->list16 ? 1 : 0, p->d_runs, p->d_tail, p->d_runs2);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

// ------------------------------------------------------------------------------ symbolic phase
// The marker of the symbolic phase is a bitmap of B's columns (ncols/8 bytes per wave, in LDS when it fits): at 50 000
// columns 24 waves fit a CU, at 1e6 columns one.  Rows with few products -- known after the row work -- therefore take an
// LDS hash set instead, wherever that is the smaller marker:
//   four classes: <= 256 / 512 / 1024 / 2048 products in 512 / 1024 / 2048 / 4096 slots (2 ... 16 KB per wave; round 4:
//   there used to be two, and a band of half-width 8 -- 289 products, 33 columns per row -- ran 8 waves per CU in the
//   4096-slot class: 11.6 ms; in the 1024-slot class 4.9 ms).
// ... and TINY rows (<= 16 products from <= 16 entries of A, whatever B looks like) go four to a wave (smm_symbolic_tiny)
constexpr int NHC = 4;
constexpr int HS[NHC] = {512, 1024, 2048, 4096};
constexpr int SB_REST = NHC, SB_TINY = NHC + 1, SB_TINY2 = NHC + 2, SB_N = NHC + 3;      // bins of the symbolic phase: hash classes, bitmap, tiny (16 / 32 lanes per row)

// What the row work leaves for the walks.
struct SymRows {
    PoolBuf<int64_t> prod;       // products per row (the numeric binning at the end applies the same tiny-row predicate)
    PoolBuf<int> slists;         // SB_N x m: the rows of each bin (binned only)
    int sbin[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int hmax1 = 0;               // most products of a row in a hash class (0: no hash classes)
    bool binned = false;
    bool safe = false;           // B has unsorted rows or repeated columns
    int64_t total_ub = 0;        // sum of the list capacities
    explicit SymRows(smm_ctx *c) : prod(c), slists(c) {}
};

// Waves per workgroup (4, 2 or 1) that fit the most waves of wave_bytes of LDS each into a CU's 160 KB; returns how many
// (at most 32).  *per_wg keeps its value when not even one wave fits.
static int most_waves_per_cu(size_t wave_bytes, int *per_wg)
{
    int best = 0;
    for (int cand : {4, 2, 1}) {
        const int waves = (int)std::min<size_t>(32, ((size_t)160 * 1024 / (cand * wave_bytes)) * cand);
        if (waves > best) { best = waves; *per_wg = cand; }
    }
    return best;
}

// smm_symbolic_ccs over `units` (slab, row) units, or over the listed rows (n_slabs = 1), of the chunked column stream cc
static int launch_ccs(smm_ctx *c, const smm_plan *p, const smm_csr::CcsView &cc, int64_t units, int n_slabs, const int *rowlist,
                      const int *nrows, int *cnt, int *counter)
{
    const size_t wave_bytes = (size_t)(cc.bm_words + WAVE) * sizeof(unsigned);
    int cw = 4;
    most_waves_per_cu(wave_bytes, &cw);
    const size_t lds = wave_bytes * cw;
    const int sgrid = (int)std::min<int64_t>((units + cw - 1) / cw, (int64_t)c->n_cu * 8 * (4 / cw));
    const bool dr = c->sym_dense == 2 || (c->sym_dense == 1 && cc.same_word >= 0.8);
    const bool batch = units >= (int64_t)64 * sgrid * cw && units < INT32_MAX - (1 << 24);        // many short units: 16 per counter round trip
    auto kern = ccs_kernel((p->flags & SMM_SYMMETRIC) != 0, dr, batch);
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    LAUNCH(c, "smm_symbolic", kern, sgrid, cw * 64, lds, (int)p->m, n_slabs, rowlist, nrows, p->row_offset, cc.ws, cc.bm_words,
           (int)p->b->rows, (int64_t)p->a->nnz, cc.guard_chunk, p->a->ptr, p->a->idx, (const int *)cc.cptr, (const unsigned short *)cc.stream,
           (const int64_t *)p->d_ub_off, (unsigned short *)p->d_tmp, p->d_P, cnt, counter);
    LAUNCH_CHECK();
    return SMM_OK;
}

// The rows of C binned for the numeric phase into p->d_lists (5 x m), the bin sizes into p->n_bin.  prod (products per
// row) fills the tiny bins; without it they stay empty.
static int bin_c_rows(smm_ctx *c, smm_plan *p, const BinSpec &spec, const int64_t *prod)
{
    const int64_t m = p->m;
    CHK(pool_get(c, (size_t)5 * m, &p->d_lists));
    int *d_counts = (int *)((char *)c->d_flags + 320);
    HIPCHK(hipMemsetAsync(d_counts, 0, 8 * sizeof(int), c->stream));
    LAUNCH(c, "smm_bin_rows", smm_bin_rows<int>, std::min<int64_t>((m + 1023) / 1024, 2048), 1024, 0, (int)m, spec,
           (const int *)p->d_rowcnt, p->d_lists, d_counts, prod ? c->tiny_max : 0, prod, prod ? p->a->ptr : nullptr);
    HIPCHK(hipMemcpyAsync(p->n_bin, d_counts, 8 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

// Row work and bins: the capacities of the per-row ordered lists and their offsets (p->d_ub_off), the products per row,
// the rows of every bin of the symbolic phase.
static int sym_row_work(smm_ctx *c, smm_plan *p, SymRows &r)
{
    const smm_csr *a = p->a, *b = p->b;
    const int64_t m = p->m;
    const int sym = (p->flags & SMM_SYMMETRIC) ? 1 : 0;
    PoolBuf<int64_t> ub(c);
    CHK(r.prod.alloc((size_t)m));
    CHK(ub.alloc((size_t)m));
    CHK(pool_get(c, (size_t)m + 1, &p->d_ub_off));
    if (a->nnz <= 8 * m) {       // short rows on average: a row per lane instead of a row per wave; rows beyond 32 entries on a list
        PoolBuf<int> d_long(c);
        CHK(d_long.alloc((size_t)(a->nnz / ROW_WORK_SHORT_MAX + 2)));      // [0]: count, [1 ...]: rows
        HIPCHK(hipMemsetAsync(d_long, 0, sizeof(int), c->stream));
        LAUNCH(c, "smm_row_work", smm_row_work_short, (int)std::min<int64_t>((m + 255) / 256, 65536), 256, 0, (int)m, (int)p->ncols,
               p->row_offset, sym, a->ptr, a->idx, b->ptr, r.prod.p, ub.p, d_long + 1, d_long.p);
        LAUNCH(c, "smm_row_work", smm_row_work_listed, c->n_cu * 8, 256, 0, (const int *)d_long, (const int *)(d_long + 1), (int)p->ncols,
               p->row_offset, sym, a->ptr, a->idx, b->ptr, r.prod.p, ub.p);
    } else
        LAUNCH(c, "smm_row_work", smm_row_work, (int)std::min<int64_t>((m + 3) / 4, 16384), 256, 0, (int)m, (int)p->ncols, p->row_offset, sym,
               a->ptr, a->idx, b->ptr, r.prod.p, ub.p);
    CHK(scan_launch<int64_t>(c, m, ub, p->d_ub_off));
    const int bm_words = (int)((p->ncols + 31) / 32);
    const size_t bm_bytes = (size_t)(bm_words + 1) * sizeof(unsigned);      // + the guard word
    r.safe = (b->vflags & (CSR_HAS_EQUAL | CSR_UNSORTED)) != 0;
    int hmax[NHC];
    for (int i = 0; i < NHC; ++i) hmax[i] = (!r.safe && bm_bytes > (size_t)HS[i] * 4) ? HS[i] / 2 : (i ? hmax[i - 1] : 0);
    r.hmax1 = hmax[NHC - 1];
    r.binned = r.hmax1 > 0 || c->tiny_max > 0;
    r.sbin[SB_REST] = (int)m;
    int *d_scounts = (int *)((char *)c->d_flags + 256);
    if (r.binned) {
        CHK(r.slists.alloc((size_t)SB_N * m));
        HIPCHK(hipMemsetAsync(d_scounts, 0, 8 * sizeof(int), c->stream));
        BinSpec spec{NHC, {hmax[0], hmax[1], hmax[2], hmax[3], 0, 0}, SB_TINY, SB_TINY2};
        LAUNCH(c, "smm_bin_rows", smm_bin_rows<int64_t>, std::min<int64_t>((m + 1023) / 1024, 2048), 1024, 0, (int)m, spec,
               (const int64_t *)ub, r.slists.p, d_scounts, c->tiny_max, (const int64_t *)r.prod, a->ptr);
    }
    HIPCHK(hipMemcpyAsync(&r.total_ub, p->d_ub_off + m, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (r.binned) HIPCHK(hipMemcpyAsync(r.sbin, d_scounts, 8 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

// Column slabs (round 3): B wider than one slab of the chunked stream (or than smm_ctx_tune_symbolic allows), sorted,
// without repeated columns, and most rows beyond the hash-set classes -> every (slab, row) is walked on its own.
static bool use_slab_walk(const smm_ctx *c, const smm_plan *p, const SymRows &r)
{
    const int ws_cap = c->sym_max_ws > 0 ? c->sym_max_ws : CCS_MAX_WS;
    const bool wide = p->ncols > ws_cap && p->g.wc <= ws_cap && p->g.wc <= 32767;
    const bool dominant = c->sym_max_ws > 0 || r.hmax1 == 0 || 2 * (int64_t)r.sbin[SB_REST] >= p->m;
    return c->sym_ccs && c->narrow_idx && wide && dominant && !r.safe && p->b_sorted && c->slab_mode != 2;
}

// The column-slab walk: the (slab, row) lists over the chunked column stream, C's row pointer, every non-empty row binned
// for the tile kernel, and the slab sub-run table (smm_runs_slab).
static int sym_slab_walk(smm_ctx *c, smm_plan *p, SymRows &r)
{
    r.slists.reset();
    r.prod.reset();
    smm_csr *a = p->a, *b = p->b;
    const int64_t m = p->m;
    const int ws_cap = c->sym_max_ws > 0 ? c->sym_max_ws : CCS_MAX_WS;
    // tiles per slab: as many as fit the slab limit (<= 8), but not so many that the marker bitmap leaves fewer
    // than 28 waves per CU (configs[4] share: 3 tiles = 60 000 columns = 21 waves 12.4 ms, 2 tiles = 31 waves 11.7 ms)
    int tps = std::max(1, std::min(8, ws_cap / p->g.wc));
    if (c->sym_max_ws == 0)
        while (tps > 1 && (160 * 1024) / ((((tps * p->g.wc + 31) / 32) + WAVE) * 4) < 28) --tps;
    p->tps = tps; p->ws = tps * p->g.wc; p->n_slabs = (p->g.nct + tps - 1) / tps;
    p->list16 = true;
    const int ns = p->n_slabs;
    smm_csr::CcsView cc{};
    CHK(ensure_ccs(c, b, p->ws, ns, &cc));
    const int *sseg = nullptr;
    CHK(ensure_seg(c, b, tiles_geom(ns, p->ws), &sseg));
    // capacities and offsets of the (slab, row) lists
    PoolBuf<int64_t> ubs(c);
    CHK(ubs.alloc((size_t)ns * m));
    pool_free(c, p->d_ub_off); p->d_ub_off = nullptr;
    CHK(pool_get(c, (size_t)ns * m + 1, &p->d_ub_off));
    LAUNCH(c, "smm_row_work", smm_ccs_row_work, (int)std::min<int64_t>((m + 3) / 4, 16384), 256, 0, (int)m, ns, p->ws, (int)p->ncols,
           (int)b->rows, p->row_offset, (p->flags & SMM_SYMMETRIC) ? 1 : 0, a->ptr, a->idx, sseg, ubs.p);
    CHK(scan_launch<int64_t>(c, (int64_t)ns * m, ubs, p->d_ub_off));
    HIPCHK(hipMemcpyAsync(&p->total_cap, p->d_ub_off + (int64_t)ns * m, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    ubs.reset();
    // (+ slack: a list longer than its capacity -- a defect the plan checker reports -- and a sub-run table that
    // points past a list must still stay inside this allocation)
    CHK(pool_alloc(c, ((size_t)std::max<int64_t>(p->total_cap, 1) + LIST_SLACK) * 2, &p->d_tmp));
    CHK(pool_get(c, (size_t)a->nnz * ns, &p->d_P));
    CHK(pool_get(c, (size_t)ns * m, &p->d_scnt));
    CHK(pool_get(c, (size_t)m, &p->d_rowcnt));
    int *d_unitctr = (int *)((char *)c->d_flags + 208);
    HIPCHK(hipMemsetAsync(d_unitctr, 0, sizeof(int), c->stream));
    if ((int64_t)ns * m >= INT32_MAX) return fail(SMM_ERR_INVALID, "too many (slab, row) units");
    CHK(launch_ccs(c, p, cc, (int64_t)ns * m, ns, nullptr, nullptr, p->d_scnt, d_unitctr));
    LAUNCH(c, "smm_slab_rowcnt", smm_slab_rowcnt, std::min<int64_t>((m + 255) / 256, 4096), 256, 0, (int)m, ns, (const int *)p->d_scnt,
           p->d_rowcnt);
    CHK(scan_launch<int>(c, m, p->d_rowcnt, p->d_cptr));
    HIPCHK(hipMemcpyAsync(&p->nnz, p->d_cptr + m, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    LAUNCH_CHECK();
    // every non-empty row goes to the tile kernel (the hash kernels read one list per row)
    if (p->nnz > 0) CHK(bin_c_rows(c, p, BinSpec{2, {0, 0, 0, 0, 0, 0}, 3, 4}, nullptr));
    if (p->n_bin[2] > 0) {
        if (p->flags & SMM_EXACT) {
            CHK(ensure_seg(c, b, p->g, &p->seg));
            CHK(ensure_loc(c, b, p->g, &p->loc));
        } else {
            CHK(ensure_pack(c, b, p->g, PACK_FMT_16, &p->pack));
        }
        CHK(pool_get(c, (size_t)a->nnz, &p->d_dst0));
        CHK(pool_get(c, (size_t)a->nnz * p->g.nct, &p->d_runs2));
        CHK(pool_get(c, (size_t)m * p->g.nct, &p->d_tflag));
        const int nd = p->n_bin[2];
        LAUNCH(c, "smm_runs", smm_runs_slab, std::min<int64_t>((nd + 3) / 4, 65536), 256, 0, nd, (int)m, ns, tps, p->g.nct, p->g.wc,
               (int64_t)a->nnz, (const int *)(p->d_lists + 2 * m), a->ptr, (const int64_t *)p->d_ub_off, (const int *)p->d_scnt,
               (const unsigned *)p->d_P, (const unsigned short *)p->d_tmp, p->d_dst0, p->d_runs2, p->d_tflag, c->d_err);
        LAUNCH_CHECK();
    }
    return SMM_OK;
}

// The row walk: tiny rows, the hash classes, then the bitmap walk (or the walk over the chunked column stream) for the
// rest; C's row pointer.
static int sym_row_walk(smm_ctx *c, smm_plan *p, SymRows &r)
{
    smm_csr *a = p->a, *b = p->b;
    const int64_t m = p->m;
    const bool sym = (p->flags & SMM_SYMMETRIC) != 0;
    const bool safe = r.safe;
    p->list16 = c->narrow_idx && p->ncols < 65535 && b->cols < 65535;
    if (p->list16) CHK(ensure_idx16(c, b));
    p->total_cap = r.total_ub;
    CHK(pool_alloc(c, ((size_t)std::max<int64_t>(r.total_ub, 1) + std::max<size_t>(LIST_SLACK, (size_t)p->ncols)) * (p->list16 ? 2 : 4),
                   &p->d_tmp));
    CHK(pool_get(c, (size_t)a->nnz, &p->d_P));
    CHK(pool_get(c, (size_t)m, &p->d_rowcnt));
    if (r.binned) HIPCHK(hipMemsetAsync(p->d_rowcnt, 0, (size_t)m * sizeof(int), c->stream));   // rows without products are in no bin: their count stays 0
    // the kernels hand rows out through these counters (one per launch)
    int *d_rowctr = (int *)((char *)c->d_flags + 288);
    HIPCHK(hipMemsetAsync(d_rowctr, 0, 8 * sizeof(int), c->stream));
    int *d_scounts = (int *)((char *)c->d_flags + 256);
    const int *d_slists = r.slists;
    // tiny rows: four (<= 16 products) or two (<= 32) to a wave, no marker at all
    for (int tc = 0; tc < 2; ++tc) {
        const int bin = tc == 0 ? SB_TINY : SB_TINY2;
        const int nt = r.sbin[bin];
        if (nt == 0) continue;
        const int per_wg = tc == 0 ? 16 : 8;                         // rows per 256-thread workgroup
        const int tgrid = (int)std::min<int64_t>(((int64_t)nt + per_wg - 1) / per_wg, (int64_t)c->n_cu * 32);
        const int *rows3 = d_slists + (size_t)bin * m;
#define TINY_CASE(S, IT, G)                                                                                                      \
        LAUNCH(c, "smm_symbolic_tiny", (smm_symbolic_tiny<S, IT, G>), tgrid, 256, 0, nt, rows3, p->row_offset, a->ptr, a->idx,     \
               b->ptr, b->idx, (const int64_t *)p->d_ub_off, (IT *)p->d_tmp, p->d_P, p->d_rowcnt, c->d_err);
#define TINY_G_CASE(S, IT) if (tc == 0) { TINY_CASE(S, IT, TINY_G) } else { TINY_CASE(S, IT, TINY_G2) }
        if (p->list16) { if (sym) { TINY_G_CASE(true, unsigned short) } else { TINY_G_CASE(false, unsigned short) } }
        else           { if (sym) { TINY_G_CASE(true, int) } else { TINY_G_CASE(false, int) } }
#undef TINY_G_CASE
#undef TINY_CASE
        LAUNCH_CHECK();
    }
    // hash classes: one wave per row, four rows per workgroup
    for (int cls = 0; cls < NHC; ++cls) {
        if (r.hmax1 == 0 || r.sbin[cls] == 0) continue;
        const int hs = HS[cls];
        const int hgrid = (int)std::min<int64_t>((r.sbin[cls] + 3) / 4, (int64_t)c->n_cu * 16);
        if (sym) CHK((launch_symbolic_t<true, false, MARK_LDS_HASH>(c, p, hs, nullptr, hgrid, 4, d_slists + (size_t)cls * m, d_scounts + cls, d_rowctr + cls)));
        else     CHK((launch_symbolic_t<false, false, MARK_LDS_HASH>(c, p, hs, nullptr, hgrid, 4, d_slists + (size_t)cls * m, d_scounts + cls, d_rowctr + cls)));
    }
    // bitmap kernels for the rest: one wave per row; waves per workgroup are chosen so that as many
    // waves as possible fit a CU's 160 KB
    const int bm_words = (int)((p->ncols + 31) / 32);
    const size_t bm_bytes = (size_t)(bm_words + 1) * sizeof(unsigned);      // + the guard word
    const bool ldsbm = bm_bytes <= 128 * 1024;
    const int64_t nbm = r.binned ? r.sbin[SB_REST] : m;
    const int *bm_rows = r.binned ? d_slists + (size_t)SB_REST * m : nullptr;
    const int *bm_count = r.binned ? d_scounts + SB_REST : nullptr;
    int wpb = 4, waves_per_cu = 8;
    if (ldsbm) waves_per_cu = most_waves_per_cu(bm_bytes, &wpb);
    // few waves per CU (wide bitmaps): a round is one memory round trip whatever it carries -> 32 loads in flight
    const bool deep = !safe && waves_per_cu <= 8;
    PoolBuf<unsigned> gbm(c);
    // Round 3: sorted B without repeated columns and 16-bit lists -> the walk over the chunk-padded stream
    const bool use_ccs = c->sym_ccs && p->list16 && !safe && p->ncols <= CCS_MAX_WS && nbm > 0;
    if (use_ccs) {
        smm_csr::CcsView cc{};
        CHK(ensure_ccs(c, b, (int)p->ncols, 1, &cc));
        CHK(launch_ccs(c, p, cc, nbm, 1, bm_rows, bm_count, p->d_rowcnt, d_rowctr + SB_REST));
    } else if (nbm > 0) {
        int sgrid = (int)std::min<int64_t>((nbm + wpb - 1) / wpb, (int64_t)c->n_cu * 8 * (4 / wpb));
        if (!ldsbm) CHK(gbm.alloc((size_t)sgrid * wpb * (bm_words + 1)));
        const int mark = ldsbm ? MARK_LDS_BITMAP : MARK_GLOBAL_BITMAP;
        // (round 4) many short rows: 16 per counter round trip (one atomic per row on one word is 11 ns of L2 time each)
        const int rbatch = nbm >= (int64_t)64 * sgrid * wpb && nbm < INT32_MAX - (1 << 24) ? 16 : 1;
#define SYM_CASE(S, F, L) if (sym == S && safe == F && mark == L && !deep) CHK((launch_symbolic_t<S, F, L>(c, p, bm_words, gbm, sgrid, wpb, bm_rows, bm_count, d_rowctr + SB_REST, rbatch)));
        SYM_CASE(false, false, MARK_LDS_BITMAP) SYM_CASE(false, true, MARK_LDS_BITMAP) SYM_CASE(true, false, MARK_LDS_BITMAP)
        SYM_CASE(true, true, MARK_LDS_BITMAP) SYM_CASE(false, false, MARK_GLOBAL_BITMAP) SYM_CASE(false, true, MARK_GLOBAL_BITMAP)
        SYM_CASE(true, false, MARK_GLOBAL_BITMAP) SYM_CASE(true, true, MARK_GLOBAL_BITMAP)
#define SYM_DEEP(S, L) if (sym == S && mark == L && deep) CHK((launch_symbolic_t<S, false, L, 32>(c, p, bm_words, gbm, sgrid, wpb, bm_rows, bm_count, d_rowctr + SB_REST, rbatch)));
        SYM_DEEP(false, MARK_LDS_BITMAP) SYM_DEEP(true, MARK_LDS_BITMAP) SYM_DEEP(false, MARK_GLOBAL_BITMAP) SYM_DEEP(true, MARK_GLOBAL_BITMAP)
#undef SYM_DEEP
#undef SYM_CASE
    }
    CHK(scan_launch<int>(c, m, p->d_rowcnt, p->d_cptr));
    HIPCHK(hipMemcpyAsync(&p->nnz, p->d_cptr + m, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    LAUNCH_CHECK();
    gbm.reset();
    r.slists.reset();
    return SMM_OK;
}

// The rows of C binned (few nonzeros -> LDS hash kernels, the rest -> dense LDS tiles) and, for the dense-tile rows, the
// slab path's choice, B's tile index or packed payload, and the sub-run table (smm_runs).
static int sym_runs(smm_ctx *c, smm_plan *p, SymRows &r)
{
    smm_csr *a = p->a, *b = p->b;
    const int64_t m = p->m;
    if (p->nnz > 0) CHK(bin_c_rows(c, p, BinSpec{2, {c->hash_small, c->hash_medium, 0, 0, 0, 0}, 3, 4}, r.prod));
    r.prod.reset();
    if (!p->b_sorted || p->n_bin[2] == 0) return SMM_OK;
    const double est_products = (double)a->nnz * ((double)b->nnz / (double)std::max<int64_t>(b->rows, 1)) * ((double)p->n_bin[2] / (double)m);
    p->use_slab = slab_geometry(c, b, p->ncols, &p->sg) &&
                  slab_pays(c, a, p->sg, (double)p->n_bin[2] * (double)p->ncols, est_products, (double)p->nnz,
                            (double)b->nnz / (double)std::max<int64_t>(b->rows, 1), (double)p->ncols);
    if (p->use_slab) CHK(ensure_slab(c, b, p->sg, &p->slab));
    // (chosen by the heuristic, not forced: the tile kernel's index is built as well, so that the numeric
    // phase can fall back to it when the slab path's dense scratch does not fit)
    if (p->use_slab && c->slab_mode == 2) { /* forced: slab only */ }
    else if (p->flags & SMM_EXACT) {
        CHK(ensure_seg(c, b, p->g, &p->seg));
        CHK(ensure_loc(c, b, p->g, &p->loc));
    } else {
        // (pack12 where the rule chooses it, the 16-bit payload otherwise; the slab path's fall-back keeps 16 bits)
        CHK(ensure_pack(c, b, p->g, p->use_slab ? PACK_FMT_16 : PACK_FMT_12, &p->pack));
    }
    CHK(pool_get(c, (size_t)a->nnz * (p->g.nct + 1), &p->d_runs));
    CHK(pool_get(c, (size_t)m, &p->d_tail));
    const int nd = p->n_bin[2];
    const int rgrid = (int)std::min<int64_t>((nd + 3) / 4, 65536);
    const int tail_min = (p->flags & SMM_EXACT) ? TAIL_MIN_EXACT : TAIL_MIN_DEFAULT;
    if (p->list16)
        LAUNCH(c, "smm_runs", smm_runs<unsigned short>, rgrid, 256, 0, nd, p->g.nct, p->g.wc, (const int *)(p->d_lists + 2 * m), a->ptr,
               p->d_ub_off, p->d_rowcnt, p->d_P, (const unsigned short *)p->d_tmp, p->d_runs, p->d_tail, c->d_err, tail_min);
    else
        LAUNCH(c, "smm_runs", smm_runs<int>, rgrid, 256, 0, nd, p->g.nct, p->g.wc, (const int *)(p->d_lists + 2 * m), a->ptr,
               p->d_ub_off, p->d_rowcnt, p->d_P, (const int *)p->d_tmp, p->d_runs, p->d_tail, c->d_err, tail_min);
    LAUNCH_CHECK();
    return SMM_OK;
}

extern "C" int smm_spgemm_symbolic(smm_ctx *c, smm_csr *a, smm_csr *b, int flags, int64_t a_row_offset,
                                   smm_plan **plan, int64_t *nnz_out)
{
    if (!plan) return fail(SMM_ERR_INVALID, "plan is NULL");
    *plan = nullptr;
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(check_pair(c, a, b));
    if (a_row_offset < 0) return fail(SMM_ERR_INVALID, "negative a_row_offset");
    CHK(exact_guard(c, flags));
    PlanPtr p(new smm_plan());
    p->ctx = c; p->a = a; p->b = b; p->flags = flags; p->row_offset = a_row_offset;
    p->m = a->rows; p->ncols = b->cols;
    p->b_sorted = !(b->vflags & CSR_UNSORTED);
    p->g = make_geom(c, p->ncols, b, (flags & SMM_EXACT) != 0);
    CHK(pool_get(c, (size_t)p->m + 1, &p->d_cptr));
    if (p->m == 0 || a->nnz == 0 || b->nnz == 0 || p->ncols == 0) {
        // sparse_sparse_sparse.cpp:181-185: zero operand -> rowPtr of zeros only
        HIPCHK(hipMemsetAsync(p->d_cptr, 0, (p->m + 1) * sizeof(int64_t), c->stream));
    } else {
        SymRows r(c);
        CHK(sym_row_work(c, p.get(), r));
        if (use_slab_walk(c, p.get(), r)) {
            CHK(sym_slab_walk(c, p.get(), r));
        } else {
            CHK(sym_row_walk(c, p.get(), r));
            CHK(sym_runs(c, p.get(), r));
        }
        if (c->check) CHK(plan_check(c, p.get()));
    }
    if (nnz_out) *nnz_out = p->nnz;
    *plan = p.release();
    return SMM_OK;
}

extern "C" int smm_spgemm_numeric(smm_ctx *c, smm_plan *p, int64_t *d_c_indptr, int32_t *d_c_indices, double *d_c_data)
{
    if (!c || !p || p->ctx != c) return fail(SMM_ERR_INVALID, "bad plan/context");
    if (!d_c_indptr) return fail(SMM_ERR_INVALID, "d_c_indptr is NULL");
    HIPCHK(hipSetDevice(c->device));
    CTX_LOCK(c);
    const int64_t m = p->m;
    HIPCHK(hipMemcpyAsync(d_c_indptr, p->d_cptr, (m + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
    if (p->nnz == 0) return SMM_OK;
    if (!d_c_indices || !d_c_data) return fail(SMM_ERR_INVALID, "output arrays are NULL but nnz > 0");
    const bool sym = p->flags & SMM_SYMMETRIC;
    const bool exact = (p->flags & SMM_EXACT) != 0;
    // rows with few nonzeros: LDS hash kernels (whole rows of B; B need not be sorted)
    if (p->n_bin[0] > 0 || p->n_bin[1] > 0) {
        HashArgs H{};
        H.row_offset = p->row_offset;
        H.a_ptr = p->a->ptr; H.a_idx = p->a->idx; H.a_val = p->a->val;
        H.b_ptr = p->b->ptr; H.b_idx = p->b->idx; H.b_val = p->b->val;
        H.c_ptr = p->d_cptr; H.c_idx = d_c_indices; H.c_val = d_c_data;
        H.ub_off = p->d_ub_off; H.tmp_idx = p->d_tmp; H.list16 = p->list16 ? 1 : 0;
        H.dummy_idx = (const int *)((const char *)c->d_flags + 64);
        H.dummy_val = (const double *)((const char *)c->d_flags + 128);
        H.err = c->d_err;
        if (p->n_bin[0] > 0) {      // one wave per row, four rows per workgroup (always reference order)
            H.nrows = p->n_bin[0]; H.rowlist = p->d_lists;
            const int grid = (int)std::min<int64_t>((H.nrows + 3) / 4, (int64_t)c->n_cu * 32);
            if (sym) LAUNCH(c, "smm_numeric_hash", (smm_numeric_hash<true, 512, 1, 4>), grid, 256, 0, H);
            else     LAUNCH(c, "smm_numeric_hash", (smm_numeric_hash<false, 512, 1, 4>), grid, 256, 0, H);
        }
        if (p->n_bin[1] > 0) {      // one workgroup per row; SMM_EXACT: a single wave keeps the order
            H.nrows = p->n_bin[1]; H.rowlist = p->d_lists + m;
            const int grid = (int)std::min<int64_t>(H.nrows, (int64_t)c->n_cu * 16);
            if (exact) {
                if (sym) LAUNCH(c, "smm_numeric_hash", (smm_numeric_hash<true, 4096, 1, 1>), grid, 64, 0, H);
                else     LAUNCH(c, "smm_numeric_hash", (smm_numeric_hash<false, 4096, 1, 1>), grid, 64, 0, H);
            } else {
                if (sym) LAUNCH(c, "smm_numeric_hash", (smm_numeric_hash<true, 4096, 4, 1>), grid, 256, 0, H);
                else     LAUNCH(c, "smm_numeric_hash", (smm_numeric_hash<false, 4096, 4, 1>), grid, 256, 0, H);
            }
        }
        LAUNCH_CHECK();
    }
    // tiny rows: four / two to a wave, first touch found among the lanes (always the reference's order of additions)
    for (int tc = 0; tc < 2; ++tc) {
        const int nt = p->n_bin[3 + tc];
        if (nt == 0) continue;
        const int per_wg = tc == 0 ? 16 : 8;
        const int tgrid = (int)std::min<int64_t>(((int64_t)nt + per_wg - 1) / per_wg, (int64_t)c->n_cu * 32);
        const int *rows3 = p->d_lists + (size_t)(3 + tc) * m;
#define TINY_NUM(S, G) LAUNCH(c, "smm_numeric_tiny", (smm_numeric_tiny<S, G>), tgrid, 256, 0, nt, rows3, p->row_offset, p->a->ptr, p->a->idx, \
                              p->a->val, p->b->ptr, p->b->idx, p->b->val, (const int64_t *)p->d_cptr, d_c_indices, d_c_data, c->d_err)
        if (tc == 0) { if (sym) TINY_NUM(true, TINY_G); else TINY_NUM(false, TINY_G); }
        else         { if (sym) TINY_NUM(true, TINY_G2); else TINY_NUM(false, TINY_G2); }
#undef TINY_NUM
        LAUNCH_CHECK();
    }
    if (p->n_bin[2] == 0) return SMM_OK;
    const int nd = p->n_bin[2];
    const int *dense_rows = p->d_lists + 2 * m;
    if (p->b_sorted) {
        NumericArgs A{};
        A.m = nd; A.ncols = (int)p->ncols; A.nct = p->g.nct; A.wc = p->g.wc; A.wf = p->g.wf; A.n_ft = p->g.n_ft;
        A.row_offset = p->row_offset;
        A.rowlist = dense_rows;
        A.a_ptr = p->a->ptr; A.a_idx = p->a->idx; A.a_val = p->a->val;
        A.b_idx = p->b->idx; A.b_val = p->b->val; A.seg = p->seg; A.b_loc = p->loc;
        A.kmax = (int)std::max<int64_t>(p->b->nnz - 1, 0);
        A.tdesc = p->pack.desc; A.tpay = p->pack.pay;
        A.piece_epl = !c->piece_walk || !p->pack.pay ? 0 : (p->pack.maxlen <= 128 ? 2 : (p->pack.maxlen <= 256 ? 4 : 0));
        A.piece_fmt = p->pack.fmt;
        A.tstride = p->pack.stride; A.tlen16 = p->pack.len16;
        if (A.piece_fmt == PACK_FMT_12 && A.piece_epl != 4) return fail(SMM_ERR_INTERNAL, "pack12 payload without the four-entries-per-lane walk");
        A.rowsB = (int)p->b->rows;
        A.c_ptr = p->d_cptr; A.c_idx = d_c_indices; A.c_val = d_c_data;
        A.ub_off = p->d_ub_off; A.tmp_idx = p->d_tmp; A.list16 = p->list16 ? 1 : 0; A.runs = p->d_runs; A.tail = p->d_tail;
        A.runs2 = p->d_runs2; A.tflag = p->d_tflag; A.n_slabs = p->n_slabs; A.tps = p->tps; A.ws = p->ws; A.mtot = (int)m; A.nnzA = p->a->nnz;
        if (p->use_slab) {
            // values in column order into a dense scratch (one row per row of the bin), then the emission
            PoolBuf<double> scratch(c);
            const int rc = scratch.alloc((size_t)nd * (size_t)p->ncols);
            if (rc != SMM_OK) {
                if (!(p->pack.pay || p->seg)) return rc;         // slab path forced: no tile index to fall back to
                return launch_numeric<OUT_SPARSE>(c, A, sym, p->g.nw, exact);
            }
            CHK(launch_slab<true>(c, p->a, p->b, p->slab, p->sg.rw, nd, dense_rows, sym, p->row_offset, scratch, p->ncols));
            A.c_dense = scratch; A.ldc = p->ncols;
            A.dummy_idx = (const int *)((const char *)c->d_flags + 64);
            A.dummy_val = (const double *)((const char *)c->d_flags + 128);
            A.err = c->d_err;
            return sym ? launch_numeric_t<OUT_SPARSE, true, 16, false, true>(c, A) : launch_numeric_t<OUT_SPARSE, false, 16, false, true>(c, A);
        }
        CHK(launch_numeric<OUT_SPARSE>(c, A, sym, p->g.nw, exact));
    } else {
        const int cgrid = (int)std::min<int64_t>(nd, 65536);
        LAUNCH(c, "smm_copy_lists", smm_copy_lists, cgrid, 256, 0, nd, dense_rows, p->d_ub_off, p->d_cptr, (const void *)p->d_tmp,
               p->list16 ? 1 : 0, d_c_indices);
        LAUNCH_CHECK();
        const int grid = (int)std::min<int64_t>((nd + 3) / 4, (int64_t)c->n_cu * 2);
        PoolBuf<int> slot(c);
        // SMM_EXACT: the ordered variant (read-modify-write in the reference's order instead of atomics; a second map per wave)
        CHK(slot.alloc((size_t)grid * 4 * (size_t)p->ncols * (exact ? 2 : 1)));
#define GEN_CASE(S, O)                                                                                                        \
        if (sym == S && exact == O)                                                                                           \
            LAUNCH(c, "smm_numeric_general", (smm_numeric_general<S, O>), grid, 256, 0, nd, (int)p->ncols, p->row_offset,      \
                   dense_rows, p->a->ptr, p->a->idx, p->a->val, p->b->ptr, p->b->idx, p->b->val, p->d_cptr,                   \
                   (const int *)d_c_indices, d_c_data, slot);
        GEN_CASE(false, false) GEN_CASE(true, false) GEN_CASE(false, true) GEN_CASE(true, true)
#undef GEN_CASE
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SMM_OK;
}

extern "C" int smm_plan_indptr_host(smm_ctx *c, smm_plan *p, int64_t *c_indptr)
{
    if (!c || !p || !c_indptr) return fail(SMM_ERR_INVALID, "NULL argument");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c_indptr, p->d_cptr, (p->m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

static int numeric_host(smm_ctx *c, smm_plan *p, int64_t *c_indptr, void *c_indices, double *c_data, bool wide);
extern "C" int smm_spgemm_numeric_host(smm_ctx *c, smm_plan *p, int64_t *c_indptr, int32_t *c_indices, double *c_data)
{
    return numeric_host(c, p, c_indptr, c_indices, c_data, false);
}
extern "C" int smm_spgemm_numeric_host_i64(smm_ctx *c, smm_plan *p, int64_t *c_indptr, int64_t *c_indices, double *c_data)
{
    return numeric_host(c, p, c_indptr, c_indices, c_data, true);
}
static int numeric_host(smm_ctx *c, smm_plan *p, int64_t *c_indptr, void *c_indices, double *c_data, bool wide)
{
    if (!c || !p || !c_indptr) return fail(SMM_ERR_INVALID, "NULL argument");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    PoolBuf<int64_t> dp(c); PoolBuf<int> di(c); PoolBuf<double> dv(c);
    const int64_t nnz = p->nnz;
    CHK(dp.alloc((size_t)p->m + 1));
    CHK(di.alloc((size_t)std::max<int64_t>(nnz, 1)));
    CHK(dv.alloc((size_t)std::max<int64_t>(nnz, 1)));
    CHK(smm_spgemm_numeric(c, p, dp, di, dv));
    if (nnz > 0 && (!c_indices || !c_data)) return fail(SMM_ERR_INVALID, "output arrays are NULL but nnz > 0");
    CHK(download(c, c_indptr, dp, (size_t)(p->m + 1) * sizeof(int64_t)));
    if (nnz > 0) {
        CHK(download(c, c_indices, di, (size_t)nnz * sizeof(int), wide));
        CHK(download(c, c_data, dv, (size_t)nnz * sizeof(double)));
    }
    (void)hipStreamSynchronize(c->stream);
    dp.reset(); di.reset(); dv.reset();
    return take_plan_error(c, "smm_spgemm_numeric");       // what the kernels' clamps recorded, if anything
}

// ------------------------------------------------------------------------------ CSR x CSR -> dense
static int dense_into(smm_ctx *c, smm_csr *a, smm_csr *b, int flags, int64_t row_offset, double *d_c, int64_t ldc)
{
    const int64_t m = a->rows, n = b->cols;
    if (m == 0 || n == 0) return SMM_OK;
    const bool sym = flags & SMM_SYMMETRIC;
    if (a->nnz == 0 || b->nnz == 0) {
        HIPCHK(hipMemset2DAsync(d_c, ldc * sizeof(double), 0, n * sizeof(double), m, c->stream));
        return SMM_OK;
    }
    SlabGeom sg;
    if (slab_geometry(c, b, n, &sg) &&
        slab_pays(c, a, sg, (double)m * (double)n, (double)a->nnz * ((double)b->nnz / (double)std::max<int64_t>(b->rows, 1)), -1.0,
                  (double)b->nnz / (double)std::max<int64_t>(b->rows, 1), (double)n)) {
        smm_csr::SlabView sl{0, 0, nullptr, nullptr, nullptr};
        CHK(ensure_slab(c, b, sg, &sl));
        return launch_slab<false>(c, a, b, sl, sg.rw, (int)m, nullptr, sym, row_offset, d_c, ldc);
    }
    if (!(b->vflags & CSR_UNSORTED)) {
        Geom g = make_geom(c, n, b, (flags & SMM_EXACT) != 0);
        const int *seg = nullptr; const short *loc = nullptr;
        smm_csr::PackView pack{0, 0, nullptr, nullptr, 0, 0};
        if (flags & SMM_EXACT) {
            CHK(ensure_seg(c, b, g, &seg));
            CHK(ensure_loc(c, b, g, &loc));
        } else {
            CHK(ensure_pack(c, b, g, PACK_FMT_16, &pack));
        }
        NumericArgs A{};
        A.m = (int)m; A.ncols = (int)n; A.nct = g.nct; A.wc = g.wc; A.wf = g.wf; A.n_ft = g.n_ft;
        A.row_offset = row_offset;
        A.a_ptr = a->ptr; A.a_idx = a->idx; A.a_val = a->val;
        A.b_idx = b->idx; A.b_val = b->val; A.seg = seg; A.b_loc = loc;
        A.kmax = (int)std::max<int64_t>(b->nnz - 1, 0);
        A.tdesc = pack.desc; A.tpay = pack.pay;
        // (dense output keeps the chunk walk: the piece walk measured 0.9 ms slower at configs[2] and 1.2-2 ms at stage 1 of
        // configs[3] with 1-3 pieces in flight -- profiles/r3_c_piece_walk.txt; env SMM_PIECE_WALK=2 forces it here too)
        A.piece_epl = c->piece_walk < 2 || !pack.pay ? 0 : (pack.maxlen <= 128 ? 2 : (pack.maxlen <= 256 ? 4 : 0));
        A.rowsB = (int)b->rows;
        A.c_dense = d_c; A.ldc = ldc;
        CHK(launch_numeric<OUT_DENSE>(c, A, sym, g.nw, (flags & SMM_EXACT) != 0));
    } else {
        const bool ordered = (flags & SMM_EXACT) != 0;
        const int grid = (int)std::min<int64_t>((m + 3) / 4, ordered ? (int64_t)c->n_cu * 2 : 65536);
        PoolBuf<int> owner(c);
        if (ordered) CHK(owner.alloc((size_t)grid * 4 * (size_t)n));
#define GEN_CASE(S, O)                                                                                                        \
        if (sym == S && ordered == O)                                                                                         \
            LAUNCH(c, "smm_dense_general", (smm_dense_general<S, O>), grid, 256, 0, (int)m, (int)n, row_offset, a->ptr, a->idx, \
                   a->val, b->ptr, b->idx, b->val, d_c, ldc, owner);
        GEN_CASE(false, false) GEN_CASE(true, false) GEN_CASE(false, true) GEN_CASE(true, true)
#undef GEN_CASE
        LAUNCH_CHECK();
        if (owner) HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SMM_OK;
}

static int mirror_upper(smm_ctx *c, int64_t n, double *d_c, int64_t ldc)
{
    if (n <= 1) return SMM_OK;
    const int64_t tiles = (n + 63) / 64;
    const int64_t pairs = tiles * (tiles + 1) / 2;
    if (pairs > 0x7fffffff) return fail(SMM_ERR_INVALID, "matrix too large for the mirror epilogue");
    LAUNCH(c, "smm_mirror_upper", smm_mirror_upper, pairs, 256, 0, (int)n, d_c, ldc);
    LAUNCH_CHECK();
    return SMM_OK;
}

extern "C" int smm_spgemm_dense(smm_ctx *c, smm_csr *a, smm_csr *b, int flags, int64_t a_row_offset, double *d_c)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(check_pair(c, a, b));
    CHK(exact_guard(c, flags));
    if (!d_c && a->rows * b->cols > 0) return fail(SMM_ERR_INVALID, "d_c is NULL");
    if (flags & SMM_MIRROR) {
        if (!(flags & SMM_SYMMETRIC) || a->rows != b->cols || a_row_offset != 0)
            return fail(SMM_ERR_INVALID, "SMM_MIRROR needs SMM_SYMMETRIC and the whole square result (no row shard)");
    }
    CHK(dense_into(c, a, b, flags, a_row_offset, d_c, b->cols));
    if (flags & SMM_MIRROR) CHK(mirror_upper(c, b->cols, d_c, b->cols));
    return SMM_OK;
}

extern "C" int smm_spgemm_dense_host(smm_ctx *c, smm_csr *a, smm_csr *b, int flags, int64_t a_row_offset, double *out)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(check_pair(c, a, b));
    const int64_t total = a->rows * b->cols;
    if (total == 0) return SMM_OK;
    if (!out) return fail(SMM_ERR_INVALID, "c is NULL");
    PoolBuf<double> d(c);
    CHK(d.alloc((size_t)total));
    CHK(smm_spgemm_dense(c, a, b, flags, a_row_offset, d));
    CHK(download(c, out, d, (size_t)total * sizeof(double)));
    (void)hipStreamSynchronize(c->stream);
    return SMM_OK;
}

// ------------------------------------------------------------------------------ CSR mirror epilogue
//  upper-triangle CSR in HBM -> full symmetric CSR in HBM, two calls: row pointer + nnz, then fill.
extern "C" int smm_csr_mirror_symbolic(smm_ctx *c, int64_t n, const int64_t *d_indptr, const int32_t *d_indices,
                                       int64_t *d_full_indptr, int64_t *nnz_full)
{
    if (!c || !d_indptr || !d_full_indptr || !nnz_full) return fail(SMM_ERR_INVALID, "NULL argument");
    if (n < 0 || n >= INT32_MAX) return fail(SMM_ERR_INVALID, "bad dimension");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    *nnz_full = 0;
    if (n == 0) { HIPCHK(hipMemsetAsync(d_full_indptr, 0, sizeof(int64_t), c->stream)); return SMM_OK; }
    PoolBuf<int> mcnt(c);
    PoolBuf<int64_t> flen(c);
    CHK(mcnt.alloc((size_t)n + 1));                       // [n] = longest mirrored segment
    CHK(flen.alloc((size_t)n));
    HIPCHK(hipMemsetAsync(mcnt, 0, ((size_t)n + 1) * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(c->d_flags, 0, sizeof(unsigned), c->stream));
    const int grid = (int)std::min<int64_t>((n + 3) / 4, 16384);
    LAUNCH(c, "smm_mirror_count", smm_mirror_count, grid, 256, 0, (int)n, d_indptr, d_indices, mcnt, c->d_flags);
    LAUNCH(c, "smm_mirror_rowlen", smm_mirror_rowlen, std::min<int64_t>((n + 255) / 256, 4096), 256, 0, (int)n, d_indptr, (const int *)mcnt,
           flen, mcnt + n);
    CHK(scan_launch<int64_t>(c, n, flen, d_full_indptr));
    unsigned bad = 0; int maxseg = 0;
    HIPCHK(hipMemcpyAsync(nnz_full, d_full_indptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&bad, c->d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&maxseg, mcnt + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad) return fail(SMM_ERR_INVALID, "CSR mirror: the input holds entries left of the diagonal or outside the n x n square");
    (void)maxseg;                 // (any length: segments beyond the LDS sort are placed by rank, smm_mirror_rank)
    return SMM_OK;
}

extern "C" int smm_csr_mirror_fill(smm_ctx *c, int64_t n, const int64_t *d_indptr, const int32_t *d_indices, const double *d_data,
                                   const int64_t *d_full_indptr, int32_t *d_full_indices, double *d_full_data)
{
    if (!c || !d_indptr || !d_full_indptr) return fail(SMM_ERR_INVALID, "NULL argument");
    if (n <= 0) return SMM_OK;
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    if (!d_indices || !d_data || !d_full_indices || !d_full_data) return fail(SMM_ERR_INVALID, "NULL CSR array");
    PoolBuf<int> mcnt(c), cursor(c);
    CHK(mcnt.alloc((size_t)n));
    CHK(cursor.alloc((size_t)n));
    HIPCHK(hipMemsetAsync(mcnt, 0, (size_t)n * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(cursor, 0, (size_t)n * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(c->d_flags, 0, sizeof(unsigned), c->stream));
    const int grid = (int)std::min<int64_t>((n + 3) / 4, 16384);
    LAUNCH(c, "smm_mirror_count", smm_mirror_count, grid, 256, 0, (int)n, d_indptr, d_indices, mcnt, c->d_flags);
    // rows that receive more mirrored entries than the LDS sort holds: their entries are staged and placed by rank
    PoolBuf<int64_t> big(c), toff(c);
    PoolBuf<int> tidx(c);
    PoolBuf<double> tval(c);
    int64_t total_big = 0;
    CHK(big.alloc((size_t)n));
    CHK(toff.alloc((size_t)n + 1));
    LAUNCH(c, "smm_mirror_big", smm_mirror_big, std::min<int64_t>((n + 255) / 256, 4096), 256, 0, (int)n, (const int *)mcnt, big);
    CHK(scan_launch<int64_t>(c, n, big, toff));
    HIPCHK(hipMemcpyAsync(&total_big, toff + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total_big > 0) {
        CHK(tidx.alloc((size_t)total_big));
        CHK(tval.alloc((size_t)total_big));
    }
    LAUNCH(c, "smm_mirror_fill", smm_mirror_fill, grid, 256, 0, (int)n, d_indptr, d_indices, d_data, d_full_indptr, (const int *)mcnt, cursor,
           d_full_indices, d_full_data, total_big > 0 ? (const int64_t *)toff : (const int64_t *)nullptr, tidx, tval);
    if (total_big > 0) {
        auto rk = smm_mirror_rank;
        const size_t rlds = (size_t)2 * RANK_WORDS * sizeof(unsigned);
        HIPCHK(hipFuncSetAttribute((const void *)rk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds));
        LAUNCH(c, "smm_mirror_rank", rk, std::min<int64_t>(n, (int64_t)c->n_cu * 4), 1024, rlds, (int)n, d_full_indptr, (const int *)mcnt,
               (const int64_t *)toff, (const int *)tidx, (const double *)tval, d_full_indices, d_full_data);
    }
    LAUNCH(c, "smm_mirror_sort", smm_mirror_sort<false>, grid, 256, 0, (int)n, d_full_indptr, (const int *)mcnt, d_full_indices, d_full_data);
    {
        auto kern = smm_mirror_sort<true>;
        const size_t lds = (size_t)MIRROR_MAX_SEG * (sizeof(double) + sizeof(int));
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        LAUNCH(c, "smm_mirror_sort", kern, std::min<int64_t>(n, (int64_t)c->n_cu * 4), 256, lds, (int)n, d_full_indptr, (const int *)mcnt,
               d_full_indices, d_full_data);
    }
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));     // mcnt / cursor / the staging array return to the pool
    return SMM_OK;
}

// ------------------------------------------------------------------------------ triple product
extern "C" int smm_triple_product(smm_ctx *c, smm_csr *h, smm_csr *q, int flags, int64_t row_begin, int64_t row_end,
                                  double *d_c)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(check_pair(c, h, q));
    CHK(exact_guard(c, flags));
    const int64_t n = h->rows, K = h->cols;
    // the reference indexes temp_values[K] with Q's columns (sparse_sparse_dense.cpp:178,196): Q may
    // be K x c with c <= K (columns c..K-1 of T stay 0); c > K would write out of bounds there
    if (q->cols > K) return fail(SMM_ERR_INVALID, "Q has more columns (%lld) than H (%lld)", (long long)q->cols, (long long)K);
    if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(SMM_ERR_INVALID, "bad row range");
    const bool full = flags & SMM_FULL_MATRIX;
    const bool mirror = (flags & SMM_MIRROR) != 0;
    if (full && mirror) return fail(SMM_ERR_INVALID, "SMM_FULL_MATRIX and SMM_MIRROR exclude each other");
    if ((full || mirror) && (row_begin != 0 || row_end != n))
        return fail(SMM_ERR_INVALID, "SMM_FULL_MATRIX / SMM_MIRROR need the whole row range [0,n)");
    const int64_t nr = row_end - row_begin;
    if (nr == 0 || n == 0) return SMM_OK;
    if (!d_c) return fail(SMM_ERR_INVALID, "d_c is NULL");
    if (h->nnz == 0 || q->nnz == 0 || K == 0) {
        HIPCHK(hipMemset2DAsync(d_c, n * sizeof(double), 0, n * sizeof(double), nr, c->stream));
        return SMM_OK;
    }
    // stage 1: T = H[row_begin:row_end, :] * Q, dense nr x K (sparse_sparse_dense.cpp:187-198)
    PoolBuf<double> T(c);
    CHK(T.alloc((size_t)nr * K));
    if (q->cols < K) HIPCHK(hipMemsetAsync(T, 0, (size_t)nr * K * sizeof(double), c->stream));
    smm_csr hv = csr_row_view(h, row_begin, nr);
    CHK(dense_into(c, &hv, q, flags & SMM_EXACT, 0, T, K));
    // stage 2
    if (h->vflags & CSR_UNSORTED) {
        // H with unsorted rows (legal CSR, e.g. an unsorted scipy product): the chunked ELL walk needs
        // sorted rows, so every (i,k) sums row k of H in its stored order, as the reference does
        dim3 grid((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(nr, 65535));
        {
            LaunchTimer lt_(c, "smm_triple_stage2_general");
            hipLaunchKernelGGL(smm_triple_stage2_general, grid, dim3(256), 0, c->stream, (int)n, (int)K, row_begin, row_end,
                               full ? 1 : 0, h->ptr, h->idx, h->val, (const double *)T, d_c, n);
        }
        if (full) LAUNCH(c, "smm_triple_mirror", smm_triple_mirror, (n * n + 255) / 256, 256, 0, (int)n, d_c, n);
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(c->stream));
        T.reset();
        if (mirror) CHK(mirror_upper(c, n, d_c, n));
        return SMM_OK;
    }
#ifndef SMM_S2_NW
#define SMM_S2_NW 16
#endif
    constexpr int NW = SMM_S2_NW;          // waves per workgroup = 64-row slices of H per k-group
    constexpr int R = 16;
    if (c->s2_ring && NW == 16 && (K + RING_PW - 1) / RING_PW < 65535) {
        // round 4: ring of column pieces, progress words instead of barriers (smm_ring.hpp)
        const bool exact_r = (flags & SMM_EXACT) != 0;
        CHK(ensure_ring(c, h, !exact_r));
        RingArgs A{};
        A.n = (int)n; A.K = (int)K; A.npieces = h->ring.npieces; A.nslices = (int)((n + WAVE - 1) / WAVE);
        A.nib = (int)((nr + R - 1) / R);
        A.row_begin = row_begin; A.row_end = row_end; A.full = full ? 1 : 0;
        A.off = h->ring.off; A.col = h->ring.col; A.val = h->ring.val; A.hdr = h->ring.hdr;
        A.T = T; A.C = d_c; A.ldc = n; A.err = c->d_err;
        const int64_t nkg = (n + 16 * WAVE - 1) / (16 * WAVE);
        A.nkg = (int)nkg;
        A.gk = (int)std::min<int64_t>(std::max(c->s2_group, 1), nkg);
        const int64_t grid2 = ((nkg + A.gk - 1) / A.gk) * A.gk * (((int64_t)A.nib + 7) / 8) * 8;
        if (grid2 > 0x7fffffff) return fail(SMM_ERR_INVALID, "triple product too large for one launch");
        const size_t lds = (size_t)RING_NB * RING_PW * (R + 2) * sizeof(double);
        auto kern = exact_r ? smm_triple_stage2_ring<R, 16, false> : smm_triple_stage2_ring<R, 16, true>;
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        LAUNCH(c, "smm_triple_stage2", kern, grid2, 16 * 64, lds, A);
        if (full) LAUNCH(c, "smm_triple_mirror", smm_triple_mirror, (n * n + 255) / 256, 256, 0, (int)n, d_c, n);
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(c->stream));   // T returns to the pool
        T.reset();
#ifdef SMM_RING_STAMPS
        {
            unsigned long long st[6];
            (void)hipMemcpy(st, c->d_err + 4, sizeof(st), hipMemcpyDeviceToHost);
            (void)hipMemset(c->d_err + 4, 0, sizeof(st));
            fprintf(stderr, "[SMM_RING_STAMPS] wave-cycles %.4g: waiting for pieces %.1f%%  tail (owed shares) %.1f%%;  slow-path entries %.3g, spins %.3g, steps %.3g\n",
                    (double)st[0], 100.0 * st[1] / st[0], 100.0 * st[2] / st[0], (double)st[3], (double)st[4], (double)st[5]);
        }
#endif
        CHK(take_plan_error(c, "smm_triple_product"));              // (a bounded wait of the ring protocol ran out: never expected)
        if (mirror) CHK(mirror_upper(c, n, d_c, n));
        return SMM_OK;
    }
    constexpr int chunk_cap = NW * 64;     // one tile column per thread; [chunk][R+2] f64 = 144 KB of LDS at 16 waves
    const int nchunks = (int)((K + chunk_cap - 1) / chunk_cap);
    const int chunk = (int)((K + nchunks - 1) / nchunks);
    const bool exact = (flags & SMM_EXACT) != 0;
    CHK(ensure_ell(c, h, nchunks, chunk, !exact));
    TripleArgs A{};
    A.n = (int)n; A.K = (int)K; A.nchunks = nchunks; A.chunk = chunk; A.nslices = (int)((n + WAVE - 1) / WAVE);
    A.nib = (int)((nr + R - 1) / R);
    A.row_begin = row_begin; A.row_end = row_end; A.full = full ? 1 : 0;
    A.off = h->ell.off; A.col = h->ell.col; A.val = h->ell.val;
    A.T = T; A.C = d_c; A.ldc = n;
    const size_t lds = (size_t)(R + 2) * chunk * sizeof(double);
    const int64_t nkg = (n + NW * WAVE - 1) / (NW * WAVE);
    auto kern = exact ? smm_triple_stage2<R, NW, chunk_cap, false> : smm_triple_stage2<R, NW, chunk_cap, true>;
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    A.nkg = (int)nkg;
    A.gk = (int)std::min<int64_t>(std::max(c->s2_group, 1), nkg);
    const int64_t grid2 = ((nkg + A.gk - 1) / A.gk) * A.gk * (((int64_t)A.nib + 7) / 8) * 8;
    if (grid2 > 0x7fffffff) return fail(SMM_ERR_INVALID, "triple product too large for one launch");
#ifdef SMM_S2_STAMPS
    PoolBuf<unsigned long long> d_st(c);
    if (d_st.alloc(8) == SMM_OK) { (void)hipMemsetAsync(d_st, 0, 64, c->stream); A.stamps = d_st; }
#endif
    LAUNCH(c, "smm_triple_stage2", kern, grid2, NW * 64, lds, A);
#ifdef SMM_S2_STAMPS
    if (d_st) {
        unsigned long long hst[8];
        (void)hipMemcpyAsync(hst, d_st, 64, hipMemcpyDeviceToHost, c->stream);
        (void)hipStreamSynchronize(c->stream);
        double tot = 0; for (int i = 0; i < 6; ++i) tot += (double)hst[i];
        fprintf(stderr, "[SMM_S2_STAMPS] wave-cycles %.4g: preload issue %.1f%%  barrier 1 %.1f%%  tile write %.1f%%  barrier 2 %.1f%%  tile load issue %.1f%%  steps %.1f%%\n",
                tot, 100 * hst[0] / tot, 100 * hst[1] / tot, 100 * hst[2] / tot, 100 * hst[3] / tot, 100 * hst[4] / tot, 100 * hst[5] / tot);
        d_st.reset();
    }
#endif
    if (full) LAUNCH(c, "smm_triple_mirror", smm_triple_mirror, (n * n + 255) / 256, 256, 0, (int)n, d_c, n);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));   // T returns to the pool
    T.reset();
    if (mirror) CHK(mirror_upper(c, n, d_c, n));
    return SMM_OK;
}

extern "C" int smm_triple_product_host(smm_ctx *c, smm_csr *h, smm_csr *q, int flags, int64_t row_begin,
                                       int64_t row_end, double *out)
{
    if (!c || !h || !q) return fail(SMM_ERR_INVALID, "NULL argument");
    CTX_LOCK(c);
    const int64_t n = h->rows, nr = row_end - row_begin;
    if (nr <= 0 || n == 0) return smm_triple_product(c, h, q, flags, row_begin, row_end, nullptr);
    if (!out) return fail(SMM_ERR_INVALID, "c is NULL");
    PoolBuf<double> d(c);
    CHK(d.alloc((size_t)nr * n));
    CHK(smm_triple_product(c, h, q, flags, row_begin, row_end, d));
    CHK(download(c, out, d, (size_t)nr * (size_t)n * sizeof(double)));
    (void)hipStreamSynchronize(c->stream);
    return SMM_OK;
}

// ------------------------------------------------------------------------------ device CSR transpose
// Segmented sort of distinct int keys in place (segments off[s] .. off[s+1], int64 offsets in HBM).
static int seg_sort(smm_ctx *c, int64_t nseg, const int64_t *off, int *key)
{
    if (nseg <= 0) return SMM_OK;
    LAUNCH(c, "smm_seg_sort", smm_seg_sort_short, std::min<int64_t>((nseg + 255) / 256, 16384), 256, 0, nseg, off, key);
    LAUNCH(c, "smm_seg_sort", smm_seg_sort<false>, std::min<int64_t>(nseg, (int64_t)c->n_cu * 4), 1024, 0, nseg, off, key);
    LAUNCH(c, "smm_seg_sort", smm_seg_sort<true>, std::min<int64_t>(nseg, (int64_t)c->n_cu), 1024, 0, nseg, off, key);
    LAUNCH_CHECK();
    return SMM_OK;
}

// A^T as a new owned operand; arrays exactly those of scipy's a.tocsc().
static int transpose_impl(smm_ctx *c, const smm_csr *a, CsrPtr *out)
{
    const int64_t rows = a->cols, nnz = a->nnz;
    CsrPtr m = new_csr(c, rows, a->rows, nnz);
    CHK(alloc_owned(c, m.get(), "the transposed operand"));
    {
        PoolBuf<int> cnt(c), key(c);
        PoolBuf<int64_t> off(c);
        CHK(cnt.alloc((size_t)rows + 1));
        CHK(off.alloc((size_t)rows + 1));
        CHK(key.alloc((size_t)std::max<int64_t>(nnz, 1)));
        HIPCHK(hipMemsetAsync(cnt, 0, ((size_t)rows + 1) * sizeof(int), c->stream));
        const int grid = (int)std::min<int64_t>(std::max<int64_t>((nnz + 255) / 256, 1), (int64_t)c->n_cu * 16);
        LAUNCH(c, "smm_transpose_count", smm_transpose_count, grid, 256, 0, nnz, a->idx, (int)rows, cnt);
        CHK(scan_launch<int>(c, rows, cnt, off));
        HIPCHK(hipMemsetAsync(cnt, 0, ((size_t)rows + 1) * sizeof(int), c->stream));       // (cursor of the scatter)
        LAUNCH(c, "smm_transpose_scatter", smm_transpose_scatter, grid, 256, 0, nnz, a->idx, (int)rows, (const int64_t *)off, cnt, key);
        CHK(seg_sort(c, rows, off, key));
        const int ggrid = (int)std::min<int64_t>(std::max<int64_t>(std::max(nnz, rows + 1) / 256 + 1, 1), (int64_t)c->n_cu * 16);
        LAUNCH(c, "smm_transpose_gather", smm_transpose_gather, ggrid, 256, 0, nnz, (int)a->rows, a->ptr, a->val, (const int *)key, (int)rows,
               (const int64_t *)off, m->own_ptr.p, m->own_idx.p, m->own_val.p);
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    CHK(validate(c, m.get()));              // (flags of the new operand: sorted rows, repeated columns where A repeats rows)
    *out = std::move(m);
    return SMM_OK;
}

extern "C" int smm_csr_transpose(smm_ctx *c, const smm_csr *a, smm_csr **out)
{
    if (!out) return fail(SMM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!c || !a) return fail(SMM_ERR_INVALID, "NULL argument");
    if (a->ctx != c) return fail(SMM_ERR_INVALID, "operand belongs to another context");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, (smm_csr *)a));
    CsrPtr t;
    CHK(transpose_impl(c, a, &t));
    *out = t.release();
    return SMM_OK;
}

extern "C" int smm_csr_download(smm_ctx *c, const smm_csr *m, int32_t *indptr, int32_t *indices, double *data)
{
    if (!c || !m || !indptr) return fail(SMM_ERR_INVALID, "NULL argument");
    if (m->ctx != c) return fail(SMM_ERR_INVALID, "operand belongs to another context");
    if (m->nnz > 0 && (!indices || !data)) return fail(SMM_ERR_INVALID, "output arrays are NULL but nnz > 0");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    CHK(download(c, indptr, m->ptr, ((size_t)m->rows + 1) * sizeof(int)));
    CHK(download(c, indices, m->idx, (size_t)m->nnz * sizeof(int)));
    CHK(download(c, data, m->val, (size_t)m->nnz * sizeof(double)));
    return SMM_OK;
}

// Device-to-device copy of an operand's own arrays (NULL skips one): how a caller that keeps results in HBM gets the
// pattern of a library-owned operand without the host.
extern "C" int smm_csr_copy_device(smm_ctx *c, const smm_csr *m, int32_t *d_indptr, int32_t *d_indices, double *d_data)
{
    if (!c || !m) return fail(SMM_ERR_INVALID, "NULL argument");
    if (m->ctx != c) return fail(SMM_ERR_INVALID, "operand belongs to another context");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    if (d_indptr) HIPCHK(hipMemcpyAsync(d_indptr, m->ptr, ((size_t)m->rows + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    if (d_indices && m->nnz > 0) HIPCHK(hipMemcpyAsync(d_indices, m->idx, (size_t)m->nnz * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    if (d_data && m->nnz > 0) HIPCHK(hipMemcpyAsync(d_data, m->val, (size_t)m->nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

// ------------------------------------------------------------------------------ localisation taper from coordinates
// (kernels and the cell-search argument: smm_taper.hpp; contract: include/smm_hip.h)
static int upload_rows(smm_ctx *c, double *d, const double *h, int64_t rows, int64_t k, int64_t ld);

// Most cells the grid over b may have: two per point (more cells than points only add empty ones; 12 bytes each),
// at least 4096, at most 2^30 (cell ids are int).
static double taper_cell_cap(int64_t nb)
{
    return (double)std::min<int64_t>(std::max<int64_t>(2 * nb, 4096), (int64_t)1 << 30);
}

// The grid over b's bounding box: edge = cutoff * (1 + 2^-20), grown by steps of 1.25 until the cells fit the cap.
// A dimension whose extent is not finite (coordinates near +-DBL_MAX) gets one cell.  Correctness of the search does
// not depend on anything chosen here (smm_taper.hpp): only the number of candidates does.
static TaperGrid taper_grid(int dim, double cutoff, const double *lo, const double *hi, int64_t nb)
{
    TaperGrid g{};
    g.cutoff = cutoff; g.cut2 = cutoff * cutoff; g.half = 0.5 * cutoff;
    double ext[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < 3; ++t) {
        g.nc[t] = 1;
        g.lo[t] = t < dim ? lo[t] : 0.0;
        g.hi[t] = t < dim ? hi[t] : 0.0;
        if (t < dim && std::isfinite(hi[t] - lo[t]) && hi[t] > lo[t]) ext[t] = hi[t] - lo[t];
    }
    const double cap = taper_cell_cap(nb);
    double h = cutoff * (1.0 + 0x1p-20);
    if (!(h >= cutoff) || !std::isfinite(h)) h = cutoff;
    for (;;) {
        const double inv = 1.0 / h;
        double n[3], total = 1.0;
        for (int t = 0; t < 3; ++t) { n[t] = std::floor(ext[t] * inv) + 1.0; total *= n[t]; }
        if (total <= cap || !std::isfinite(h * 1.25)) {
            if (total <= cap && inv > 0.0) { for (int t = 0; t < 3; ++t) g.nc[t] = (int)n[t]; g.inv_h = inv; }
            else g.inv_h = 0.0;                                     // (one cell: every nc stays 1)
            return g;
        }
        h *= 1.25;
    }
}

// Cell-order permutation of n points (order; with `sorted` also their coordinates in that order) and, with `start`, the
// first sorted position of every cell.  cell_of / cnt / scratch64: caller's temporaries (n, ncells + 1, ncells + 1).
template <int DIM>
static int taper_bin(smm_ctx *c, const TaperGrid &g, int ncells, int64_t n, const double *pts, int64_t ld, int *cell_of, int *cnt,
                     int64_t *start, int *order, double *sorted)
{
    const int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)c->n_cu * 16);
    HIPCHK(hipMemsetAsync(cnt, 0, ((size_t)ncells + 1) * sizeof(int), c->stream));
    LAUNCH(c, "smm_taper_bin", smm_taper_cell_count<DIM>, grid, 256, 0, g, n, pts, ld, ncells, cell_of, cnt);
    CHK(scan_launch<int>(c, ncells, cnt, start));
    HIPCHK(hipMemsetAsync(cnt, 0, ((size_t)ncells + 1) * sizeof(int), c->stream));           // (cursor of the scatter)
    LAUNCH(c, "smm_taper_bin", smm_taper_cell_scatter<DIM>, grid, 256, 0, n, pts, ld, ncells, (const int *)cell_of, (const int64_t *)start, cnt,
           order, sorted, c->d_err);
    LAUNCH_CHECK();
    return SMM_OK;
}

// Bounding box (box[0..2] min, box[3..5] max) and the number of non-finite coordinates of n > 0 points.
template <int DIM>
static int taper_bbox(smm_ctx *c, int64_t n, const double *pts, int64_t ld, double *box, double *bad)
{
    const int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)c->n_cu * 4);
    PoolBuf<double> part(c);
    CHK(part.alloc((size_t)grid * TP_PART));
    LAUNCH(c, "smm_taper_bbox", smm_taper_bbox<DIM>, grid, 256, 0, n, pts, ld, part.p);
    LAUNCH_CHECK();
    std::vector<double> h((size_t)grid * TP_PART);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int t = 0; t < 3; ++t) { box[t] = DBL_MAX; box[3 + t] = -DBL_MAX; }
    *bad = 0.0;
    for (int b = 0; b < grid; ++b) {
        const double *p = h.data() + (size_t)b * TP_PART;
        for (int t = 0; t < 3; ++t) { box[t] = std::min(box[t], p[t]); box[3 + t] = std::max(box[3 + t], p[3 + t]); }
        *bad += p[6];
    }
    return SMM_OK;
}

// An operand of rows x cols without entries: no launch (its flags are those smm_validate would find).
static int empty_csr(smm_ctx *c, int64_t rows, int64_t cols, CsrPtr *out)
{
    CsrPtr m = new_csr(c, rows, cols, 0);
    CHK(alloc_owned(c, m.get(), "an empty operand"));
    HIPCHK(hipMemsetAsync(m->own_ptr, 0, ((size_t)rows + 1) * sizeof(int), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    m->validated = true;
    m->vflags = 0;
    *out = std::move(m);
    return SMM_OK;
}

template <int DIM>
static int taper_impl(smm_ctx *c, int kind, double cutoff, int64_t na, const double *a, int64_t lda, int64_t nb, const double *b,
                      int64_t ldb, CsrPtr *out)
{
    const bool same = a == b && lda == ldb && na == nb;
    double box[6], bad = 0.0, abox[6], abad = 0.0;
    CHK(taper_bbox<DIM>(c, nb, b, ldb, box, &bad));
    if (!same) CHK(taper_bbox<DIM>(c, na, a, lda, abox, &abad));
    if (bad + abad > 0.0)
        return fail(SMM_ERR_INVALID, "smm_taper_build: %.0f coordinates are not finite (NaN or inf)", bad + abad);
    const TaperGrid g = taper_grid(DIM, cutoff, box, box + 3, nb);
    const int ncells = g.nc[0] * g.nc[1] * g.nc[2];

    PoolBuf<int> cell_of(c), cnt(c), order_b(c), order_a(c), rowcnt(c);
    PoolBuf<int64_t> start(c), start_a(c), rowoff(c);
    PoolBuf<double> sorted_b(c);
    CHK(cell_of.alloc((size_t)std::max(na, nb)));
    CHK(cnt.alloc((size_t)ncells + 1));
    CHK(start.alloc((size_t)ncells + 1));
    CHK(order_b.alloc((size_t)nb));
    CHK(sorted_b.alloc((size_t)nb * DIM));
    CHK(taper_bin<DIM>(c, g, ncells, nb, b, ldb, cell_of, cnt, start, order_b, sorted_b));
    if (!same) {                                                     // queries in cell order too: a's own counting sort
        CHK(order_a.alloc((size_t)na));
        CHK(start_a.alloc((size_t)ncells + 1));
        CHK(taper_bin<DIM>(c, g, ncells, na, a, lda, cell_of, cnt, start_a, order_a, nullptr));
    }
    CHK(rowcnt.alloc((size_t)na + 1));
    CHK(rowoff.alloc((size_t)na + 1));

    TaperSearch S{};
    S.g = g; S.na = na; S.nb = nb; S.ncells = ncells; S.a = a; S.lda = lda;
    S.order_a = same ? order_b.p : order_a.p;
    S.start = start; S.sorted_b = sorted_b; S.order_b = order_b; S.rowcnt = rowcnt; S.err = c->d_err;
    const int64_t waves = (na + WAVE / TP_G - 1) / (WAVE / TP_G);
    const int sgrid = (int)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)c->n_cu * 32));
    LAUNCH(c, "smm_taper_count", (smm_taper_search<DIM, false>), sgrid, 256, 0, S);
    CHK(scan_launch<int>(c, na, rowcnt, rowoff));
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, rowoff.p + na, sizeof(nnz), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (nnz < 0 || nnz >= INT32_MAX)
        return fail(SMM_ERR_OVERFLOW, "smm_taper_build: %lld entries do not fit an operand (int32 row pointers, nnz < 2^31 - 1)", (long long)nnz);

    CsrPtr m = new_csr(c, na, nb, nnz);
    CHK(alloc_owned(c, m.get(), "the taper operand"));
    S.rowoff = rowoff; S.idx = m->own_idx;
    LAUNCH(c, "smm_taper_fill", (smm_taper_search<DIM, true>), sgrid, 256, 0, S);
    CHK(seg_sort(c, na, rowoff, m->own_idx));
    const int64_t vthreads = std::max<int64_t>(na * TP_G, na + 1);
    const int vgrid = (int)std::max<int64_t>(1, std::min<int64_t>((vthreads + 255) / 256, (int64_t)c->n_cu * 32));
    LAUNCH(c, "smm_taper_values", smm_taper_values<DIM>, vgrid, 256, 0, kind, g.half, na, a, lda, nb, b, ldb, (const int64_t *)rowoff,
           (const int *)m->own_idx.p, m->own_ptr.p, m->own_val.p, c->d_err);
    LAUNCH_CHECK();
    CHK(take_plan_error(c, "smm_taper_build"));              // (synchronises: the temporaries may go back to the pool)
    CHK(validate(c, m.get()));                               // (flags of the new operand: rows strictly ascending)
    *out = std::move(m);
    return SMM_OK;
}

// Everything smm_taper_build[_host] refuse before any launch.
static int taper_args(smm_ctx *c, int dim, int kind, double cutoff, int64_t na, const double *a, int64_t lda, int64_t nb,
                      const double *b, int64_t ldb, smm_csr **out, const char *where)
{
    if (!out) return fail(SMM_ERR_INVALID, "%s: out is NULL", where);
    *out = nullptr;
    if (!c) return fail(SMM_ERR_INVALID, "%s: ctx is NULL", where);
    if (dim < 1 || dim > 3) return fail(SMM_ERR_INVALID, "%s: dim must be 1, 2 or 3, got %d", where, dim);
    if (kind != SMM_TAPER_BOXCAR && kind != SMM_TAPER_GASPARI_COHN) return fail(SMM_ERR_INVALID, "%s: unknown taper kind %d", where, kind);
    if (!(cutoff > 0.0) || !std::isfinite(cutoff)) return fail(SMM_ERR_INVALID, "%s: cutoff must be finite and positive, got %g", where, cutoff);
    if (na < 0 || nb < 0 || na >= INT32_MAX || nb >= INT32_MAX)
        return fail(SMM_ERR_INVALID, "%s: point counts must be in [0, 2^31 - 1) (na %lld, nb %lld)", where, (long long)na, (long long)nb);
    if (lda < dim || ldb < dim) return fail(SMM_ERR_INVALID, "%s: need lda, ldb >= dim (dim %d, lda %lld, ldb %lld)", where, dim,
                                            (long long)lda, (long long)ldb);
    if ((na > 0 && !a) || (nb > 0 && !b)) return fail(SMM_ERR_INVALID, "%s: a or b is NULL", where);
    HIPCHK(hipSetDevice(c->device));
    return SMM_OK;
}

static int taper_dispatch(smm_ctx *c, int dim, int kind, double cutoff, int64_t na, const double *a, int64_t lda, int64_t nb,
                          const double *b, int64_t ldb, smm_csr **out)
{
    CsrPtr m;
    if (na == 0 || nb == 0) CHK(empty_csr(c, na, nb, &m));
    else if (dim == 1) CHK(taper_impl<1>(c, kind, cutoff, na, a, lda, nb, b, ldb, &m));
    else if (dim == 2) CHK(taper_impl<2>(c, kind, cutoff, na, a, lda, nb, b, ldb, &m));
    else CHK(taper_impl<3>(c, kind, cutoff, na, a, lda, nb, b, ldb, &m));
    *out = m.release();
    return SMM_OK;
}

extern "C" int smm_taper_build(smm_ctx *c, int dim, int kind, double cutoff, int64_t na, const double *d_a, int64_t lda, int64_t nb,
                               const double *d_b, int64_t ldb, smm_csr **out)
{
    CHK(taper_args(c, dim, kind, cutoff, na, d_a, lda, nb, d_b, ldb, out, "smm_taper_build"));
    CTX_LOCK(c);
    return taper_dispatch(c, dim, kind, cutoff, na, d_a, lda, nb, d_b, ldb, out);
}

// Same with host coordinates; b == a with ldb == lda and nb == na is uploaded once.
extern "C" int smm_taper_build_host(smm_ctx *c, int dim, int kind, double cutoff, int64_t na, const double *a, int64_t lda, int64_t nb,
                                    const double *b, int64_t ldb, smm_csr **out)
{
    CHK(taper_args(c, dim, kind, cutoff, na, a, lda, nb, b, ldb, out, "smm_taper_build_host"));
    CTX_LOCK(c);
    if (na == 0 || nb == 0) return taper_dispatch(c, dim, kind, cutoff, na, nullptr, dim, nb, nullptr, dim, out);
    const bool same = a == b && lda == ldb && na == nb;
    PoolBuf<double> da(c), db(c);
    CHK(da.alloc((size_t)na * dim));
    if (!same) CHK(db.alloc((size_t)nb * dim));
    CHK(upload_rows(c, da, a, na, dim, lda));
    if (!same) CHK(upload_rows(c, db, b, nb, dim, ldb));
    return taper_dispatch(c, dim, kind, cutoff, na, da, dim, nb, same ? (const double *)da : (const double *)db, dim, out);
}

// ------------------------------------------------------------------------------ observation operator from coordinates
// (kernels: smm_interp.hpp; contract: include/smm_hip.h)

// Everything smm_interp_build[_host] refuse before any launch; on success A holds the grid (not yet the device arrays).
static int interp_args(smm_ctx *c, int dim, const int64_t *axis_len, const double *axes, int method, int outside, int64_t n,
                       const double *pts, int64_t ldp, smm_csr **out, const char *where, InterpArgs *A)
{
    if (!out) return fail(SMM_ERR_INVALID, "%s: out is NULL", where);
    *out = nullptr;
    if (!c) return fail(SMM_ERR_INVALID, "%s: ctx is NULL", where);
    if (dim < 1 || dim > IP_MAX_DIM) return fail(SMM_ERR_INVALID, "%s: dim must be 1, 2, 3 or 4, got %d", where, dim);
    if (method != SMM_INTERP_LINEAR && method != SMM_INTERP_NEAREST) return fail(SMM_ERR_INVALID, "%s: unknown method %d", where, method);
    if (outside != SMM_INTERP_REJECT && outside != SMM_INTERP_CLAMP && outside != SMM_INTERP_ZERO)
        return fail(SMM_ERR_INVALID, "%s: unknown policy %d for points outside the grid", where, outside);
    if (!axis_len || !axes) return fail(SMM_ERR_INVALID, "%s: axis_len or axes is NULL", where);
    int64_t K = 1, nodes = 0;
    for (int t = 0; t < dim; ++t) {
        const int64_t m = axis_len[t];
        if (m < 2) return fail(SMM_ERR_INVALID, "%s: axis %d has %lld nodes, an axis needs at least 2", where, t, (long long)m);
        if (m >= INT32_MAX || K > (int64_t)(INT32_MAX - 1) / m)
            return fail(SMM_ERR_INVALID, "%s: the grid must have fewer than 2^31 - 1 nodes (an operand's columns)", where);
        const double *a = axes + nodes;
        for (int64_t j = 0; j < m; ++j) {
            if (!std::isfinite(a[j])) return fail(SMM_ERR_INVALID, "%s: node %lld of axis %d is not finite", where, (long long)j, t);
            if (j > 0 && !(a[j] > a[j - 1]))
                return fail(SMM_ERR_INVALID, "%s: axis %d is not strictly ascending at node %lld", where, t, (long long)j);
        }
        A->m[t] = (int)m; A->off[t] = (int)nodes; A->lo[t] = a[0]; A->hi[t] = a[m - 1];
        K *= m;
        nodes += m;
    }
    for (int t = dim - 1, s = 1; t >= 0; --t) { A->stride[t] = s; s *= A->m[t]; }          // (row-major, axis 0 slowest; ends at K)
    A->nodes = (int)nodes; A->K = (int)K; A->outside = outside;
    if (n < 0 || n >= INT32_MAX) return fail(SMM_ERR_INVALID, "%s: the number of points must be in [0, 2^31 - 1), got %lld", where, (long long)n);
    if (ldp < dim) return fail(SMM_ERR_INVALID, "%s: need ldp >= dim (dim %d, ldp %lld)", where, dim, (long long)ldp);
    if (n > 0 && !pts) return fail(SMM_ERR_INVALID, "%s: the points are NULL", where);
    const int64_t per_row = method == SMM_INTERP_NEAREST ? 1 : (int64_t)1 << dim;
    if (n > (int64_t)(INT32_MAX - 1) / per_row)
        return fail(SMM_ERR_OVERFLOW, "%s: %lld rows of %lld entries do not fit an operand (int32 row pointers, nnz <= 2^31 - 2)", where,
                    (long long)n, (long long)per_row);
    A->n = n; A->ldp = ldp; A->pts = pts;
    HIPCHK(hipSetDevice(c->device));
    return SMM_OK;
}

template <int DIM>
static int interp_impl(smm_ctx *c, InterpArgs A, const double *axes, int method, const char *where, CsrPtr *out)
{
    const int64_t per_row = method == SMM_INTERP_NEAREST ? 1 : (int64_t)1 << DIM;
    PoolBuf<double> d_axes(c);
    PoolBuf<unsigned long long> counts(c);
    CHK(d_axes.alloc((size_t)A.nodes));
    CHK(counts.alloc(2));
    HIPCHK(hipMemcpyAsync(d_axes, axes, (size_t)A.nodes * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), c->stream));
    A.axes = d_axes; A.counts = counts; A.err = c->d_err;
    const int cgrid = (int)std::min<int64_t>((A.n + 255) / 256, (int64_t)c->n_cu * 8);
    LAUNCH(c, "smm_interp_check", smm_interp_check<DIM>, cgrid, 256, 0, A);
    LAUNCH_CHECK();
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, counts, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h[0] > 0) return fail(SMM_ERR_INVALID, "%s: %llu coordinates are not finite (NaN or inf)", where, h[0]);
    if (h[1] > 0 && A.outside == SMM_INTERP_REJECT)
        return fail(SMM_ERR_INVALID, "%s: %llu points lie outside the grid (SMM_INTERP_CLAMP or SMM_INTERP_ZERO accept them)", where, h[1]);

    CsrPtr m = new_csr(c, A.n, A.K, A.n * per_row);
    CHK(alloc_owned(c, m.get(), "the interpolation operand"));
    A.optr = m->own_ptr; A.oidx = m->own_idx; A.oval = m->own_val;
    const int64_t chunks = (m->nnz + 3) / 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((std::max(chunks, A.n + 1) + 255) / 256, (int64_t)c->n_cu * 8));
    const bool stage = c->interp_stage && A.nodes <= IP_STAGE_NODES;
    const size_t lds = stage ? (size_t)A.nodes * sizeof(double) : 0;
    if (method == SMM_INTERP_NEAREST) {
        if (stage) LAUNCH(c, "smm_interp_fill", (smm_interp_fill<DIM, true, true>), grid, 256, lds, A);
        else LAUNCH(c, "smm_interp_fill", (smm_interp_fill<DIM, true, false>), grid, 256, lds, A);
    } else {
        if (stage) LAUNCH(c, "smm_interp_fill", (smm_interp_fill<DIM, false, true>), grid, 256, lds, A);
        else LAUNCH(c, "smm_interp_fill", (smm_interp_fill<DIM, false, false>), grid, 256, lds, A);
    }
    LAUNCH_CHECK();
    CHK(take_plan_error(c, where));                          // (synchronises: the temporaries may go back to the pool)
    // The flags smm_validate would find, by construction: ptr is i * per_row, and inside a row the columns ascend strictly
    // with the entry number (stride_t >= 2 stride_{t+1}); the fill has just reported that every column is inside [0, K).
    m->validated = true;
    m->vflags = 0;
    *out = std::move(m);
    return SMM_OK;
}

static int interp_dispatch(smm_ctx *c, int dim, const InterpArgs &A, const double *axes, int method, const char *where, smm_csr **out)
{
    CsrPtr m;
    if (A.n == 0) CHK(empty_csr(c, 0, A.K, &m));
    else if (dim == 1) CHK(interp_impl<1>(c, A, axes, method, where, &m));
    else if (dim == 2) CHK(interp_impl<2>(c, A, axes, method, where, &m));
    else if (dim == 3) CHK(interp_impl<3>(c, A, axes, method, where, &m));
    else CHK(interp_impl<4>(c, A, axes, method, where, &m));
    *out = m.release();
    return SMM_OK;
}

extern "C" int smm_interp_build(smm_ctx *c, int dim, const int64_t *axis_len, const double *axes, int method, int outside, int64_t n,
                                const double *d_pts, int64_t ldp, smm_csr **out)
{
    InterpArgs A{};
    CHK(interp_args(c, dim, axis_len, axes, method, outside, n, d_pts, ldp, out, "smm_interp_build", &A));
    CTX_LOCK(c);
    return interp_dispatch(c, dim, A, axes, method, "smm_interp_build", out);
}

// Same with the points in host memory.
extern "C" int smm_interp_build_host(smm_ctx *c, int dim, const int64_t *axis_len, const double *axes, int method, int outside, int64_t n,
                                     const double *pts, int64_t ldp, smm_csr **out)
{
    InterpArgs A{};
    CHK(interp_args(c, dim, axis_len, axes, method, outside, n, pts, ldp, out, "smm_interp_build_host", &A));
    CTX_LOCK(c);
    PoolBuf<double> dp(c);
    if (n > 0) {
        CHK(dp.alloc((size_t)n * dim));
        CHK(upload_rows(c, dp, pts, n, dim, ldp));
        A.pts = dp; A.ldp = dim;
    }
    return interp_dispatch(c, dim, A, axes, method, "smm_interp_build_host", out);
}

// ------------------------------------------------------------------------------ triple product, sparse output
// The result is held by the library as one CSR piece per row block (row blocking: nnz is known only at the end).
struct smm_result {
    smm_ctx *ctx = nullptr;
    int64_t rows = 0, cols = 0, nnz = 0;
    struct Piece { int64_t rows, nnz; int64_t *ptr; int *idx; double *val; };    // ptr: local, ptr[0] = 0
    std::vector<Piece> pieces;
};

extern "C" void smm_result_destroy(smm_result *r)
{
    if (!r) return;
    smm_ctx *c = r->ctx;
    {
        CTX_LOCK(c);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        for (auto &p : r->pieces) { pool_free(c, p.ptr); pool_free(c, p.idx); pool_free(c, p.val); }
    }
    delete r;
}
extern "C" int64_t smm_result_nnz(const smm_result *r) { return r ? r->nnz : -1; }
extern "C" int64_t smm_result_rows(const smm_result *r) { return r ? r->rows : -1; }

extern "C" int smm_ctx_tune_triple_sparse(smm_ctx *c, int64_t max_t_nnz)
{
    if (!c || max_t_nnz < 0) return fail(SMM_ERR_INVALID, "bad argument");
    CTX_LOCK(c);
    c->t3_max_t = max_t_nnz > 0 ? max_t_nnz : (int64_t)1 << 27;
    return SMM_OK;
}

// The pieces' row pointers, rebased and joined, into d_ptr (rows+1 int64); indices / values copied behind each other.
static int result_join(smm_ctx *c, const smm_result *r, int64_t *d_ptr, int32_t *d_idx, double *d_val)
{
    int64_t row = 0, base = 0;
    if (r->pieces.empty()) { HIPCHK(hipMemsetAsync(d_ptr, 0, ((size_t)r->rows + 1) * sizeof(int64_t), c->stream)); return SMM_OK; }
    for (const auto &p : r->pieces) {
        LAUNCH(c, "smm_triple_sparse_rebase", smm_triple_sparse_rebase, std::min<int64_t>((p.rows + 256) / 256, 4096), 256, 0, p.rows,
               (const int64_t *)p.ptr, base, d_ptr + row);
        LAUNCH_CHECK();
        if (p.nnz > 0) {
            HIPCHK(hipMemcpyAsync(d_idx + base, p.idx, (size_t)p.nnz * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_val + base, p.val, (size_t)p.nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        }
        row += p.rows; base += p.nnz;
    }
    return SMM_OK;
}

extern "C" int smm_result_copy_device(smm_ctx *c, smm_result *r, int64_t *d_indptr, int32_t *d_indices, double *d_data)
{
    if (!c || !r || r->ctx != c || !d_indptr) return fail(SMM_ERR_INVALID, "bad argument");
    if (r->nnz > 0 && (!d_indices || !d_data)) return fail(SMM_ERR_INVALID, "output arrays are NULL but nnz > 0");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    CHK(result_join(c, r, d_indptr, d_indices, d_data));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

extern "C" int smm_result_download(smm_ctx *c, smm_result *r, int64_t *indptr, void *indices, int index_bytes, double *data)
{
    if (!c || !r || r->ctx != c || !indptr) return fail(SMM_ERR_INVALID, "bad argument");
    if (index_bytes != 4 && index_bytes != 8) return fail(SMM_ERR_INVALID, "index_bytes must be 4 or 8");
    if (r->nnz > 0 && (!indices || !data)) return fail(SMM_ERR_INVALID, "output arrays are NULL but nnz > 0");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    indptr[0] = 0;
    int64_t row = 0, base = 0;
    std::vector<int64_t> tmp;
    for (const auto &p : r->pieces) {
        tmp.resize((size_t)p.rows + 1);
        CHK(download(c, tmp.data(), p.ptr, ((size_t)p.rows + 1) * sizeof(int64_t)));
        for (int64_t i = 1; i <= p.rows; ++i) indptr[row + i] = tmp[(size_t)i] + base;
        if (p.nnz > 0) {
            CHK(download(c, (char *)indices + (size_t)base * index_bytes, p.idx, (size_t)p.nnz * sizeof(int), index_bytes == 8));
            CHK(download(c, data + base, p.val, (size_t)p.nnz * sizeof(double)));
        }
        row += p.rows; base += p.nnz;
    }
    for (int64_t i = row + 1; i <= r->rows; ++i) indptr[i] = base;        // (no pieces: an empty result)
    return SMM_OK;
}

// ------------------------------------------------------------------------------ row classes (triple, masked, sparse x dense)
// Rows sorted into class lists on the device: list(c) holds count[c] rows of class c (at most 8 classes).  One pool
// block holds the lists and the counts; bin(lists, counts) launches the caller's binning kernels on the zeroed counts,
// and the counts come down with one synchronisation.
struct ClassLists {
    PoolBuf<int> buf;
    int64_t m = 0;
    int count[8] = {0};
    explicit ClassLists(smm_ctx *c) : buf(c) {}
    int *list(int cls) const { return buf + (size_t)cls * m; }
};
template <typename Bin> static int bin_rows(smm_ctx *c, int64_t m, int ncls, ClassLists &out, Bin bin)
{
    out.m = m;
    CHK(out.buf.alloc((size_t)ncls * m + 8));
    int *cnt = out.buf + (size_t)ncls * m;
    HIPCHK(hipMemsetAsync(cnt, 0, 8 * sizeof(int), c->stream));
    bin((int *)out.buf, cnt);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(out.count, cnt, sizeof(out.count), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}
// Workgroups of a global class, each with one zeroed row of row_bytes in HBM: at most one per CU and 256 MB of rows in
// flight.
static int64_t global_grid(const smm_ctx *c, int64_t nrows, int64_t row_bytes)
{
    return std::max<int64_t>(1, std::min<int64_t>({nrows, (int64_t)c->n_cu, ((int64_t)1 << 28) / std::max<int64_t>(row_bytes, 1)}));
}
// Opt-in of a kernel to `lds` bytes of dynamic LDS (the workgroup hash classes).
template <typename Kern> static int lds_opt_in(Kern kern, size_t lds)
{
    HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return SMM_OK;
}

// One row block [b0, b1) of H (global rows): T_b = H[b] * Q, the pattern of its rows of S (k >= i, ascending), their values.
// With a mask (canonical, n x n) the pattern is the mask's rows [b0, b1) filtered to k >= i: no H^T, no stage-2 symbolic
// phase, no sort.
static int triple_sparse_block(smm_ctx *c, smm_csr *h, smm_csr *q, smm_csr *ht, const smm_csr *mask, int flags, int64_t b0, int64_t b1,
                               smm_result::Piece *out)
{
    const int64_t nb = b1 - b0, n = h->rows, K = h->cols;
    const bool exact = (flags & SMM_EXACT) != 0;
    smm_csr hv = csr_row_view(h, b0, nb);
    PlanPtr p1, p2;
    CsrPtr tb;
    int64_t tnnz = 0, snnz = 0;
    PoolBuf<int64_t> tptr(c), sptr(c);
    PoolBuf<int> tidx(c), tptr32(c), mcnt(c), sidx(c);
    PoolBuf<double> tval(c), dense(c), sval(c);
    ClassLists bins(c);
    // stage 1: T_b, the engine's SpGEMM (first-touch rows, SMM_EXACT values in the reference's order)
    const bool zero = h->nnz == 0 || q->nnz == 0;       // (masked only: S is the mask's pattern filled with +0.0)
    smm_plan *pp = nullptr;
    if (!zero) { CHK(smm_spgemm_symbolic(c, &hv, q, flags & SMM_EXACT, 0, &pp, &tnnz)); p1.reset(pp); }
    CHK(tptr.alloc((size_t)nb + 1));
    CHK(tidx.alloc((size_t)std::max<int64_t>(tnnz, 1) + 2));
    CHK(tval.alloc((size_t)std::max<int64_t>(tnnz, 1)));
    if (!zero) CHK(smm_spgemm_numeric(c, p1.get(), tptr, tidx, tval));
    else HIPCHK(hipMemsetAsync(tptr, 0, ((size_t)nb + 1) * sizeof(int64_t), c->stream));
    p1.reset();
    if (tnnz >= INT32_MAX) return fail(SMM_ERR_INVALID, "sparse triple product: one row of T has >= 2^31 entries");
    if (mask) {
        // stage 2, pattern: the mask's rows filtered to k >= i (count, scan, copy)
        CHK(mcnt.alloc((size_t)2 * nb + 2));
        CHK(sptr.alloc((size_t)nb + 1));
        const int g = (int)std::min<int64_t>((nb + 255) / 256, 4096);
        LAUNCH(c, "smm_masked_tri_count", smm_masked_tri_count, g, 256, 0, (int)nb, b0, mask->ptr, mask->idx, mcnt, mcnt + nb + 1);
        CHK(scan_launch<int>(c, nb, mcnt, sptr));
        HIPCHK(hipMemcpyAsync(&snnz, sptr + nb, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        CHK(sidx.alloc((size_t)std::max<int64_t>(snnz, 1)));
        CHK(sval.alloc((size_t)std::max<int64_t>(snnz, 1)));
        if (snnz > 0)
            LAUNCH(c, "smm_masked_tri_copy", smm_masked_tri_copy, std::min<int64_t>((nb + 3) / 4, 16384), 256, 0, (int)nb,
                   (const int *)(mcnt + nb + 1), (const int *)mcnt, (const int64_t *)sptr, mask->idx, sidx);
        LAUNCH_CHECK();
    } else {
        // stage 2, pattern: T_b (int32 row pointer, borrowed) times H^T, i <= k
        CHK(tptr32.alloc((size_t)nb + 1));
        LAUNCH(c, "smm_triple_sparse_narrow", smm_triple_sparse_narrow, std::min<int64_t>((nb + 256) / 256, 4096), 256, 0, nb, (const int64_t *)tptr, tptr32);
        smm_csr *t = nullptr;
        CHK(smm_csr_from_device(c, nb, K, tnnz, tptr32, tidx, tval, &t));
        tb.reset(t);
        CHK(smm_spgemm_symbolic(c, tb.get(), ht, SMM_SYMMETRIC, b0, &pp, &snnz));
        p2.reset(pp);
        CHK(sptr.alloc((size_t)nb + 1));
        CHK(sidx.alloc((size_t)std::max<int64_t>(snnz, 1)));
        CHK(sval.alloc((size_t)std::max<int64_t>(snnz, 1)));
        CHK(smm_spgemm_numeric(c, p2.get(), sptr, sidx, sval));        // (its values are T * H^T in T's order: overwritten below)
        p2.reset();
        CHK(seg_sort(c, nb, sptr, sidx));
    }
    // stage 2, values: rows binned by the length of T_i
    if (snnz > 0) {
        CHK(bin_rows(c, nb, 3, bins, [&](int *lists, int *cnt) {
            LAUNCH(c, "smm_triple_sparse_bin", smm_triple_sparse_bin, std::min<int64_t>((nb + 255) / 256, 4096), 256, 0, (int)nb,
                   (const int64_t *)tptr, (const int64_t *)sptr, lists, cnt);
        }));
        const int *hc = bins.count;
        Triple3Args A{};
        A.m = (int)nb; A.row0 = b0;
        A.t_ptr = tptr; A.t_idx = tidx; A.t_val = tval;
        A.s_ptr = sptr; A.s_idx = sidx; A.s_val = sval;
        A.h_ptr = h->ptr; A.h_idx = h->idx; A.h_val = h->val; A.n = (int)n; A.K = (int)K;
        A.err = c->d_err;
        if (hc[0] > 0) {            // one wave per row, four rows per workgroup
            A.rowlist = bins.list(0); A.nrows = hc[0];
            const size_t lds = t3_hash_lds<WaveHash>();
            const int grid = (int)std::min<int64_t>((hc[0] + 3) / 4, (int64_t)c->n_cu * 16);
            if (exact) LAUNCH(c, "smm_triple_sparse_s2", (t3_hash_kernel<WaveHash, false>), grid, 256, lds, A);
            else       LAUNCH(c, "smm_triple_sparse_s2", (t3_hash_kernel<WaveHash, true>), grid, 256, lds, A);
            LAUNCH_CHECK();
        }
        if (hc[1] > 0) {            // one workgroup per row
            A.rowlist = bins.list(1); A.nrows = hc[1];
            const size_t lds = t3_hash_lds<WgHash>();
            auto kern = exact ? t3_hash_kernel<WgHash, false> : t3_hash_kernel<WgHash, true>;
            CHK(lds_opt_in(kern, lds));
            LAUNCH(c, "smm_triple_sparse_s2", kern, std::min<int64_t>(hc[1], (int64_t)c->n_cu), 256, lds, A);
            LAUNCH_CHECK();
        }
        if (hc[2] > 0) {            // a zeroed global row of K doubles per workgroup, a bounded number in flight
            A.rowlist = bins.list(2); A.nrows = hc[2];
            const int64_t grid = global_grid(c, hc[2], 8 * K);
            CHK(dense.alloc((size_t)grid * (size_t)K));
            HIPCHK(hipMemsetAsync(dense, 0, (size_t)grid * (size_t)K * sizeof(double), c->stream));
            A.dense = dense;
            if (exact) LAUNCH(c, "smm_triple_sparse_s2", smm_triple_sparse_s2_global<false>, grid, 256, 0, A);
            else       LAUNCH(c, "smm_triple_sparse_s2", smm_triple_sparse_s2_global<true>, grid, 256, 0, A);
            LAUNCH_CHECK();
        }
    }
    tb.reset();
    (void)hipStreamSynchronize(c->stream);      // the temporaries go back to the pool
    out->rows = nb; out->nnz = snnz; out->ptr = sptr.release(); out->idx = sidx.release(); out->val = sval.release();
    return SMM_OK;
}

// SMM_FULL_MATRIX: the pieces of r (rows [0,n), k >= i) joined into one CSR and mirrored on the device; r then holds the one
// full piece (rows stay ascending: mirrored part first, then k >= i).
static int result_mirror(smm_ctx *c, smm_result *r, int64_t n)
{
    PoolBuf<int64_t> up_ptr(c), fp_ptr(c);
    PoolBuf<int> up_idx(c), fp_idx(c);
    PoolBuf<double> up_val(c), fp_val(c);
    int64_t fnnz = 0;
    CHK(up_ptr.alloc((size_t)n + 1));
    CHK(up_idx.alloc((size_t)std::max<int64_t>(r->nnz, 1)));
    CHK(up_val.alloc((size_t)std::max<int64_t>(r->nnz, 1)));
    CHK(result_join(c, r, up_ptr, up_idx, up_val));
    CHK(fp_ptr.alloc((size_t)n + 1));
    CHK(smm_csr_mirror_symbolic(c, n, up_ptr, up_idx, fp_ptr, &fnnz));
    CHK(fp_idx.alloc((size_t)std::max<int64_t>(fnnz, 1)));
    CHK(fp_val.alloc((size_t)std::max<int64_t>(fnnz, 1)));
    CHK(smm_csr_mirror_fill(c, n, up_ptr, up_idx, up_val, fp_ptr, fp_idx, fp_val));
    (void)hipStreamSynchronize(c->stream);
    for (auto &p : r->pieces) { pool_free(c, p.ptr); pool_free(c, p.idx); pool_free(c, p.val); }
    up_ptr.reset(); up_idx.reset(); up_val.reset();
    r->pieces.assign(1, smm_result::Piece{n, fnnz, fp_ptr.release(), fp_idx.release(), fp_val.release()});
    r->nnz = fnnz;
    return SMM_OK;
}

// mask == nullptr: smm_triple_product_sparse; else smm_triple_product_sparse_masked (mask validated, canonical, n x n)
static int triple_sparse_impl(smm_ctx *c, smm_csr *h, smm_csr *q, const smm_csr *mask, int flags, int64_t row_begin, int64_t row_end,
                              smm_result **out)
{
    const int64_t n = h->rows, K = h->cols;
    if (q->cols > K) return fail(SMM_ERR_INVALID, "Q has more columns (%lld) than H (%lld)", (long long)q->cols, (long long)K);
    if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(SMM_ERR_INVALID, "bad row range");
    if (flags & SMM_MIRROR) return fail(SMM_ERR_INVALID, "smm_triple_product_sparse: SMM_MIRROR is not a flag of this call (SMM_FULL_MATRIX mirrors)");
    const bool full = (flags & SMM_FULL_MATRIX) != 0;
    if (full && (row_begin != 0 || row_end != n)) return fail(SMM_ERR_INVALID, "SMM_FULL_MATRIX needs the whole row range [0,n)");
    const int64_t nr = row_end - row_begin;
    std::unique_ptr<smm_result, Destroyer<smm_result_destroy>> r(new smm_result());
    r->ctx = c; r->rows = nr; r->cols = n;
    if (nr == 0 || (mask ? mask->nnz == 0 : (h->nnz == 0 || q->nnz == 0 || K == 0))) { *out = r.release(); return SMM_OK; }
    if (!mask && !h->tr) CHK(transpose_impl(c, h, &h->tr));
    // row blocks: products of H[i] * Q (an upper bound of nnz(T_i)) summed up to the budget, at least one row per block
    std::vector<int64_t> prod((size_t)nr);
    if (h->nnz > 0 && q->nnz > 0) {
        smm_csr hv = csr_row_view(h, row_begin, nr);
        CHK(smm_row_products(c, &hv, q, prod.data()));
    }
    int64_t b0 = row_begin;
    while (b0 < row_end) {
        int64_t b1 = b0, acc = 0;
        while (b1 < row_end && (b1 == b0 || acc + prod[(size_t)(b1 - row_begin)] <= c->t3_max_t)) acc += prod[(size_t)(b1++ - row_begin)];
        smm_result::Piece pc{0, 0, nullptr, nullptr, nullptr};
        CHK(triple_sparse_block(c, h, q, h->tr.get(), mask, flags, b0, b1, &pc));
        r->pieces.push_back(pc);
        r->nnz += pc.nnz;
        b0 = b1;
    }
    CHK(take_plan_error(c, "smm_triple_product_sparse"));
    if (full) CHK(result_mirror(c, r.get(), n));
    *out = r.release();
    return SMM_OK;
}

extern "C" int smm_triple_product_sparse(smm_ctx *c, smm_csr *h, smm_csr *q, int flags, int64_t row_begin, int64_t row_end, smm_result **out)
{
    if (!out) return fail(SMM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(check_pair(c, h, q));
    CHK(exact_guard(c, flags));
    return triple_sparse_impl(c, h, q, nullptr, flags, row_begin, row_end, out);
}

// A mask operand: same context, the expected shape, canonical (rows strictly ascending).
static int check_mask(smm_ctx *c, smm_csr *mask, int64_t rows, int64_t cols, const char *where)
{
    if (!mask) return fail(SMM_ERR_INVALID, "%s: mask is NULL", where);
    if (mask->ctx != c) return fail(SMM_ERR_INVALID, "%s: mask belongs to another context", where);
    if (mask->rows != rows || mask->cols != cols)
        return fail(SMM_ERR_INVALID, "%s: mask is %lld x %lld, expected %lld x %lld", where, (long long)mask->rows, (long long)mask->cols,
                    (long long)rows, (long long)cols);
    CHK(validate(c, mask));
    if (mask->vflags & (CSR_UNSORTED | CSR_HAS_EQUAL))
        return fail(SMM_ERR_INVALID, "%s: the mask is not canonical (rows must hold strictly ascending columns)", where);
    return SMM_OK;
}

extern "C" int smm_triple_product_sparse_masked(smm_ctx *c, smm_csr *h, smm_csr *q, smm_csr *mask, int flags, int64_t row_begin,
                                                int64_t row_end, smm_result **out)
{
    if (!out) return fail(SMM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(check_pair(c, h, q));
    CHK(check_mask(c, mask, h->rows, h->rows, "smm_triple_product_sparse_masked"));
    CHK(exact_guard(c, flags));
    return triple_sparse_impl(c, h, q, mask, flags, row_begin, row_end, out);
}

// ------------------------------------------------------------------------------ masked SpGEMM
extern "C" int smm_ctx_tune_masked(smm_ctx *c, int mode)
{
    if (!c || mode < 0 || mode > 2) return fail(SMM_ERR_INVALID, "bad argument (mode: 0 auto, 1 dot, 2 row)");
    CTX_LOCK(c);
    c->masked_mode = mode;
    return SMM_OK;
}

// nnz(mask) values of (A * B) on the mask's pattern into d_out (validated operands, canonical mask of A.rows x B.cols).
static int masked_impl(smm_ctx *c, smm_csr *a, smm_csr *b, smm_csr *mask, int flags, double *d_out)
{
    const int64_t m = a->rows, nm = mask->nnz;
    if (nm == 0) return SMM_OK;
    if (a->nnz == 0 || b->nnz == 0) {                 // the mask's pattern filled with +0.0
        HIPCHK(hipMemsetAsync(d_out, 0, (size_t)nm * sizeof(double), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    }
    const bool exact = (flags & SMM_EXACT) != 0;
    const bool a_canonical = !(a->vflags & (CSR_UNSORTED | CSR_HAS_EQUAL));
    const bool dot = a_canonical && c->masked_mode != 2;
    if (dot && !b->trv) CHK(transpose_impl(c, b, &b->trv));
    PoolBuf<int> cls(c), map(c);
    ClassLists bins(c);
    CHK(cls.alloc((size_t)m));
    CHK(bin_rows(c, m, MK_NCLS, bins, [&](int *lists, int *cnt) {
        LAUNCH(c, "smm_masked_cost", smm_masked_cost, std::min<int64_t>((m + 3) / 4, 16384), 256, 0, (int)m, mask->ptr, mask->idx, a->ptr,
               a->idx, b->ptr, (int)b->rows, dot ? (const int *)b->trv->ptr : nullptr, (int)b->cols, c->masked_mode, cls);
        LAUNCH(c, "smm_masked_bin", smm_masked_bin, std::min<int64_t>((m + 255) / 256, 4096), 256, 0, (int)m, (const int *)cls, lists, cnt);
    }));
    const int *hc = bins.count;
    MaskedArgs A{};
    A.m = (int)m;
    A.a_ptr = a->ptr; A.a_idx = a->idx; A.a_val = a->val; A.K = (int)a->cols;
    A.b_ptr = b->ptr; A.b_idx = b->idx; A.b_val = b->val; A.n = (int)b->cols;
    if (dot) { A.t_ptr = b->trv->ptr; A.t_idx = b->trv->idx; A.t_val = b->trv->val; }
    A.m_ptr = mask->ptr; A.m_idx = mask->idx; A.out = d_out;
    A.bdup = (b->vflags & (CSR_UNSORTED | CSR_HAS_EQUAL)) ? 1 : 0;
    A.err = c->d_err;
    // dot path: lanes per mask entry, the mean length of a row of B^T rounded up to a power of two in [4, 64]
    int dot_g = 4;
    while (dot_g < WAVE && (int64_t)dot_g * b->cols < b->nnz) dot_g *= 2;
    for (int cl = 0; cl < MK_NCLS; ++cl) {
        if (hc[cl] <= 0) continue;
        A.rowlist = bins.list(cl); A.nrows = hc[cl];
        if (cl == MK_DOT_WAVE) {               // one wave per row, four rows per workgroup
            const int64_t grid = std::min<int64_t>((hc[cl] + 3) / 4, (int64_t)c->n_cu * 16);
            LAUNCH(c, "smm_masked_dot", mk_dot_kernel<WaveHash>, grid, 256, mk_dot_lds<WaveHash>(), A, dot_g);
        } else if (cl == MK_DOT_WG) {          // one workgroup per row
            CHK(lds_opt_in(mk_dot_kernel<WgHash>, mk_dot_lds<WgHash>()));
            LAUNCH(c, "smm_masked_dot", mk_dot_kernel<WgHash>, std::min<int64_t>(hc[cl], (int64_t)c->n_cu * 2), 256, mk_dot_lds<WgHash>(), A, dot_g);
        } else if (cl == MK_ROW_WAVE) {
            const int64_t grid = std::min<int64_t>((hc[cl] + 3) / 4, (int64_t)c->n_cu * 16);
            if (exact) LAUNCH(c, "smm_masked_row", (mk_row_kernel<WaveHash, true>), grid, 256, mk_row_lds<WaveHash>(), A);
            else       LAUNCH(c, "smm_masked_row", (mk_row_kernel<WaveHash, false>), grid, 256, mk_row_lds<WaveHash>(), A);
        } else if (cl == MK_ROW_WG) {
            auto kern = exact ? mk_row_kernel<WgHash, true> : mk_row_kernel<WgHash, false>;
            CHK(lds_opt_in(kern, mk_row_lds<WgHash>()));
            LAUNCH(c, "smm_masked_row", kern, std::min<int64_t>(hc[cl], (int64_t)c->n_cu), 256, mk_row_lds<WgHash>(), A);
        } else {                               // MK_DOT_GLOBAL / MK_ROW_GLOBAL: one zeroed row of `width` ints per workgroup
            const int64_t width = cl == MK_DOT_GLOBAL ? a->cols : b->cols;
            const int64_t grid = global_grid(c, hc[cl], width * (int64_t)sizeof(int));
            CHK(map.alloc((size_t)grid * (size_t)width));      // (the previous class's map goes back to the pool first)
            HIPCHK(hipMemsetAsync(map, 0, (size_t)grid * (size_t)width * sizeof(int), c->stream));
            A.map = map;
            if (cl == MK_DOT_GLOBAL) {
                LAUNCH(c, "smm_masked_dot", smm_masked_dot_global, grid, 256, 0, A, dot_g);
            } else {
                if (exact) LAUNCH(c, "smm_masked_row", smm_masked_row_global<true>, grid, 256, 0, A);
                else       LAUNCH(c, "smm_masked_row", smm_masked_row_global<false>, grid, 256, 0, A);
            }
        }
        LAUNCH_CHECK();
    }
    (void)hipStreamSynchronize(c->stream);
    cls.reset(); bins.buf.reset(); map.reset();
    return take_plan_error(c, "smm_spgemm_masked");
}

static int masked_args(smm_ctx *c, smm_csr *a, smm_csr *b, smm_csr *mask, int flags)
{
    if (flags & ~SMM_EXACT) return fail(SMM_ERR_INVALID, "smm_spgemm_masked: only SMM_EXACT is a flag of this call");
    CHK(check_pair(c, a, b));
    CHK(check_mask(c, mask, a->rows, b->cols, "smm_spgemm_masked"));
    CHK(exact_guard(c, flags));
    return SMM_OK;
}

extern "C" int smm_spgemm_masked(smm_ctx *c, smm_csr *a, smm_csr *b, smm_csr *mask, int flags, double *d_c_data)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(masked_args(c, a, b, mask, flags));
    if (mask->nnz > 0 && !d_c_data) return fail(SMM_ERR_INVALID, "d_c_data is NULL but nnz(mask) > 0");
    return masked_impl(c, a, b, mask, flags, d_c_data);
}

extern "C" int smm_spgemm_masked_host(smm_ctx *c, smm_csr *a, smm_csr *b, smm_csr *mask, int flags, double *c_data)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(masked_args(c, a, b, mask, flags));
    if (mask->nnz == 0) return SMM_OK;
    if (!c_data) return fail(SMM_ERR_INVALID, "c_data is NULL but nnz(mask) > 0");
    PoolBuf<double> d(c);
    CHK(d.alloc((size_t)mask->nnz));
    CHK(masked_impl(c, a, b, mask, flags, d));
    CHK(download(c, c_data, d, (size_t)mask->nnz * sizeof(double)));
    (void)hipStreamSynchronize(c->stream);
    return SMM_OK;
}

// ------------------------------------------------------------------------------ sparse x dense: Y = op(A) * X
extern "C" int smm_ctx_tune_spmm(smm_ctx *c, int mode, int64_t apply_budget_bytes)
{
    if (!c || mode < 0 || mode > 3 || apply_budget_bytes < 0)
        return fail(SMM_ERR_INVALID, "bad argument (mode: 0 auto, 1 tiny, 2 group, 3 long; apply_budget_bytes >= 0)");
    CTX_LOCK(c);
    c->spmm_mode = mode;
    c->apply_budget = apply_budget_bytes > 0 ? apply_budget_bytes : (int64_t)1 << 30;
    return SMM_OK;
}

// op(A) as a CSR: A, or A^T -- the transpose cached on A's handle (built on first use, dropped by a value update).
static int spmm_op(smm_ctx *c, smm_csr *a, bool transpose, const smm_csr **out)
{
    if (transpose && !a->trv) CHK(transpose_impl(c, a, &a->trv));
    *out = transpose ? a->trv.get() : a;
    return SMM_OK;
}

// Y = op X on the context's stream (validated op; k, ldx, ldy checked by the caller).  Rows are binned by length and each
// class goes to its kernel (smm_spmm.hpp); every row of Y gets columns [0, k) written, nothing else.  In two halves: the
// rows of op binned for width k (one synchronisation for the class counts), and the class kernels launched from such
// lists without one.  A solver that applies one operator many times at one width bins it once.
static int spmm_bin(smm_ctx *c, const smm_csr *op, int64_t k, ClassLists &bins)
{
    const int64_t m = op->rows;
    if (m == 0 || k == 0) return SMM_OK;
    return bin_rows(c, m, SP_NCLS, bins, [&](int *lists, int *cnt) {
        LAUNCH(c, "smm_spmm_bin", smm_spmm_bin, std::min<int64_t>((m + 255) / 256, 4096), 256, 0, (int)m, op->ptr, k, c->spmm_mode, lists, cnt);
    });
}
static int spmm_launch(smm_ctx *c, const smm_csr *op, const ClassLists &bins, bool exact, int64_t k, const double *x, int64_t ldx, double *y,
                       int64_t ldy)
{
    const int64_t m = op->rows;
    if (m == 0 || k == 0) return SMM_OK;
    const int *hc = bins.count;
    SpmmArgs A{};
    A.m = (int)m; A.K = (int)op->cols; A.nnz = (int)op->nnz;
    A.ptr = op->ptr; A.idx = op->idx; A.val = op->val;
    A.k = k; A.ldx = ldx; A.ldy = ldy; A.x = x; A.y = y; A.err = c->d_err;
    // 16-byte loads and stores of X and Y where every lane's pair of columns is aligned
    const int vec = (k % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0) ? 2 : 1;
    int gk = 4;                                        // lanes per row of the group class: one per VEC columns, 4 .. 64
    while (gk < WAVE && (int64_t)gk * vec < k) gk *= 2;
    const int64_t cap = (int64_t)c->n_cu * 32;         // workgroups of the grid-stride kernels
    auto rows_grid = [&](int nrows, int rows_per_wave) {
        return std::max<int64_t>(1, std::min<int64_t>(((int64_t)nrows + 4 * rows_per_wave - 1) / (4 * rows_per_wave), cap));
    };
    for (int cl = 0; cl < SP_NCLS; ++cl) {
        if (hc[cl] <= 0) continue;
        A.rowlist = bins.list(cl); A.nrows = hc[cl];
        const bool split = cl == SP_LONG && !exact;    // (SMM_EXACT: one wave walks a long row in order)
        if (k == 1) {
            if (split) {
                LAUNCH(c, "smm_spmv_long", smm_spmv_long<SP_LONG_WAVES>, std::min<int64_t>(hc[cl], cap), SP_LONG_WAVES * WAVE, 0, A);
            } else if (cl == SP_TINY) {
                if (exact) LAUNCH(c, "smm_spmv_group", (smm_spmv_group<16, true>), rows_grid(hc[cl], 4), 256, 0, A);
                else       LAUNCH(c, "smm_spmv_group", (smm_spmv_group<16, false>), rows_grid(hc[cl], 4), 256, 0, A);
            } else {
                if (exact) LAUNCH(c, "smm_spmv_group", (smm_spmv_group<64, true>), rows_grid(hc[cl], 1), 256, 0, A);
                else       LAUNCH(c, "smm_spmv_group", (smm_spmv_group<64, false>), rows_grid(hc[cl], 1), 256, 0, A);
            }
        } else if (split) {
            const int64_t ntiles = (k + (int64_t)WAVE * vec - 1) / ((int64_t)WAVE * vec);
            if (ntiles > INT32_MAX) return fail(SMM_ERR_INVALID, "smm_spmm: k too large");
            const int64_t grid = std::min<int64_t>((int64_t)hc[cl] * ntiles, cap);
            if (vec == 2) LAUNCH(c, "smm_spmm_long", (smm_spmm_long<2, SP_LONG_WAVES>), grid, SP_LONG_WAVES * WAVE, 0, A, (int)ntiles);
            else          LAUNCH(c, "smm_spmm_long", (smm_spmm_long<1, SP_LONG_WAVES>), grid, SP_LONG_WAVES * WAVE, 0, A, (int)ntiles);
        } else {
            const int g = cl == SP_TINY ? 4 : (cl == SP_LONG ? WAVE : gk);
            const int64_t grid = rows_grid(hc[cl], WAVE / g);
#define SPMM_GROUP(G_, V_)                                                                                                    \
    if (g == G_ && vec == V_) {                                                                                               \
        if (exact) LAUNCH(c, "smm_spmm_group", (smm_spmm_group<G_, V_, true>), grid, 256, 0, A);                              \
        else       LAUNCH(c, "smm_spmm_group", (smm_spmm_group<G_, V_, false>), grid, 256, 0, A);                             \
    }
            SPMM_GROUP(4, 1) SPMM_GROUP(8, 1) SPMM_GROUP(16, 1) SPMM_GROUP(32, 1) SPMM_GROUP(64, 1)
            SPMM_GROUP(4, 2) SPMM_GROUP(8, 2) SPMM_GROUP(16, 2) SPMM_GROUP(32, 2) SPMM_GROUP(64, 2)
#undef SPMM_GROUP
        }
        LAUNCH_CHECK();
    }
    return SMM_OK;
}
// Both halves back to back.
static int spmm_impl(smm_ctx *c, const smm_csr *op, bool exact, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy)
{
    ClassLists bins(c);
    CHK(spmm_bin(c, op, k, bins));
    return spmm_launch(c, op, bins, exact, k, x, ldx, y, ldy);
}

// Bytes spanned by a row-major rows x k block with leading dimension ld (0 when empty).
static int64_t span_bytes(int64_t rows, int64_t k, int64_t ld)
{
    return (rows <= 0 || k <= 0) ? 0 : ((rows - 1) * ld + k) * (int64_t)sizeof(double);
}
static bool ranges_overlap(const void *p, int64_t pb, const void *q, int64_t qb)
{
    if (pb <= 0 || qb <= 0) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

// The one size check of a pair of row-major blocks: 0 <= k <= both leading dimensions, under the names the header gives them.
static int dense_dims(const char *where, int64_t k, int64_t ld_a, int64_t ld_b, const char *name_a = "ldx", const char *name_b = "ldy")
{
    if (k < 0 || ld_a < k || ld_b < k)
        return fail(SMM_ERR_INVALID, "%s: need 0 <= k <= %s, %s (k %lld, %s %lld, %s %lld)", where, name_a, name_b, (long long)k, name_a,
                    (long long)ld_a, name_b, (long long)ld_b);
    return SMM_OK;
}

constexpr bool ON_DEVICE = false, ON_HOST = true;               // where an entry's two blocks live: the `host` of what follows
// The two blocks of an entry, in (in_rows x k) and out (out_rows x k): present where they hold anything and, on the device,
// apart.  Host blocks of one height n (the triple apply, the solve) hold data both or neither, so for them this is
// span_bytes(n, k, max(ld_in, ld_out)) > 0 && (!in || !out).  out_always: a NULL out is refused even where it would hold
// nothing -- the rule of the _coef entries alone (include/smm_hip.h); the plain solves take one with k == 0.
static int blocks_check(const char *where, bool host, const double *in, int64_t in_rows, int64_t ld_in, const double *out, int64_t out_rows,
                        int64_t ld_out, int64_t k, const char *name_in, const char *name_out, bool out_always = false)
{
    const int64_t ib = span_bytes(in_rows, k, ld_in), ob = span_bytes(out_rows, k, ld_out);
    if ((ib > 0 && !in) || ((ob > 0 || out_always) && !out)) return fail(SMM_ERR_INVALID, "%s: %s or %s is NULL", where, name_in, name_out);
    if (!host && ranges_overlap(in, ib, out, ob))
        return fail(SMM_ERR_INVALID, "%s: the device ranges of %s and %s overlap", where, name_in, name_out);
    return SMM_OK;
}

// Host rows x k (leading dimension ld) <-> packed device rows x k.
static int upload_rows(smm_ctx *c, double *d, const double *h, int64_t rows, int64_t k, int64_t ld)
{
    if (rows <= 0 || k <= 0) return SMM_OK;
    if (ld == k) HIPCHK(hipMemcpyAsync(d, h, (size_t)(rows * k) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpy2DAsync(d, (size_t)k * sizeof(double), h, (size_t)ld * sizeof(double), (size_t)k * sizeof(double), (size_t)rows,
                                 hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}
static int download_rows(smm_ctx *c, double *h, const double *d, int64_t rows, int64_t k, int64_t ld)
{
    if (rows <= 0 || k <= 0) return SMM_OK;
    if (ld == k) return download(c, h, d, (size_t)(rows * k) * sizeof(double));
    HIPCHK(hipMemcpy2DAsync(h, (size_t)ld * sizeof(double), d, (size_t)k * sizeof(double), (size_t)k * sizeof(double), (size_t)rows,
                            hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}

// body(d_in, ld_in, d_out, ld_out) on an entry's checked blocks, then the error word of its kernels.  Device blocks go to body as
// they are.  Host blocks are staged through packed pool copies: an empty problem returns before anything is allocated; the
// input's copy is allocated first, then the output's, then whatever body takes.
template <typename Body>
static int blocks_run(smm_ctx *c, const char *where, bool host, const double *in, int64_t in_rows, int64_t ld_in, double *out, int64_t out_rows,
                      int64_t ld_out, int64_t k, Body body)
{
    if (!host) {
        CHK(body(in, ld_in, out, ld_out));
        return take_plan_error(c, where);
    }
    if (out_rows == 0 || k == 0) return SMM_OK;
    PoolBuf<double> d_in(c), d_out(c);
    CHK(d_in.alloc((size_t)std::max<int64_t>(in_rows * k, 1)));   // (op(A) without columns: in_rows 0; else in_rows * k as it is)
    CHK(d_out.alloc((size_t)(out_rows * k)));
    CHK(upload_rows(c, d_in, in, in_rows, k, ld_in));
    CHK(body(d_in, k, d_out, k));
    CHK(take_plan_error(c, where));
    return download_rows(c, out, d_out, out_rows, k, ld_out);
}

// smm_spmm[_host]: flags, operand and sizes, then Y = op(A) X on the device's or the host's blocks.
static int spmm_entry(smm_ctx *c, smm_csr *a, int flags, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy, bool host,
                      const char *where)
{
    if (flags & ~(SMM_EXACT | SMM_TRANSPOSE)) return fail(SMM_ERR_INVALID, "%s: only SMM_EXACT and SMM_TRANSPOSE are flags of this call", where);
    if (!a) return fail(SMM_ERR_INVALID, "%s: NULL operand", where);
    if (a->ctx != c) return fail(SMM_ERR_INVALID, "%s: operand belongs to another context", where);
    CHK(dense_dims(where, k, ldx, ldy));
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, a));
    const bool tr = (flags & SMM_TRANSPOSE) != 0, exact = (flags & SMM_EXACT) != 0;
    const int64_t m = tr ? a->cols : a->rows, kx = tr ? a->rows : a->cols;
    CHK(blocks_check(where, host, x, kx, ldx, y, m, ldy, k, "X", "Y"));
    if (m == 0 || k == 0) return SMM_OK;                          // (ahead of op(A): an empty product builds no transpose)
    const smm_csr *op = nullptr;
    CHK(spmm_op(c, a, tr, &op));
    return blocks_run(c, where, host, x, kx, ldx, y, m, ldy, k, [&](const double *dx, int64_t lx, double *dy, int64_t ly) {
        return spmm_impl(c, op, exact, k, dx, lx, dy, ly);
    });
}

extern "C" int smm_spmm(smm_ctx *c, smm_csr *a, int flags, int64_t k, const double *d_x, int64_t ldx, double *d_y, int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return spmm_entry(c, a, flags, k, d_x, ldx, d_y, ldy, ON_DEVICE, "smm_spmm");
}

extern "C" int smm_spmm_host(smm_ctx *c, smm_csr *a, int flags, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return spmm_entry(c, a, flags, k, x, ldx, y, ldy, ON_HOST, "smm_spmm_host");
}

// ------------------------------------------------------------------------------ Kronecker operand Q = D (x) E
// Kernels: smm_kron.hpp; the contract is in include/smm_hip.h.
static KronArgs kron_args(smm_ctx *c, const smm_csr *d, const smm_csr *e)
{
    KronArgs A{};
    A.p = (int)d->rows; A.pc = (int)d->cols; A.r = (int)e->rows; A.rc = (int)e->cols;
    A.nnz_d = (int)d->nnz; A.nnz_e = (int)e->nnz;
    A.dptr = d->ptr; A.didx = d->idx; A.dval = d->val;
    A.eptr = e->ptr; A.eidx = e->idx; A.eval = e->val;
    A.err = c->d_err;
    return A;
}

// The two factors of a call: present, of this context, validated, with a product whose dimensions fit an operand's.
static int kron_factors(smm_ctx *c, smm_csr *d, smm_csr *e, const char *where)
{
    if (!d || !e) return fail(SMM_ERR_INVALID, "%s: NULL factor", where);
    if (d->ctx != c || e->ctx != c) return fail(SMM_ERR_INVALID, "%s: operand belongs to another context", where);
    if (d->rows * e->rows >= INT32_MAX || d->cols * e->cols >= INT32_MAX)
        return fail(SMM_ERR_INVALID, "%s: D (x) E would be %lld x %lld, dimensions must be < 2^31 - 1", where,
                    (long long)(d->rows * e->rows), (long long)(d->cols * e->cols));
    return SMM_OK;
}

extern "C" int smm_kron_build(smm_ctx *c, smm_csr *d, smm_csr *e, smm_csr **out)
{
    if (!out) return fail(SMM_ERR_INVALID, "smm_kron_build: out is NULL");
    *out = nullptr;
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(kron_factors(c, d, e, "smm_kron_build"));
    const int64_t rows = d->rows * e->rows, cols = d->cols * e->cols;
    if (d->nnz > 0 && e->nnz > (int64_t)(INT32_MAX - 1) / d->nnz)
        return fail(SMM_ERR_OVERFLOW, "smm_kron_build: nnz(D) * nnz(E) = %lld * %lld entries do not fit an operand (int32 row pointers, "
                                      "nnz <= 2^31 - 2); use the factors through smm_kron_apply", (long long)d->nnz, (long long)e->nnz);
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, d));
    CHK(validate(c, e));
    CsrPtr m;
    if (d->nnz == 0 || e->nnz == 0) {
        CHK(empty_csr(c, rows, cols, &m));
        *out = m.release();
        return SMM_OK;
    }
    m = new_csr(c, rows, cols, d->nnz * e->nnz);
    CHK(alloc_owned(c, m.get(), "the Kronecker operand"));
    KronArgs A = kron_args(c, d, e);
    A.optr = m->own_ptr; A.oidx = m->own_idx; A.oval = m->own_val;
    const int64_t cap = (int64_t)c->n_cu * 64;
    if (m->nnz / rows < 128) {                                   // short rows: 16 lanes (64 entries a pass), four rows per wave
        LAUNCH(c, "smm_kron_fill", smm_kron_fill<16>, std::max<int64_t>(1, std::min<int64_t>((rows + 15) / 16, cap)), 256, 0, A);
    } else {
        LAUNCH(c, "smm_kron_fill", smm_kron_fill<64>, std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, cap)), 256, 0, A);
    }
    LAUNCH_CHECK();
    CHK(take_plan_error(c, "smm_kron_build"));
    CHK(validate(c, m.get()));                                   // (flags of the new operand: canonical iff both factors are)
    *out = m.release();
    return SMM_OK;
}

// Y = (D (x) E) X for one column block on the context's stream, through u ((pc * r) x k, packed): the E-step and the
// D-step, nothing binned, nothing synchronised.  Every element of Y's k columns is written.
static int kron_apply_launch(smm_ctx *c, const smm_csr *d, const smm_csr *e, bool exact, int64_t k, const double *x, int64_t ldx, double *u,
                             double *y, int64_t ldy)
{
    if (k == 0) return SMM_OK;
    KronArgs A = kron_args(c, d, e);
    A.k = k; A.ldx = ldx; A.ldy = ldy; A.x = x; A.u = u; A.y = y;
    const int64_t cap = (int64_t)c->n_cu * 32;
    if ((int64_t)A.pc * A.r > 0) {
        const int vec = (k % 2 == 0 && ldx % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)u % 16 == 0) ? 2 : 1;
        const int64_t w = (int64_t)A.pc * k;                     // virtual columns of a row of E
        const int g = w <= 4 * vec ? 4 : (w <= 16 * vec ? 16 : WAVE);
        const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(((int64_t)A.r + 4 * (WAVE / g) - 1) / (4 * (WAVE / g)), cap));
#define KRON_INNER(G_, V_)                                                                                                    \
    if (g == G_ && vec == V_) {                                                                                               \
        if (exact) LAUNCH(c, "smm_kron_inner", (smm_kron_inner<G_, V_, true>), grid, 256, 0, A);                              \
        else       LAUNCH(c, "smm_kron_inner", (smm_kron_inner<G_, V_, false>), grid, 256, 0, A);                             \
    }
        KRON_INNER(4, 1) KRON_INNER(16, 1) KRON_INNER(64, 1) KRON_INNER(4, 2) KRON_INNER(16, 2) KRON_INNER(64, 2)
#undef KRON_INNER
    }
    if ((int64_t)A.p * A.r > 0) {
        const int vec = (k % 2 == 0 && ldy % 2 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)u % 16 == 0) ? 2 : 1;
        const int64_t chunks = ((int64_t)A.r * k + 256 * vec - 1) / (256 * vec);
        const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)A.p * chunks, cap * 8));
        if (vec == 2) { if (exact) LAUNCH(c, "smm_kron_outer", (smm_kron_outer<2, true>), grid, 256, 0, A, chunks);
                        else       LAUNCH(c, "smm_kron_outer", (smm_kron_outer<2, false>), grid, 256, 0, A, chunks); }
        else          { if (exact) LAUNCH(c, "smm_kron_outer", (smm_kron_outer<1, true>), grid, 256, 0, A, chunks);
                        else       LAUNCH(c, "smm_kron_outer", (smm_kron_outer<1, false>), grid, 256, 0, A, chunks); }
    }
    LAUNCH_CHECK();
    return SMM_OK;
}

// Y = (D (x) E) X, X taken in column blocks whose U fits the context's apply budget (lanes own elements in both kernels,
// so the blocking changes no bit in either mode).
static int kron_apply_impl(smm_ctx *c, const smm_csr *d, const smm_csr *e, bool exact, int64_t k, const double *x, int64_t ldx, double *y,
                           int64_t ldy)
{
    const int64_t m = d->rows * e->rows, urows = d->cols * e->rows;
    if (m == 0 || k == 0) return SMM_OK;
    const int64_t kb = std::max<int64_t>(1, std::min<int64_t>(k, c->apply_budget / std::max<int64_t>(urows * (int64_t)sizeof(double), 1)));
    PoolBuf<double> u(c);
    CHK(u.alloc((size_t)std::max<int64_t>(urows * kb, 1)));
    for (int64_t j0 = 0; j0 < k; j0 += kb) {
        const int64_t b = std::min(kb, k - j0);
        CHK(kron_apply_launch(c, d, e, exact, b, x + j0, ldx, u, y + j0, ldy));
    }
    return SMM_OK;
}

// smm_kron_apply[_host]: flags, factors and sizes, then Y = (D (x) E) X on the device's or the host's blocks.
static int kron_apply_entry(smm_ctx *c, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy,
                            bool host, const char *where)
{
    if (flags & ~SMM_EXACT) return fail(SMM_ERR_INVALID, "%s: only SMM_EXACT is a flag of this call ((D (x) E)^T is D^T (x) E^T: pass "
                                                         "transposed factors)", where);
    CHK(kron_factors(c, d, e, where));
    CHK(dense_dims(where, k, ldx, ldy));
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, d));
    CHK(validate(c, e));
    const int64_t m = d->rows * e->rows, kx = d->cols * e->cols;
    CHK(blocks_check(where, host, x, kx, ldx, y, m, ldy, k, "X", "Y"));
    return blocks_run(c, where, host, x, kx, ldx, y, m, ldy, k, [&](const double *dx, int64_t lx, double *dy, int64_t ly) {
        return kron_apply_impl(c, d, e, (flags & SMM_EXACT) != 0, k, dx, lx, dy, ly);
    });
}

extern "C" int smm_kron_apply(smm_ctx *c, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *d_x, int64_t ldx, double *d_y,
                              int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return kron_apply_entry(c, d, e, flags, k, d_x, ldx, d_y, ldy, ON_DEVICE, "smm_kron_apply");
}

extern "C" int smm_kron_apply_host(smm_ctx *c, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *x, int64_t ldx, double *y,
                                   int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return kron_apply_entry(c, d, e, flags, k, x, ldx, y, ldy, ON_HOST, "smm_kron_apply_host");
}

// ------------------------------------------------------------------------------ masked products with Q = D (x) E
// Kernels: smm_kron_masked.hpp; the contract is in include/smm_hip.h.  Q, T = H Q and their transposes are never formed.
// What both entries ask of H (or A), the factors and the mask.  Everything that needs no launch comes first -- contexts, the
// factors' shapes, the mask's shape (mask_cols: n for the triple product, p' r' for A Q) --, then the operands are validated
// and the factors must be canonical.  check_mask, after this, validates the mask.
static int kron_masked_operands(smm_ctx *c, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *mask, bool square, const char *where)
{
    if (!h) return fail(SMM_ERR_INVALID, "%s: NULL operand", where);
    if (h->ctx != c) return fail(SMM_ERR_INVALID, "%s: operand belongs to another context", where);
    CHK(kron_factors(c, d, e, where));
    if (square && (d->rows != d->cols || e->rows != e->cols))
        return fail(SMM_ERR_INVALID, "%s: the factors must be square (D is %lld x %lld, E is %lld x %lld)", where, (long long)d->rows,
                    (long long)d->cols, (long long)e->rows, (long long)e->cols);
    if (d->rows * e->rows != h->cols)
        return fail(SMM_ERR_INVALID, "%s: D (x) E has %lld rows, the left operand %lld columns", where, (long long)(d->rows * e->rows),
                    (long long)h->cols);
    const int64_t mask_cols = square ? h->rows : d->cols * e->cols;
    if (!mask) return fail(SMM_ERR_INVALID, "%s: mask is NULL", where);
    if (mask->ctx != c) return fail(SMM_ERR_INVALID, "%s: mask belongs to another context", where);
    if (mask->rows != h->rows || mask->cols != mask_cols)
        return fail(SMM_ERR_INVALID, "%s: mask is %lld x %lld, expected %lld x %lld", where, (long long)mask->rows, (long long)mask->cols,
                    (long long)h->rows, (long long)mask_cols);
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, h));
    CHK(validate(c, d));
    CHK(validate(c, e));
    if ((d->vflags | e->vflags) & (CSR_UNSORTED | CSR_HAS_EQUAL))
        return fail(SMM_ERR_INVALID, "%s: a factor is not canonical (its rows must hold strictly ascending columns: the entries of D and E "
                                     "are searched in sorted rows; sum_duplicates() of a host copy makes one)", where);
    return SMM_OK;
}

template <typename PT>
static KronMaskedArgs<PT> kron_masked_args(smm_ctx *c, const smm_csr *h, const smm_csr *d, const smm_csr *e)
{
    KronMaskedArgs<PT> A{};
    A.h_ptr = h->ptr; A.h_idx = h->idx; A.h_val = h->val; A.n = (int)h->rows; A.K = (int)h->cols; A.nnz_h = (int)h->nnz;
    A.p = (int)d->rows; A.pc = (int)d->cols; A.r = (int)e->rows; A.rc = (int)e->cols;
    A.nnz_d = (int)d->nnz; A.nnz_e = (int)e->nnz;
    A.dptr = d->ptr; A.didx = d->idx; A.dval = d->val;
    A.eptr = e->ptr; A.eidx = e->idx; A.eval = e->val;
    A.err = c->d_err;
    return A;
}

// The values of a pattern (A.nb rows, A.s_ptr / s_idx / s_val set, at least one position, H and the factors with entries):
// the per-entry table of H, the rows binned by their lanes per position, one launch per class.
template <bool TRIPLE, typename PT>
static int kron_masked_values(smm_ctx *c, KronMaskedArgs<PT> A, bool exact, PoolBuf<int> &scratch, int64_t nnz_h)
{
    const int64_t nb = A.nb;
    PoolBuf<int> cls(c);
    ClassLists bins(c);
    CHK(scratch.alloc((size_t)6 * (size_t)nnz_h));
    A.h_rng = reinterpret_cast<int4 *>((int *)scratch);               // (pool blocks are 256-byte aligned)
    A.h_tj = reinterpret_cast<int2 *>((int *)scratch + 4 * (size_t)nnz_h);
    CHK(cls.alloc((size_t)nb));
    const int64_t cap = (int64_t)c->n_cu * 16;
    const bool dlds = (int64_t)A.p * A.pc <= KM_DLDS;      // D as a table in LDS when p p' fits, else bisected from L2
    LAUNCH(c, "smm_kron_masked_prep", smm_kron_masked_prep<PT>, std::max<int64_t>(1, std::min<int64_t>(((int64_t)A.n + 3) / 4, cap)), 256, 0, A);
    LAUNCH_CHECK();
    CHK(bin_rows(c, nb, MK_NCLS, bins, [&](int *lists, int *cnt) {
        LAUNCH(c, "smm_kron_masked_class", (smm_kron_masked_class<TRIPLE, PT>), std::min<int64_t>((nb + 3) / 4, 16384), 256, 0, A, (int *)cls);
        LAUNCH(c, "smm_masked_bin", smm_masked_bin, std::min<int64_t>((nb + 255) / 256, 4096), 256, 0, (int)nb, (const int *)cls, lists, cnt);
    }));
    for (int cl = 0; cl < 5; ++cl) {                   // G = 4 << cl lanes per position, one wave per pattern row
        if (bins.count[cl] <= 0) continue;
        A.rowlist = bins.list(cl); A.nrows = bins.count[cl];
        const int64_t grid = std::min<int64_t>(((int64_t)A.nrows + 3) / 4, cap);
        if constexpr (TRIPLE) {
            if (dlds) { if (exact) LAUNCH(c, "smm_kron_masked_triple", (smm_kron_masked_triple<true, true>), grid, 256, 0, A, 4 << cl);
                        else       LAUNCH(c, "smm_kron_masked_triple", (smm_kron_masked_triple<false, true>), grid, 256, 0, A, 4 << cl); }
            else      { if (exact) LAUNCH(c, "smm_kron_masked_triple", (smm_kron_masked_triple<true, false>), grid, 256, 0, A, 4 << cl);
                        else       LAUNCH(c, "smm_kron_masked_triple", (smm_kron_masked_triple<false, false>), grid, 256, 0, A, 4 << cl); }
        } else {
            if (dlds) { if (exact) LAUNCH(c, "smm_kron_masked_spgemm", (smm_kron_masked_spgemm<true, true>), grid, 256, 0, A, 4 << cl);
                        else       LAUNCH(c, "smm_kron_masked_spgemm", (smm_kron_masked_spgemm<false, true>), grid, 256, 0, A, 4 << cl); }
            else      { if (exact) LAUNCH(c, "smm_kron_masked_spgemm", (smm_kron_masked_spgemm<true, false>), grid, 256, 0, A, 4 << cl);
                        else       LAUNCH(c, "smm_kron_masked_spgemm", (smm_kron_masked_spgemm<false, false>), grid, 256, 0, A, 4 << cl); }
        }
        LAUNCH_CHECK();
    }
    (void)hipStreamSynchronize(c->stream);              // the temporaries go back to the pool
    return SMM_OK;
}

extern "C" int smm_triple_product_sparse_masked_kron(smm_ctx *c, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *mask, int flags,
                                                     int64_t row_begin, int64_t row_end, smm_result **out)
{
    static const char *where = "smm_triple_product_sparse_masked_kron";
    if (!out) return fail(SMM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(kron_masked_operands(c, h, d, e, mask, /*square=*/true, where));
    CHK(check_mask(c, mask, h->rows, h->rows, where));
    const int64_t n = h->rows;
    if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(SMM_ERR_INVALID, "bad row range");
    if (flags & SMM_MIRROR) return fail(SMM_ERR_INVALID, "%s: SMM_MIRROR is not a flag of this call (SMM_FULL_MATRIX mirrors)", where);
    const bool full = (flags & SMM_FULL_MATRIX) != 0;
    if (full && (row_begin != 0 || row_end != n)) return fail(SMM_ERR_INVALID, "SMM_FULL_MATRIX needs the whole row range [0,n)");
    CHK(exact_guard(c, flags));
    const int64_t nb = row_end - row_begin;
    std::unique_ptr<smm_result, Destroyer<smm_result_destroy>> r(new smm_result());
    r->ctx = c; r->rows = nb; r->cols = n;
    if (nb == 0 || mask->nnz == 0) { *out = r.release(); return SMM_OK; }
    // the pattern: the mask's rows [row_begin, row_end) filtered to k >= i (count, scan, copy), as the CSR form's stage 2
    int64_t snnz = 0;
    PoolBuf<int64_t> sptr(c);
    PoolBuf<int> mcnt(c), sidx(c), scratch(c);
    PoolBuf<double> sval(c);
    CHK(mcnt.alloc((size_t)2 * nb + 2));
    CHK(sptr.alloc((size_t)nb + 1));
    LAUNCH(c, "smm_masked_tri_count", smm_masked_tri_count, (int)std::min<int64_t>((nb + 255) / 256, 4096), 256, 0, (int)nb, row_begin,
           mask->ptr, mask->idx, mcnt, mcnt + nb + 1);
    CHK(scan_launch<int>(c, nb, mcnt, sptr));
    HIPCHK(hipMemcpyAsync(&snnz, sptr + nb, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    CHK(sidx.alloc((size_t)std::max<int64_t>(snnz, 1)));
    CHK(sval.alloc((size_t)std::max<int64_t>(snnz, 1)));
    if (snnz > 0) {
        LAUNCH(c, "smm_masked_tri_copy", smm_masked_tri_copy, std::min<int64_t>((nb + 3) / 4, 16384), 256, 0, (int)nb,
               (const int *)(mcnt + nb + 1), (const int *)mcnt, (const int64_t *)sptr, mask->idx, sidx);
        LAUNCH_CHECK();
        if (h->nnz == 0 || d->nnz == 0 || e->nnz == 0) {       // nothing reaches any position: +0.0
            HIPCHK(hipMemsetAsync(sval, 0, (size_t)snnz * sizeof(double), c->stream));
        } else {
            KronMaskedArgs<int64_t> A = kron_masked_args<int64_t>(c, h, d, e);
            A.nb = (int)nb; A.row0 = row_begin;
            A.s_ptr = sptr; A.s_idx = sidx; A.s_val = sval; A.cols = (int)n;
            CHK((kron_masked_values<true, int64_t>(c, A, (flags & SMM_EXACT) != 0, scratch, h->nnz)));
        }
    }
    (void)hipStreamSynchronize(c->stream);
    mcnt.reset(); scratch.reset();
    r->pieces.push_back(smm_result::Piece{nb, snnz, sptr.release(), sidx.release(), sval.release()});
    r->nnz = snnz;
    CHK(take_plan_error(c, where));
    if (full) CHK(result_mirror(c, r.get(), n));
    *out = r.release();
    return SMM_OK;
}

// nnz(mask) values of A * (D (x) E) on the mask's pattern into d_out (checked operands, canonical mask of A.rows x p' r').
static int masked_kron_impl(smm_ctx *c, smm_csr *a, smm_csr *d, smm_csr *e, smm_csr *mask, int flags, double *d_out)
{
    const int64_t nm = mask->nnz;
    if (nm == 0) return SMM_OK;
    if (a->nnz == 0 || d->nnz == 0 || e->nnz == 0) {     // the mask's pattern filled with +0.0
        HIPCHK(hipMemsetAsync(d_out, 0, (size_t)nm * sizeof(double), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    }
    PoolBuf<int> scratch(c);
    KronMaskedArgs<int> A = kron_masked_args<int>(c, a, d, e);
    A.nb = (int)a->rows; A.row0 = 0;
    A.s_ptr = mask->ptr; A.s_idx = mask->idx; A.s_val = d_out; A.cols = (int)mask->cols;
    CHK((kron_masked_values<false, int>(c, A, (flags & SMM_EXACT) != 0, scratch, a->nnz)));
    scratch.reset();
    return take_plan_error(c, "smm_spgemm_masked_kron");
}

static int masked_kron_args(smm_ctx *c, smm_csr *a, smm_csr *d, smm_csr *e, smm_csr *mask, int flags)
{
    static const char *where = "smm_spgemm_masked_kron";
    if (flags & ~SMM_EXACT) return fail(SMM_ERR_INVALID, "%s: only SMM_EXACT is a flag of this call", where);
    CHK(kron_masked_operands(c, a, d, e, mask, /*square=*/false, where));
    CHK(check_mask(c, mask, a->rows, d->cols * e->cols, where));
    CHK(exact_guard(c, flags));
    return SMM_OK;
}

extern "C" int smm_spgemm_masked_kron(smm_ctx *c, smm_csr *a, smm_csr *d, smm_csr *e, smm_csr *mask, int flags, double *d_c_data)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(masked_kron_args(c, a, d, e, mask, flags));
    if (mask->nnz > 0 && !d_c_data) return fail(SMM_ERR_INVALID, "d_c_data is NULL but nnz(mask) > 0");
    return masked_kron_impl(c, a, d, e, mask, flags, d_c_data);
}

extern "C" int smm_spgemm_masked_kron_host(smm_ctx *c, smm_csr *a, smm_csr *d, smm_csr *e, smm_csr *mask, int flags, double *c_data)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(masked_kron_args(c, a, d, e, mask, flags));
    if (mask->nnz == 0) return SMM_OK;
    if (!c_data) return fail(SMM_ERR_INVALID, "c_data is NULL but nnz(mask) > 0");
    PoolBuf<double> dv(c);
    CHK(dv.alloc((size_t)mask->nnz));
    CHK(masked_kron_impl(c, a, d, e, mask, flags, dv));
    CHK(download(c, c_data, dv, (size_t)mask->nnz * sizeof(double)));
    (void)hipStreamSynchronize(c->stream);
    return SMM_OK;
}

// The K x K operator in the middle of H Q H^T as the host code sees it: one CSR, or a pair of factors D (x) E (square, with
// p * r == K) that is applied without being formed.  Which of the two is said, not read off the pointers: a call may pass NULL.
struct QOp {
    smm_csr *q = nullptr, *d = nullptr, *e = nullptr;
    bool factors = false;
};
static QOp q_factors(smm_csr *d, smm_csr *e) { return QOp{nullptr, d, e, true}; }

// H and Q of a call: present, of this context, validated, Q square with as many rows as H has columns.
static int hq_args(smm_ctx *c, smm_csr *h, const QOp &q, const char *where)
{
    if (!q.factors) {
        CHK(check_pair(c, h, q.q));
        if (q.q->rows != q.q->cols)
            return fail(SMM_ERR_INVALID, "%s: Q must be square, got %lld x %lld", where, (long long)q.q->rows, (long long)q.q->cols);
        return SMM_OK;
    }
    smm_csr *d = q.d, *e = q.e;
    if (!c || !h) return fail(SMM_ERR_INVALID, "%s: NULL argument", where);
    if (h->ctx != c) return fail(SMM_ERR_INVALID, "%s: operand belongs to another context", where);
    CHK(kron_factors(c, d, e, where));
    if (d->rows != d->cols || e->rows != e->cols)
        return fail(SMM_ERR_INVALID, "%s: D and E must be square, got %lld x %lld and %lld x %lld", where, (long long)d->rows,
                    (long long)d->cols, (long long)e->rows, (long long)e->cols);
    if (d->rows * e->rows != h->cols)
        return fail(SMM_ERR_INVALID, "Matrix dimensions are incompatible for multiplication (%lld x %lld times (%lld * %lld) squared)",
                    (long long)h->rows, (long long)h->cols, (long long)d->rows, (long long)e->rows);
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, h));
    CHK(validate(c, d));
    CHK(validate(c, e));
    return SMM_OK;
}

// Y = H (Q (H^T X)): H^T X through H's cached transpose, two pool intermediates of K x kb (three when Q is a pair of factors:
// the U of its E-step), X taken in column blocks of kb columns so that they fit the context's apply budget (columns are
// independent: blocking changes no bit).
static int triple_apply_impl(smm_ctx *c, smm_csr *h, const QOp &q, bool exact, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy)
{
    const int64_t n = h->rows, K = h->cols;
    if (n == 0 || k == 0) return SMM_OK;
    const smm_csr *ht = nullptr;
    CHK(spmm_op(c, h, true, &ht));
    const int64_t nz = q.factors ? 3 : 2;
    const int64_t kb = std::max<int64_t>(1, std::min<int64_t>(k, c->apply_budget / std::max<int64_t>(nz * K * (int64_t)sizeof(double), 1)));
    PoolBuf<double> z1(c), z2(c), u(c);
    CHK(z1.alloc((size_t)std::max<int64_t>(K * kb, 1)));
    CHK(z2.alloc((size_t)std::max<int64_t>(K * kb, 1)));
    if (q.factors) CHK(u.alloc((size_t)std::max<int64_t>(K * kb, 1)));
    for (int64_t j0 = 0; j0 < k; j0 += kb) {
        const int64_t b = std::min(kb, k - j0);
        CHK(spmm_impl(c, ht, exact, b, x + j0, ldx, z1, b));      // Z1 = H^T X[:, j0 .. j0 + b)
        if (q.factors) CHK(kron_apply_launch(c, q.d, q.e, exact, b, z1, b, u, z2, b));
        else          CHK(spmm_impl(c, q.q, exact, b, z1, b, z2, b));             // Z2 = Q Z1
        CHK(spmm_impl(c, h, exact, b, z2, b, y + j0, ldy));       // Y[:, j0 .. j0 + b) = H Z2
    }
    return SMM_OK;
}

// smm_triple_apply[_kron][_host]: flags, operands and sizes, then Y = H Q H^T X on the device's or the host's blocks.
static int triple_apply_entry(smm_ctx *c, smm_csr *h, const QOp &q, int flags, int64_t k, const double *x, int64_t ldx, double *y, int64_t ldy,
                              bool host, const char *where)
{
    if (flags & ~SMM_EXACT) return fail(SMM_ERR_INVALID, "%s: only SMM_EXACT is a flag of this call", where);
    CHK(hq_args(c, h, q, where));
    CHK(dense_dims(where, k, ldx, ldy));
    const int64_t n = h->rows;
    CHK(blocks_check(where, host, x, n, ldx, y, n, ldy, k, "X", "Y"));
    return blocks_run(c, where, host, x, n, ldx, y, n, ldy, k, [&](const double *dx, int64_t lx, double *dy, int64_t ly) {
        return triple_apply_impl(c, h, q, (flags & SMM_EXACT) != 0, k, dx, lx, dy, ly);
    });
}

extern "C" int smm_triple_apply(smm_ctx *c, smm_csr *h, smm_csr *q, int flags, int64_t k, const double *d_x, int64_t ldx, double *d_y,
                                int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return triple_apply_entry(c, h, QOp{q}, flags, k, d_x, ldx, d_y, ldy, ON_DEVICE, "smm_triple_apply");
}

extern "C" int smm_triple_apply_host(smm_ctx *c, smm_csr *h, smm_csr *q, int flags, int64_t k, const double *x, int64_t ldx, double *y,
                                     int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return triple_apply_entry(c, h, QOp{q}, flags, k, x, ldx, y, ldy, ON_HOST, "smm_triple_apply_host");
}

extern "C" int smm_triple_apply_kron(smm_ctx *c, smm_csr *h, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *d_x, int64_t ldx,
                                     double *d_y, int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return triple_apply_entry(c, h, q_factors(d, e), flags, k, d_x, ldx, d_y, ldy, ON_DEVICE, "smm_triple_apply_kron");
}

extern "C" int smm_triple_apply_kron_host(smm_ctx *c, smm_csr *h, smm_csr *d, smm_csr *e, int flags, int64_t k, const double *x, int64_t ldx,
                                          double *y, int64_t ldy)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return triple_apply_entry(c, h, q_factors(d, e), flags, k, x, ldx, y, ldy, ON_HOST, "smm_triple_apply_kron_host");
}

// ------------------------------------------------------------------------------ sampled dense product (X Y^T on a pattern)
extern "C" int smm_ctx_tune_sddmm(smm_ctx *c, int mode)
{
    if (!c || mode < 0 || mode > 2) return fail(SMM_ERR_INVALID, "bad argument (mode: 0 auto, 1 interleaved entries, 2 runs of entries)");
    CTX_LOCK(c);
    c->sddmm_mode = mode;
    return SMM_OK;
}

// Arguments common to smm_sddmm[_host]: flags, sizes, the mask (any legal CSR of this context).
static int sddmm_args(smm_ctx *c, smm_csr *mask, int flags, int64_t k, int64_t ldx, int64_t ldy, const char *where)
{
    if (flags & ~(SMM_EXACT | SMM_SCALE_BY_MASK)) return fail(SMM_ERR_INVALID, "%s: only SMM_EXACT and SMM_SCALE_BY_MASK are flags of this call", where);
    if (!mask) return fail(SMM_ERR_INVALID, "%s: mask is NULL", where);
    if (mask->ctx != c) return fail(SMM_ERR_INVALID, "%s: mask belongs to another context", where);
    CHK(dense_dims(where, k, ldx, ldy));
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, mask));
    if ((flags & SMM_SCALE_BY_MASK) && mask->nnz > 0 && !mask->val) return fail(SMM_ERR_INVALID, "%s: SMM_SCALE_BY_MASK needs the mask's values", where);
    return SMM_OK;
}

// nnz(mask) values into d_out on the context's stream (validated mask with nnz > 0; sizes and buffers checked by the
// caller).  One launch: no pattern, no symbolic phase, no transpose, no allocation.
static int sddmm_impl(smm_ctx *c, const smm_csr *mask, int flags, int64_t k, const double *x, int64_t ldx, const double *y, int64_t ldy,
                      double *d_out)
{
    const bool exact = (flags & SMM_EXACT) != 0;
    SddmmArgs A{};
    A.m = (int)mask->rows; A.n = (int)mask->cols; A.nnz = (int)mask->nnz;
    A.ptr = mask->ptr; A.idx = mask->idx; A.w = mask->val;
    A.k = k; A.ldx = ldx; A.ldy = ldy; A.x = x; A.y = y; A.out = d_out;
    A.scale = (flags & SMM_SCALE_BY_MASK) ? 1 : 0;
    A.err = c->d_err;
    // 16-byte loads of X and Y where every lane's pair of elements is aligned (the rule of spmm_launch)
    const int vec = (k % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0) ? 2 : 1;
    int g = 4;                                         // lanes per entry: one per two elements, 4 .. 64 -- from k alone
    while (g < WAVE && (int64_t)g * 2 < k) g *= 2;
    const int gpw = WAVE / g;
    // runs of entries where the mask has enough of them to fill the device that way, else one entry per group and step
    const int64_t full = (int64_t)c->n_cu * 16 * gpw * SD_RUN;
    const int cls = c->sddmm_mode ? c->sddmm_mode : (mask->nnz >= full ? 2 : 1);
    A.run = cls == 2 ? SD_RUN : 1;
    const int64_t runs = (mask->nnz + A.run - 1) / A.run, waves = (runs + gpw - 1) / gpw;
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)c->n_cu * 16));
#define SDDMM_CASE(G_, V_)                                                                                                    \
    if (g == G_ && vec == V_) {                                                                                               \
        if (exact) LAUNCH(c, "smm_sddmm", (smm_sddmm<G_, V_, true>), grid, 256, 0, A);                                        \
        else       LAUNCH(c, "smm_sddmm", (smm_sddmm<G_, V_, false>), grid, 256, 0, A);                                       \
    }
    SDDMM_CASE(4, 1) SDDMM_CASE(8, 1) SDDMM_CASE(16, 1) SDDMM_CASE(32, 1) SDDMM_CASE(64, 1)
    SDDMM_CASE(4, 2) SDDMM_CASE(8, 2) SDDMM_CASE(16, 2) SDDMM_CASE(32, 2) SDDMM_CASE(64, 2)
#undef SDDMM_CASE
    LAUNCH_CHECK();
    return SMM_OK;
}

extern "C" int smm_sddmm(smm_ctx *c, smm_csr *mask, int flags, int64_t k, const double *d_x, int64_t ldx, const double *d_y, int64_t ldy,
                         double *d_c_data)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(sddmm_args(c, mask, flags, k, ldx, ldy, "smm_sddmm"));
    const int64_t xb = span_bytes(mask->rows, k, ldx), yb = span_bytes(mask->cols, k, ldy), cb = mask->nnz * (int64_t)sizeof(double);
    if ((xb > 0 && !d_x) || (yb > 0 && !d_y) || (cb > 0 && !d_c_data)) return fail(SMM_ERR_INVALID, "smm_sddmm: X, Y or the output is NULL");
    if (ranges_overlap(d_c_data, cb, d_x, xb) || ranges_overlap(d_c_data, cb, d_y, yb))
        return fail(SMM_ERR_INVALID, "smm_sddmm: the output's device range overlaps X or Y");
    if (mask->nnz == 0) return SMM_OK;
    CHK(sddmm_impl(c, mask, flags, k, d_x, ldx, d_y, ldy, d_c_data));
    return take_plan_error(c, "smm_sddmm");
}

// Same with host X, Y and output; y == x with ldy == ldx (a square mask) is uploaded once.
extern "C" int smm_sddmm_host(smm_ctx *c, smm_csr *mask, int flags, int64_t k, const double *x, int64_t ldx, const double *y, int64_t ldy,
                              double *c_data)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CHK(sddmm_args(c, mask, flags, k, ldx, ldy, "smm_sddmm_host"));
    const int64_t m = mask->rows, n = mask->cols;
    if ((span_bytes(m, k, ldx) > 0 && !x) || (span_bytes(n, k, ldy) > 0 && !y) || (mask->nnz > 0 && !c_data))
        return fail(SMM_ERR_INVALID, "smm_sddmm_host: X, Y or the output is NULL");
    if (mask->nnz == 0) return SMM_OK;
    const bool same = y == x && ldy == ldx && m == n;
    PoolBuf<double> dx(c), dy(c), dc(c);
    CHK(dx.alloc((size_t)std::max<int64_t>(m * k, 1)));
    if (!same) CHK(dy.alloc((size_t)std::max<int64_t>(n * k, 1)));
    CHK(dc.alloc((size_t)mask->nnz));
    CHK(upload_rows(c, dx, x, m, k, ldx));
    if (!same) CHK(upload_rows(c, dy, y, n, k, ldy));
    CHK(sddmm_impl(c, mask, flags, k, dx, k, same ? (const double *)dx : (const double *)dy, k, dc));
    CHK(take_plan_error(c, "smm_sddmm_host"));
    return download(c, c_data, dc, (size_t)mask->nnz * sizeof(double));
}

// ------------------------------------------------------------------------------ parametric covariance on a pattern
// (kernel: smm_cov.hpp; contract: include/smm_hip.h)

// Everything smm_cov_eval[_host] refuse before any launch; on success A holds the model, the lengths and the pattern.
static int cov_args(smm_ctx *c, smm_csr *pat, int flags, int model, int dim, const double *length, double variance, int wrt, int64_t na,
                    const double *a, int64_t lda, int64_t nb, const double *b, int64_t ldb, const double *val, const double *dval,
                    const char *where, CovArgs *A)
{
    if (flags & ~SMM_COV_SCALE_BY_PATTERN) return fail(SMM_ERR_INVALID, "%s: only SMM_COV_SCALE_BY_PATTERN is a flag of this call", where);
    if (!pat) return fail(SMM_ERR_INVALID, "%s: pattern is NULL", where);
    if (pat->ctx != c) return fail(SMM_ERR_INVALID, "%s: pattern belongs to another context", where);
    if (model < SMM_COV_SPHERICAL || model > SMM_COV_MATERN52) return fail(SMM_ERR_INVALID, "%s: unknown model %d", where, model);
    if (dim < 1 || dim > 3) return fail(SMM_ERR_INVALID, "%s: dim must be 1, 2 or 3, got %d", where, dim);
    if (!length) return fail(SMM_ERR_INVALID, "%s: length is NULL", where);
    for (int t = 0; t < dim; ++t)
        if (!(length[t] > 0.0) || !std::isfinite(length[t]))
            return fail(SMM_ERR_INVALID, "%s: length[%d] must be finite and positive, got %g", where, t, length[t]);
    if (!std::isfinite(variance)) return fail(SMM_ERR_INVALID, "%s: variance must be finite, got %g", where, variance);
    if (wrt != SMM_COV_WRT_NONE && wrt != SMM_COV_WRT_ALL && (wrt < 0 || wrt >= dim))
        return fail(SMM_ERR_INVALID, "%s: wrt must be SMM_COV_WRT_NONE, a coordinate 0 .. %d or SMM_COV_WRT_ALL, got %d", where, dim - 1, wrt);
    if (wrt == SMM_COV_WRT_ALL)
        for (int t = 1; t < dim; ++t)
            if (length[t] != length[0]) return fail(SMM_ERR_INVALID, "%s: SMM_COV_WRT_ALL needs one common length, got %g and %g", where, length[0], length[t]);
    if ((dval != nullptr) != (wrt != SMM_COV_WRT_NONE)) return fail(SMM_ERR_INVALID, "%s: dval and wrt go together (dval %s, wrt %d)", where, dval ? "given" : "NULL", wrt);
    if (!val && !dval) return fail(SMM_ERR_INVALID, "%s: val and dval are both NULL", where);
    if (lda < dim || ldb < dim) return fail(SMM_ERR_INVALID, "%s: need lda, ldb >= dim (dim %d, lda %lld, ldb %lld)", where, dim, (long long)lda, (long long)ldb);
    if ((na > 0 && !a) || (nb > 0 && !b)) return fail(SMM_ERR_INVALID, "%s: a or b is NULL", where);
    if (na != pat->rows || nb != pat->cols)
        return fail(SMM_ERR_INVALID, "%s: the pattern is %lld x %lld, the points are %lld and %lld", where, (long long)pat->rows, (long long)pat->cols,
                    (long long)na, (long long)nb);
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, pat));
    if ((flags & SMM_COV_SCALE_BY_PATTERN) && pat->nnz > 0 && !pat->val) return fail(SMM_ERR_INVALID, "%s: SMM_COV_SCALE_BY_PATTERN needs the pattern's values", where);
    *A = CovArgs{};
    A->m = (int)pat->rows; A->n = (int)pat->cols; A->nnz = (int)pat->nnz;
    A->ptr = pat->ptr; A->idx = pat->idx; A->w = pat->val;
    for (int t = 0; t < 3; ++t) A->len[t] = t < dim ? length[t] : 1.0;
    A->variance = variance; A->model = model; A->wrt = wrt;
    A->scale = (flags & SMM_COV_SCALE_BY_PATTERN) ? 1 : 0;
    A->err = c->d_err;
    return SMM_OK;
}

// One launch on the context's stream (nnz > 0; the device arrays set by the caller): no allocation, no synchronisation.
static int cov_launch(smm_ctx *c, int dim, const CovArgs &A)
{
    const int64_t waves = ((int64_t)A.nnz + CV_RUN - 1) / CV_RUN;
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)c->n_cu * 8));
    if (dim == 1) LAUNCH(c, "smm_cov_eval", smm_cov_eval<1>, grid, 256, 0, A);
    else if (dim == 2) LAUNCH(c, "smm_cov_eval", smm_cov_eval<2>, grid, 256, 0, A);
    else LAUNCH(c, "smm_cov_eval", smm_cov_eval<3>, grid, 256, 0, A);
    LAUNCH_CHECK();
    return SMM_OK;
}

extern "C" int smm_cov_eval(smm_ctx *c, smm_csr *pattern, int flags, int model, int dim, const double *length, double variance, int wrt,
                            int64_t na, const double *d_a, int64_t lda, int64_t nb, const double *d_b, int64_t ldb, double *d_val, double *d_dval)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CovArgs A;
    CHK(cov_args(c, pattern, flags, model, dim, length, variance, wrt, na, d_a, lda, nb, d_b, ldb, d_val, d_dval, "smm_cov_eval", &A));
    const int64_t ab = span_bytes(na, dim, lda), bb = span_bytes(nb, dim, ldb), ob = pattern->nnz * (int64_t)sizeof(double);
    for (const double *out : {(const double *)d_val, (const double *)d_dval})
        if (out && (ranges_overlap(out, ob, d_a, ab) || ranges_overlap(out, ob, d_b, bb)))
            return fail(SMM_ERR_INVALID, "smm_cov_eval: an output's device range overlaps the coordinates");
    if (d_val && d_dval && ranges_overlap(d_val, ob, d_dval, ob)) return fail(SMM_ERR_INVALID, "smm_cov_eval: val and dval overlap");
    if (pattern->nnz == 0) return SMM_OK;
    A.a = d_a; A.lda = lda; A.b = d_b; A.ldb = ldb; A.val = d_val; A.dval = d_dval;
    CHK(cov_launch(c, dim, A));
    return take_plan_error(c, "smm_cov_eval");
}

// Same with host coordinates and outputs; b == a with ldb == lda (a square pattern) is uploaded once.
extern "C" int smm_cov_eval_host(smm_ctx *c, smm_csr *pattern, int flags, int model, int dim, const double *length, double variance, int wrt,
                                 int64_t na, const double *a, int64_t lda, int64_t nb, const double *b, int64_t ldb, double *val, double *dval)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    CovArgs A;
    CHK(cov_args(c, pattern, flags, model, dim, length, variance, wrt, na, a, lda, nb, b, ldb, val, dval, "smm_cov_eval_host", &A));
    const int64_t nnz = pattern->nnz;
    if (nnz == 0) return SMM_OK;
    const bool same = a == b && lda == ldb && na == nb;
    PoolBuf<double> da(c), db(c), dv(c), dd(c);
    CHK(da.alloc((size_t)na * dim));
    if (!same) CHK(db.alloc((size_t)nb * dim));
    if (val) CHK(dv.alloc((size_t)nnz));
    if (dval) CHK(dd.alloc((size_t)nnz));
    CHK(upload_rows(c, da, a, na, dim, lda));
    if (!same) CHK(upload_rows(c, db, b, nb, dim, ldb));
    A.a = da; A.lda = dim; A.b = same ? (const double *)da : (const double *)db; A.ldb = dim; A.val = dv; A.dval = dd;
    CHK(cov_launch(c, dim, A));
    CHK(take_plan_error(c, "smm_cov_eval_host"));
    if (val) CHK(download(c, val, dv, (size_t)nnz * sizeof(double)));
    if (dval) CHK(download(c, dval, dd, (size_t)nnz * sizeof(double)));
    return SMM_OK;
}

// ------------------------------------------------------------------------------ empirical variogram on a pattern
// (kernels: smm_variogram.hpp; contract: include/smm_hip.h)

// Everything smm_variogram[_host] refuse before any launch or allocation; on success A holds the pattern, the bins and the sizes.
static int vg_args(smm_ctx *c, smm_csr *pat, int flags, int dim, const double *a, int64_t lda, int64_t k, const double *y, int64_t ldy,
                   int nb, const double *edges, const int64_t *count, const double *sum_h, const double *sum_sq, const char *where, VgArgs *A)
{
    if (flags & ~SMM_VG_ALL_ENTRIES) return fail(SMM_ERR_INVALID, "%s: only SMM_VG_ALL_ENTRIES is a flag of this call", where);
    if (!pat) return fail(SMM_ERR_INVALID, "%s: pattern is NULL", where);
    if (pat->ctx != c) return fail(SMM_ERR_INVALID, "%s: pattern belongs to another context", where);
    if (dim < 1 || dim > 3) return fail(SMM_ERR_INVALID, "%s: dim must be 1, 2 or 3, got %d", where, dim);
    if (nb < 1 || nb > SMM_VG_MAX_BINS) return fail(SMM_ERR_INVALID, "%s: nb must be 1 .. %d, got %d", where, (int)SMM_VG_MAX_BINS, nb);
    if (!edges || !count || !sum_h || !sum_sq) return fail(SMM_ERR_INVALID, "%s: edges, count, sum_h or sum_sq is NULL", where);
    for (int q = 0; q <= nb; ++q)
        if (!std::isfinite(edges[q])) return fail(SMM_ERR_INVALID, "%s: edges[%d] is not finite", where, q);
    if (edges[0] < 0.0) return fail(SMM_ERR_INVALID, "%s: edges[0] must be >= 0, got %g", where, edges[0]);
    for (int q = 1; q <= nb; ++q)
        if (!(edges[q - 1] < edges[q]))
            return fail(SMM_ERR_INVALID, "%s: edges must ascend strictly, got edges[%d] = %g, edges[%d] = %g", where, q - 1, edges[q - 1], q, edges[q]);
    if (pat->rows != pat->cols)
        return fail(SMM_ERR_INVALID, "%s: the pattern must be square, got %lld x %lld", where, (long long)pat->rows, (long long)pat->cols);
    if (k < 0 || lda < dim || ldy < k)
        return fail(SMM_ERR_INVALID, "%s: need k >= 0, lda >= dim, ldy >= k (dim %d, lda %lld, k %lld, ldy %lld)", where, dim, (long long)lda,
                    (long long)k, (long long)ldy);
    if (pat->rows > 0 && (!a || (k > 0 && !y))) return fail(SMM_ERR_INVALID, "%s: a or y is NULL", where);
    HIPCHK(hipSetDevice(c->device));
    CHK(validate(c, pat));
    *A = VgArgs{};
    A->n = (int)pat->rows; A->nnz = (int)pat->nnz; A->nb = nb;
    A->all = (flags & SMM_VG_ALL_ENTRIES) ? 1 : 0;
    A->ptr = pat->ptr; A->idx = pat->idx;
    A->k = k;
    for (int q = 0; q <= VG_MAX_BINS; ++q) A->edges[q] = q <= nb ? edges[q] : HUGE_VAL;
    A->err = c->d_err;
    return SMM_OK;
}

// The two launches on the context's stream and the three small downloads (nnz > 0; A.a, A.y and their leading dimensions
// set by the caller).  Pool blocks: the sums (results in front, then one partial per bin and workgroup), then the counts.
static int vg_run(smm_ctx *c, int dim, VgArgs &A, int64_t *count, double *sum_h, double *sum_sq, const char *where)
{
    const size_t nb = (size_t)A.nb, per = nb * (size_t)VG_GROUPS;
    PoolBuf<double> ds(c);
    PoolBuf<int64_t> dc(c);
    CHK(ds.alloc(2 * nb + 2 * per));
    CHK(dc.alloc(nb + per));
    double *out_h = ds, *out_s = ds + nb;
    int64_t *out_c = dc;
    A.part_h = ds + 2 * nb; A.part_s = A.part_h + per; A.part_c = dc + nb;
    if (dim == 1) LAUNCH(c, "smm_variogram_bins", smm_variogram_bins<1>, VG_GROUPS, VG_BLOCK, 0, A);
    else if (dim == 2) LAUNCH(c, "smm_variogram_bins", smm_variogram_bins<2>, VG_GROUPS, VG_BLOCK, 0, A);
    else LAUNCH(c, "smm_variogram_bins", smm_variogram_bins<3>, VG_GROUPS, VG_BLOCK, 0, A);
    LAUNCH_CHECK();
    LAUNCH(c, "smm_variogram_finish", smm_variogram_finish, 1, 1024, 0, A.nb, (const double *)A.part_h, (const double *)A.part_s,
           (const int64_t *)A.part_c, out_h, out_s, out_c);
    LAUNCH_CHECK();
    CHK(take_plan_error(c, where));
    CHK(download(c, sum_h, out_h, nb * sizeof(double)));
    CHK(download(c, sum_sq, out_s, nb * sizeof(double)));
    return download(c, count, out_c, nb * sizeof(int64_t));
}

static void vg_zero(int nb, int64_t *count, double *sum_h, double *sum_sq)
{
    for (int b = 0; b < nb; ++b) { count[b] = 0; sum_h[b] = 0.0; sum_sq[b] = 0.0; }
}

extern "C" int smm_variogram(smm_ctx *c, smm_csr *pattern, int flags, int dim, const double *d_a, int64_t lda, int64_t k, const double *d_y,
                             int64_t ldy, int nb, const double *edges, int64_t *count, double *sum_h, double *sum_sq)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    VgArgs A;
    CHK(vg_args(c, pattern, flags, dim, d_a, lda, k, d_y, ldy, nb, edges, count, sum_h, sum_sq, "smm_variogram", &A));
    if (pattern->nnz == 0) { vg_zero(nb, count, sum_h, sum_sq); return SMM_OK; }
    A.a = d_a; A.lda = lda; A.y = d_y; A.ldy = ldy;
    return vg_run(c, dim, A, count, sum_h, sum_sq, "smm_variogram");
}

extern "C" int smm_variogram_host(smm_ctx *c, smm_csr *pattern, int flags, int dim, const double *a, int64_t lda, int64_t k, const double *y,
                                  int64_t ldy, int nb, const double *edges, int64_t *count, double *sum_h, double *sum_sq)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    VgArgs A;
    CHK(vg_args(c, pattern, flags, dim, a, lda, k, y, ldy, nb, edges, count, sum_h, sum_sq, "smm_variogram_host", &A));
    if (pattern->nnz == 0) { vg_zero(nb, count, sum_h, sum_sq); return SMM_OK; }
    const int64_t n = pattern->rows;
    PoolBuf<double> da(c), dy(c);
    CHK(da.alloc((size_t)n * dim));
    CHK(dy.alloc((size_t)std::max<int64_t>(n * k, 1)));
    CHK(upload_rows(c, da, a, n, dim, lda));
    CHK(upload_rows(c, dy, y, n, k, ldy));
    A.a = da; A.lda = dim; A.y = dy; A.ldy = k;
    return vg_run(c, dim, A, count, sum_h, sum_sq, "smm_variogram_host");
}

// ------------------------------------------------------------------------------ CG on (H Q H^T + R) Z = D
// The pinned words and events through which the host follows the count of live columns (made on first use).
static int cg_host_words(smm_ctx *c)
{
    if (!c->cg_live) {
        if (hipHostMalloc((void **)&c->cg_live, 64, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            c->cg_live = nullptr;
            return fail(SMM_ERR_ALLOC, "smm_innovation_solve: hipHostMalloc of the live-column words failed");
        }
    }
    for (hipEvent_t &e : c->cg_ev)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return SMM_OK;
}

// One column block of the solve (smm_cg.hpp; the contract is in include/smm_hip.h).  b / x point at the block's first column.
// The host enqueues iteration it, then waits for the live count that iteration it - 1 left: the device always has one
// iteration queued, and at most one runs after the last column froze -- on frozen columns, which no kernel writes.
// hist (smm_innovation_solve_coef) or NULL: the block's two device histories (maxiter x k each) and the caller's host arrays,
// pointing at the block's first column, with their leading dimension.
struct CgHist { double *d_alpha, *d_beta, *alpha, *beta; int64_t ld; };
static int cg_block(smm_ctx *c, const smm_csr *ht, const QOp &q, const smm_csr *h, const smm_csr *r, bool exact, int64_t k,
                    const double *b, int64_t ldb, double *x, int64_t ldx, double tol, int64_t maxiter, double *rv, double *pv, double *wv,
                    double *rpv, double *z1, double *z2, double *zu, double *part, double *sc, int *iterations, int *status,
                    double *residual_sq, double *rhs_sq, const CgHist *hist)
{
    const int64_t n = h->rows;
    ClassLists bht(c), bq(c), bh(c), br(c);
    CHK(spmm_bin(c, ht, k, bht));
    if (!q.factors) CHK(spmm_bin(c, q.q, k, bq));                  // (the kernels of a pair of factors bin nothing)
    CHK(spmm_bin(c, h, k, bh));
    if (r) CHK(spmm_bin(c, r, k, br));
    int *st = reinterpret_cast<int *>(sc + CG_NSC * k);
    CgArgs A{};
    A.n = n; A.k = k; A.b = b; A.ldb = ldb; A.x = x; A.ldx = ldx;
    A.r = rv; A.p = pv; A.w = wv; A.rp = rpv; A.part = part; A.sc = sc; A.st = st;
    // 16-byte accesses where every thread's pair of columns is aligned in every vector (the pool's blocks are)
    const int vec = (k % 2 == 0 && ldb % 2 == 0 && ldx % 2 == 0 && (uintptr_t)b % 16 == 0 && (uintptr_t)x % 16 == 0) ? 2 : 1;
    const int64_t threads = (int64_t)CG_T * (k / vec);
    const int block = threads <= 16384 ? 64 : 256;            // (few columns: the T partials spread over more CUs)
    const int64_t grid = (threads + block - 1) / block;
    const double tol2 = tol * tol;
#define CG_LAUNCH(name, kern, ...)                                                                          \
    do {                                                                                                 \
        if (vec == 2) { if (exact) LAUNCH(c, name, (kern<2, true __VA_ARGS__>), grid, block, 0, A);      \
                        else       LAUNCH(c, name, (kern<2, false __VA_ARGS__>), grid, block, 0, A); }   \
        else          { if (exact) LAUNCH(c, name, (kern<1, true __VA_ARGS__>), grid, block, 0, A);      \
                        else       LAUNCH(c, name, (kern<1, false __VA_ARGS__>), grid, block, 0, A); }   \
    } while (0)
#define CG_COMMA ,
    HIPCHK(hipMemsetAsync(st + 3 * k, 0, sizeof(int), c->stream));
    if (hist) {                                                   // +0.0 wherever no coefficient is written
        HIPCHK(hipMemsetAsync(hist->d_alpha, 0, (size_t)(maxiter * k) * sizeof(double), c->stream));
        HIPCHK(hipMemsetAsync(hist->d_beta, 0, (size_t)(maxiter * k) * sizeof(double), c->stream));
    }
    double *const none = nullptr;
    CG_LAUNCH("smm_cg_init", smm_cg_init);
    LAUNCH(c, "smm_cg_finish", smm_cg_finish<0>, k, CG_FIN, 0, part, k, sc, st, tol2, 0, none);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(c->cg_live, st + 3 * k, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    bool live = c->cg_live[0] > 0;
    int64_t ran = 0;                                              // iterations enqueued
    for (int64_t it = 1; live && it <= maxiter; ++it) {
        ran = it;
        CHK(spmm_launch(c, ht, bht, exact, k, pv, k, z1, k));         // Z1 = H^T P
        if (q.factors) CHK(kron_apply_launch(c, q.d, q.e, exact, k, z1, k, zu, z2, k));
        else          CHK(spmm_launch(c, q.q, bq, exact, k, z1, k, z2, k));           // Z2 = Q Z1
        CHK(spmm_launch(c, h, bh, exact, k, z2, k, wv, k));           // W = H Z2
        if (r) {
            CHK(spmm_launch(c, r, br, exact, k, pv, k, rpv, k));      // R P, added to W on the way to dot(p, w)
            CG_LAUNCH("smm_cg_pw", smm_cg_pw, CG_COMMA true);
        } else {
            CG_LAUNCH("smm_cg_pw", smm_cg_pw, CG_COMMA false);
        }
        if (hist) LAUNCH(c, "smm_cg_finish", (smm_cg_finish<1, true>), k, CG_FIN, 0, part, k, sc, st, tol2, (int)it, hist->d_alpha);
        else      LAUNCH(c, "smm_cg_finish", smm_cg_finish<1>, k, CG_FIN, 0, part, k, sc, st, tol2, (int)it, none);
        CG_LAUNCH("smm_cg_update", smm_cg_update);
        if (hist) LAUNCH(c, "smm_cg_finish", (smm_cg_finish<2, true>), k, CG_FIN, 0, part, k, sc, st, tol2, (int)it, hist->d_beta);
        else      LAUNCH(c, "smm_cg_finish", smm_cg_finish<2>, k, CG_FIN, 0, part, k, sc, st, tol2, (int)it, none);
        CG_LAUNCH("smm_cg_direction", smm_cg_direction);
        LAUNCH_CHECK();
        const int slot = (int)(it & 1);
        HIPCHK(hipMemcpyAsync(c->cg_live + 8 * slot, st + 3 * k, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->cg_ev[slot], c->stream));
        if (it >= 2) {
            HIPCHK(hipEventSynchronize(c->cg_ev[slot ^ 1]));
            live = c->cg_live[8 * (slot ^ 1)] > 0;
        }
    }
#undef CG_COMMA
#undef CG_LAUNCH
    // the histories' rows that an iteration could have written (the rest are the caller's zeros), queued in front of the
    // scalars' download: its synchronisation serves all three copies
    if (hist && ran > 0) {
        const size_t row = (size_t)k * sizeof(double), pitch = (size_t)hist->ld * sizeof(double);
        if (hist->ld == k) {                                      // one block: the rows are contiguous on both sides
            HIPCHK(hipMemcpyAsync(hist->alpha, hist->d_alpha, row * (size_t)ran, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(hist->beta, hist->d_beta, row * (size_t)ran, hipMemcpyDeviceToHost, c->stream));
        } else {
            HIPCHK(hipMemcpy2DAsync(hist->alpha, pitch, hist->d_alpha, row, row, (size_t)ran, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpy2DAsync(hist->beta, pitch, hist->d_beta, row, row, (size_t)ran, hipMemcpyDeviceToHost, c->stream));
        }
    }
    // the block's scalars, as the device left them
    std::vector<double> hs((size_t)(CG_NSC * k + (3 * k + 2) / 2 + 1));
    CHK(download(c, hs.data(), sc, ((size_t)CG_NSC * k) * sizeof(double) + ((size_t)3 * k + 1) * sizeof(int)));
    const int *hst = reinterpret_cast<const int *>(hs.data() + CG_NSC * k);
    for (int64_t j = 0; j < k; ++j) {
        status[j] = hst[j]; iterations[j] = hst[k + j];
        residual_sq[j] = hs[(size_t)(CG_RES * k + j)]; rhs_sq[j] = hs[(size_t)(CG_RHS * k + j)];
    }
    return SMM_OK;
}

// Vectors of one column block: r, p, w, R p (n x kb), the two intermediates (K x kb; three for a pair of factors), the dot
// partials and the scalars.
static int innovation_impl(smm_ctx *c, smm_csr *h, const QOp &q, smm_csr *r, bool exact, int64_t k, const double *b, int64_t ldb, double *x,
                           int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status, double *residual_sq, double *rhs_sq,
                           double *alpha = nullptr, double *beta = nullptr)
{
    const int64_t n = h->rows, K = h->cols;
    if (alpha) {                                                  // maxiter x k each: +0.0 wherever no coefficient lands
        memset(alpha, 0, (size_t)(maxiter * k) * sizeof(double));
        memset(beta, 0, (size_t)(maxiter * k) * sizeof(double));
    }
    if (n == 0 || k == 0) return SMM_OK;
    const smm_csr *ht = nullptr;
    CHK(spmm_op(c, h, true, &ht));
    CHK(cg_host_words(c));
    const int64_t per_col = (5 * n + (q.factors ? 3 : 2) * K) * (int64_t)sizeof(double);
    int64_t kb = std::max<int64_t>(1, std::min<int64_t>(k, c->apply_budget / std::max<int64_t>(per_col, 1)));
    const int64_t nblocks = (k + kb - 1) / kb, even = (k + nblocks - 1) / nblocks;      // blocks of one size (64 = 32 + 32, not 44 + 20),
    kb = (even % 2 && even < kb) ? even + 1 : even;                                      // of an even width where the budget allows
    PoolBuf<double> rv(c), pv(c), wv(c), rpv(c), z1(c), z2(c), zu(c), part(c), sc(c), ha(c), hb(c);
    CHK(rv.alloc((size_t)(n * kb)));
    CHK(pv.alloc((size_t)(n * kb)));
    CHK(wv.alloc((size_t)(n * kb)));
    if (r) CHK(rpv.alloc((size_t)(n * kb)));
    CHK(z1.alloc((size_t)std::max<int64_t>(K * kb, 1)));
    CHK(z2.alloc((size_t)std::max<int64_t>(K * kb, 1)));
    if (q.factors) CHK(zu.alloc((size_t)std::max<int64_t>(K * kb, 1)));
    CHK(part.alloc((size_t)CG_T * kb));
    CHK(sc.alloc((size_t)(CG_NSC * kb + (3 * kb + 2) / 2 + 1)));
    if (alpha) {
        CHK(ha.alloc((size_t)(maxiter * kb)));
        CHK(hb.alloc((size_t)(maxiter * kb)));
    }
    for (int64_t j0 = 0; j0 < k; j0 += kb) {
        const int64_t w = std::min(kb, k - j0);
        const CgHist hist{ha, hb, alpha ? alpha + j0 : nullptr, beta ? beta + j0 : nullptr, k};
        CHK(cg_block(c, ht, q, h, r, exact, w, b + j0, ldb, x + j0, ldx, tol, maxiter, rv, pv, wv, rpv, z1, z2, zu, part, sc, iterations + j0,
                     status + j0, residual_sq + j0, rhs_sq + j0, alpha ? &hist : nullptr));
    }
    return SMM_OK;
}

// What every solve asks of its arguments; Q as one CSR or as its factors (applied through smm_kron.hpp, never formed).
static int innovation_args(smm_ctx *c, smm_csr *h, const QOp &q, smm_csr *r, int flags, int64_t k, int64_t ldb, int64_t ldx, double tol,
                           int64_t maxiter, const int *iterations, const int *status, const double *residual_sq, const double *rhs_sq,
                           const char *where)
{
    if (flags & ~SMM_EXACT) return fail(SMM_ERR_INVALID, "%s: only SMM_EXACT is a flag of this call", where);
    CHK(hq_args(c, h, q, where));
    if (r) {
        if (r->ctx != c) return fail(SMM_ERR_INVALID, "%s: operand belongs to another context", where);
        if (r->rows != h->rows || r->cols != h->rows)
            return fail(SMM_ERR_INVALID, "%s: R must be %lld x %lld, got %lld x %lld", where, (long long)h->rows, (long long)h->rows,
                        (long long)r->rows, (long long)r->cols);
        CHK(validate(c, r));
    }
    CHK(dense_dims(where, k, ldb, ldx, "ldb", "ldx"));
    if (!(tol > 0.0) || !std::isfinite(tol)) return fail(SMM_ERR_INVALID, "%s: tol must be a finite positive number", where);
    if (maxiter < 0 || maxiter > INT32_MAX) return fail(SMM_ERR_INVALID, "%s: need 0 <= maxiter < 2^31", where);
    if (k > 0 && (!iterations || !status || !residual_sq || !rhs_sq)) return fail(SMM_ERR_INVALID, "%s: a per-column output is NULL", where);
    return SMM_OK;
}

// What the recording entries ask beyond their plain counterparts: the histories are sized by maxiter.
static int coef_args(int64_t k, int64_t maxiter, const double *alpha, const double *beta, const char *where)
{
    if (maxiter < 1 || maxiter > 65536) return fail(SMM_ERR_INVALID, "%s: need 1 <= maxiter <= 65536 (the histories are maxiter x k), got %lld",
                                                    where, (long long)maxiter);
    if (k > 0 && (!alpha || !beta)) return fail(SMM_ERR_INVALID, "%s: alpha or beta is NULL", where);
    return SMM_OK;
}

// The per-column outputs of a solve, and the two histories of a recording one.
struct SolveOut { int *iterations, *status; double *residual_sq, *rhs_sq, *alpha = nullptr, *beta = nullptr; };

// smm_innovation_solve[_kron][_host] and, with coef (device blocks only), smm_innovation_solve_coef[_kron]: arguments, then the
// solve on the device's or the host's blocks.  Everything is checked, and every operand validated, ahead of the first
// allocation, whatever k is; innovation_impl zeroes the histories ahead of its own return for an empty problem.
static int innovation_entry(smm_ctx *c, smm_csr *h, const QOp &q, smm_csr *r, int flags, int64_t k, const double *b, int64_t ldb, double *x,
                            int64_t ldx, double tol, int64_t maxiter, const SolveOut &o, bool host, const char *where, bool coef = false)
{
    CHK(innovation_args(c, h, q, r, flags, k, ldb, ldx, tol, maxiter, o.iterations, o.status, o.residual_sq, o.rhs_sq, where));
    if (coef) CHK(coef_args(k, maxiter, o.alpha, o.beta, where));
    const int64_t n = h->rows;
    CHK(blocks_check(where, host, b, n, ldb, x, n, ldx, k, "B", "X", /*out_always=*/coef));
    return blocks_run(c, where, host, b, n, ldb, x, n, ldx, k, [&](const double *db, int64_t lb, double *dx, int64_t lx) {
        return innovation_impl(c, h, q, r, (flags & SMM_EXACT) != 0, k, db, lb, dx, lx, tol, maxiter, o.iterations, o.status, o.residual_sq,
                               o.rhs_sq, k > 0 ? o.alpha : nullptr, k > 0 ? o.beta : nullptr);
    });
}

extern "C" int smm_innovation_solve(smm_ctx *c, smm_csr *h, smm_csr *q, smm_csr *r, int flags, int64_t k, const double *d_b, int64_t ldb,
                                    double *d_x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status, double *residual_sq,
                                    double *rhs_sq)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return innovation_entry(c, h, QOp{q}, r, flags, k, d_b, ldb, d_x, ldx, tol, maxiter, {iterations, status, residual_sq, rhs_sq}, ON_DEVICE,
                            "smm_innovation_solve");
}

extern "C" int smm_innovation_solve_host(smm_ctx *c, smm_csr *h, smm_csr *q, smm_csr *r, int flags, int64_t k, const double *b, int64_t ldb,
                                         double *x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                                         double *residual_sq, double *rhs_sq)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return innovation_entry(c, h, QOp{q}, r, flags, k, b, ldb, x, ldx, tol, maxiter, {iterations, status, residual_sq, rhs_sq}, ON_HOST,
                            "smm_innovation_solve_host");
}

extern "C" int smm_innovation_solve_kron(smm_ctx *c, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *r, int flags, int64_t k, const double *d_b,
                                         int64_t ldb, double *d_x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                                         double *residual_sq, double *rhs_sq)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return innovation_entry(c, h, q_factors(d, e), r, flags, k, d_b, ldb, d_x, ldx, tol, maxiter, {iterations, status, residual_sq, rhs_sq},
                            ON_DEVICE, "smm_innovation_solve_kron");
}

extern "C" int smm_innovation_solve_kron_host(smm_ctx *c, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *r, int flags, int64_t k, const double *b,
                                              int64_t ldb, double *x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                                              double *residual_sq, double *rhs_sq)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return innovation_entry(c, h, q_factors(d, e), r, flags, k, b, ldb, x, ldx, tol, maxiter, {iterations, status, residual_sq, rhs_sq}, ON_HOST,
                            "smm_innovation_solve_kron_host");
}

// ------------------------------------------------------------------------------ probes and recorded CG coefficients (SLQ)
extern "C" int smm_probe_fill(smm_ctx *c, int64_t n, int64_t k, uint64_t seed, double *d_x, int64_t ldx)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    if (n < 0 || k < 0 || ldx < k) return fail(SMM_ERR_INVALID, "smm_probe_fill: need n >= 0 and 0 <= k <= ldx (n %lld, k %lld, ldx %lld)",
                                               (long long)n, (long long)k, (long long)ldx);
    if (n == 0 || k == 0) return SMM_OK;
    if (!d_x) return fail(SMM_ERR_INVALID, "smm_probe_fill: X is NULL");
    if (n > INT64_MAX / ldx) return fail(SMM_ERR_INVALID, "smm_probe_fill: n * ldx does not fit 64 bits");
    HIPCHK(hipSetDevice(c->device));
    // 16-byte stores where every thread's pair of columns is aligned (the rule of cg_block)
    const int vec = (k % 2 == 0 && ldx % 2 == 0 && (uintptr_t)d_x % 16 == 0) ? 2 : 1;
    const int64_t total = n * (k / vec);
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)c->n_cu * 32));
    if (vec == 2) LAUNCH(c, "smm_probe_fill", smm_probe_fill_k<2>, grid, 256, 0, n, k, (unsigned long long)seed, d_x, ldx);
    else          LAUNCH(c, "smm_probe_fill", smm_probe_fill_k<1>, grid, 256, 0, n, k, (unsigned long long)seed, d_x, ldx);
    LAUNCH_CHECK();
    return SMM_OK;
}

extern "C" int smm_innovation_solve_coef(smm_ctx *c, smm_csr *h, smm_csr *q, smm_csr *r, int flags, int64_t k, const double *d_b, int64_t ldb,
                                         double *d_x, int64_t ldx, double tol, int64_t maxiter, int *iterations, int *status,
                                         double *residual_sq, double *rhs_sq, double *alpha, double *beta)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return innovation_entry(c, h, QOp{q}, r, flags, k, d_b, ldb, d_x, ldx, tol, maxiter, {iterations, status, residual_sq, rhs_sq, alpha, beta},
                            ON_DEVICE, "smm_innovation_solve_coef", /*coef=*/true);
}

extern "C" int smm_innovation_solve_coef_kron(smm_ctx *c, smm_csr *h, smm_csr *d, smm_csr *e, smm_csr *r, int flags, int64_t k,
                                              const double *d_b, int64_t ldb, double *d_x, int64_t ldx, double tol, int64_t maxiter,
                                              int *iterations, int *status, double *residual_sq, double *rhs_sq, double *alpha, double *beta)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    return innovation_entry(c, h, q_factors(d, e), r, flags, k, d_b, ldb, d_x, ldx, tol, maxiter,
                            {iterations, status, residual_sq, rhs_sq, alpha, beta}, ON_DEVICE, "smm_innovation_solve_coef_kron", /*coef=*/true);
}

// ------------------------------------------------------------------------------ memory helpers
extern "C" int smm_device_malloc(smm_ctx *c, int64_t bytes, void **d_ptr)
{
    if (!c || !d_ptr || bytes < 0) return fail(SMM_ERR_INVALID, "bad argument");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    hipError_t e = dev_malloc(c, d_ptr, (size_t)std::max<int64_t>(bytes, 16));
    if (e != hipSuccess) { return fail(SMM_ERR_ALLOC, "hipMalloc(%lld): %s", (long long)bytes, hipGetErrorString(e)); }
    return SMM_OK;
}
extern "C" int smm_device_free(smm_ctx *c, void *d_ptr)
{
    if (!c) return fail(SMM_ERR_INVALID, "ctx is NULL");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipFree(d_ptr));
    return SMM_OK;
}
extern "C" int smm_memcpy_d2h(smm_ctx *c, void *dst, const void *src, int64_t bytes)
{
    if (!c || bytes < 0) return fail(SMM_ERR_INVALID, "bad argument");
    if (bytes == 0) return SMM_OK;
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}
extern "C" int smm_memcpy_h2d(smm_ctx *c, void *dst, const void *src, int64_t bytes)
{
    if (!c || bytes < 0) return fail(SMM_ERR_INVALID, "bad argument");
    if (bytes == 0) return SMM_OK;
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SMM_OK;
}
