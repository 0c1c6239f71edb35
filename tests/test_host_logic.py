"""Host-side behaviour of sparse_matrix_multiply() that needs no GPU: the argument checks, the
raised errors and the nnz==0 early returns of the reference (matrix_ops.py:288-322), plus the
shard planner of the multi-GPU driver."""
import numpy as np
import pytest
import scipy.sparse as sp

from sparse_matrix_mult_amd import operand_cache as oc, sparse_matrix_multiply
from sparse_matrix_mult_amd.distributed import balanced_row_shards


def test_signature_is_the_references():
    import inspect
    sig = inspect.signature(sparse_matrix_multiply)
    assert list(sig.parameters) == ["matrix_a", "matrix_b", "output_format", "symmetric", "imem_size",
                                    "use_triple_product", "compute_full_matrix"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["output_format"] == "sparse" and d["symmetric"] is False and d["imem_size"] is None
    assert d["use_triple_product"] is False and d["compute_full_matrix"] is None


def test_import_name_shim():
    from sparse_matrix_mult import sparse_matrix_multiply as f
    assert f is sparse_matrix_multiply


def test_dimension_mismatch_raises():            # reference matrix_ops.py:312-313
    with pytest.raises(ValueError, match="incompatible"):
        sparse_matrix_multiply(np.ones((2, 3)), np.ones((4, 2)))


def test_symmetric_needs_square_result():        # reference matrix_ops.py:321-322
    with pytest.raises(ValueError, match="square"):
        sparse_matrix_multiply(np.ones((2, 3)), np.ones((3, 4)), symmetric=True)


def test_bad_imem_size_and_full_matrix():        # reference matrix_ops.py:291-304
    with pytest.raises(ValueError, match="imem_size"):
        sparse_matrix_multiply(np.ones((2, 2)), np.ones((2, 2)), imem_size="x")
    with pytest.raises(ValueError, match="compute_full_matrix"):
        sparse_matrix_multiply(np.ones((2, 2)), np.ones((2, 2)), compute_full_matrix=2)


def test_zero_operands_return_empty_without_touching_the_gpu():
    """reference tests/test_edge_case.py:54-71 and matrix_ops.py:315-319."""
    z33, z34 = np.zeros((3, 3)), np.zeros((3, 4))
    r = sparse_matrix_multiply(z33, z34, output_format="sparse")
    assert sp.isspmatrix_csr(r) and r.shape == (3, 4) and r.nnz == 0 and r.dtype == np.float64
    r = sparse_matrix_multiply(sp.csr_matrix(z33), sp.csr_matrix(z34), output_format="dense")
    assert isinstance(r, np.ndarray) and r.shape == (3, 4) and not r.any()
    r = sparse_matrix_multiply(z33, np.ones((3, 4)), use_triple_product=False, output_format="dense", symmetric=False)
    assert r.shape == (3, 4)
    # the zero check comes before the symmetric-square check, as in the reference (:315 before :321)
    assert sparse_matrix_multiply(z33, z34, symmetric=True).shape == (3, 4)


def test_unknown_output_format_prints_and_returns_zeros(capsys):   # reference :367-368, :377-387
    r = sparse_matrix_multiply(np.ones((2, 2)), np.ones((2, 2)), output_format="coo")
    assert isinstance(r, np.ndarray) and r.shape == (2, 2) and not r.any()
    assert "Invalid output_format" in capsys.readouterr().out


def test_balanced_row_shards():
    work = np.array([1, 1, 1, 1, 100, 1, 1, 1], dtype=float)
    sh = balanced_row_shards(work, 2)
    assert sh[0][0] == 0 and sh[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(sh, sh[1:]))
    assert all(e > b for b, e in sh)
    # more shards than rows: clamped like limits() (workdivision.cpp:26-29)
    assert balanced_row_shards(np.ones(3), 8) == [(0, 1), (1, 2), (2, 3)]
    # uniform work -> near-equal row counts
    sh = balanced_row_shards(np.ones(1000), 8)
    assert max(e - b for b, e in sh) - min(e - b for b, e in sh) <= 1
    # skewed work is balanced by work, not rows
    w = np.concatenate([np.full(100, 50.0), np.full(900, 1.0)])
    sh = balanced_row_shards(w, 4)
    loads = [w[b:e].sum() for b, e in sh]
    assert max(loads) / (sum(loads) / 4) < 1.1
    assert balanced_row_shards([], 4) == [(0, 0)]


# ---- operand cache key (no GPU involved: smm_host_hash64 is host code)
def test_operand_key_sees_every_single_element_edit():
    """The reference marshals the caller's CURRENT arrays on every call (matrix_ops.py:339-340, :187-202); the
    operand cache may therefore only recognise an operand whose every element is unchanged.  Its key is a
    full-content hash: an in-place edit of ANY one element of indptr / indices / data changes the part of the
    key it belongs to (the round-2 key, a strided sample, missed exactly these edits)."""
    from sparse_matrix_mult_amd.operand_cache import _operand_key
    B = sp.random(5000, 5000, density=0.01, format="csr", random_state=np.random.default_rng(1))
    assert B.nnz == 250000
    pat0, dat0 = _operand_key(B)
    assert _operand_key(B.copy()) == (pat0, dat0)                 # content, not identity
    rng = np.random.default_rng(7)
    for k in [12345, 0, B.nnz - 1] + rng.integers(0, B.nnz, 40).tolist():
        old = B.data[k]
        B.data[k] = np.nextafter(old, 2.0)                        # one ulp
        pat, dat = _operand_key(B)
        assert pat == pat0 and dat != dat0, k
        B.data[k] = old
    for k in [777, 0, B.nnz - 1] + rng.integers(0, B.nnz, 40).tolist():
        old = B.indices[k]
        B.indices[k] = old ^ 1
        pat, dat = _operand_key(B)
        assert pat != pat0 and dat == dat0, k
        B.indices[k] = old
    i = 2500
    B.indptr[i] -= 1
    assert _operand_key(B)[0] != pat0
    B.indptr[i] += 1
    assert _operand_key(B) == (pat0, dat0)
    # swapping two elements (same multiset) is seen too: the hash is position-dependent
    B.data[[10, 11]] = B.data[[11, 10]]
    assert _operand_key(B)[1] != dat0


def test_host_hash_is_the_same_for_every_thread_count_and_length_aware(monkeypatch):
    import ctypes
    from sparse_matrix_mult_amd._lib import SmmLibrary
    lib = SmmLibrary().get_lib()
    a = np.random.default_rng(3).integers(0, 255, 40 << 20, dtype=np.uint8)     # 10 blocks of 4 MB
    h = lambda x: lib.smm_host_hash64(ctypes.c_void_p(x.ctypes.data), x.nbytes)
    monkeypatch.setenv("SMM_HASH_THREADS", "1")
    one = h(a)
    monkeypatch.setenv("SMM_HASH_THREADS", "5")
    assert h(a) == one
    assert h(a[:-1]) != one and h(a[:1000]) != h(a[:1001])
    z = np.zeros(64, np.uint8)
    assert len({h(z[:n]) for n in range(1, 65)}) == 64                          # zero padding of the tail is not a collision


# ---- operand / plan cache policy with a stub engine (the same code paths sparse_matrix_multiply() takes; no GPU)
class _FakeHandle:
    def __init__(self, ctx, m):
        self.ctx, self.handle, self.nnz, self.rows, self.cols = ctx, object(), int(m.nnz), m.shape[0], m.shape[1]
        self.values = np.array(m.data[:m.nnz], dtype=np.float64)
        self.updates, self.closes = 0, 0

    def update_values(self, data):
        assert len(data) == self.nnz
        self.values = np.array(data, dtype=np.float64); self.updates += 1

    def device_bytes(self):
        return 12 * self.nnz + 1000 if self.handle else 0

    def close(self):
        self.handle = None
        self.closes += 1


class _FakePlan:
    def __init__(self, a, b):
        self.a, self.b, self.handle, self.nnz, self.closes = a, b, object(), 1, 0

    def device_bytes(self):
        return 5000 if self.handle else 0

    def close(self):
        self.handle = None
        self.closes += 1


class _FakeCtx:
    def __init__(self):
        self.uploads, self.plans = 0, 0

    def csr_from_scipy(self, m):
        self.uploads += 1
        return _FakeHandle(self, m)

    def spgemm_plan(self, a, b, symmetric=False, exact=False):
        self.plans += 1
        return _FakePlan(a, b)


@pytest.fixture()
def cache():
    """A fresh cache with the default limits, whatever the environment says; nothing of the package's own cache is touched."""
    c = oc.OperandCache(entries=4, max_bytes=1 << 40, plan_entries=2)
    yield c
    c.clear_cache()


def _rand(m, n, seed):
    return sp.random(m, n, density=0.1, format="csr", random_state=np.random.default_rng(seed))


def test_cache_policy_hit_update_and_plan_replay(cache):
    ctx = _FakeCtx()
    A, B = _rand(30, 40, 1), _rand(40, 50, 2)

    def call(a, b):
        ka, kb = oc._operand_key(a), oc._operand_key(b)
        la = cache.acquire(ctx, a, ka, protect=(kb[0],)); lb = cache.acquire(ctx, b, kb)
        plan, release = cache.plan_for(ctx, la, lb, False, False)
        vals = (la.handle.values.copy(), lb.handle.values.copy())
        release(); lb.release(); la.release()
        return plan, vals

    p1, _ = call(A, B)
    assert (ctx.uploads, ctx.plans) == (2, 1) and len(cache.operands) == 2 and len(cache.plans) == 1
    p2, _ = call(A, B)                                           # unchanged: both hit, plan replayed
    assert p2 is p1 and (ctx.uploads, ctx.plans) == (2, 1) and cache.stats["hit"] == 2 and cache.stats["plan_hit"] == 1
    B.data[7] += 1.0                                             # in-place edit of one value: seen, values only
    p3, (va, vb) = call(A, B)
    assert p3 is p1 and ctx.uploads == 2 and cache.stats["values_update"] == 1 and np.array_equal(vb, B.data)
    B2 = B.copy(); B2.data *= 2                                  # equal pattern in other arrays: same entry, values replaced
    p4, (va, vb) = call(A, B2)
    assert p4 is p1 and ctx.uploads == 2 and np.array_equal(vb, B2.data)
    B.indices[3] = (B.indices[3] + 1) % 50                       # structural edit in place: a new operand, a new plan
    p5, _ = call(A, B)
    assert p5 is not p1 and ctx.uploads == 3 and ctx.plans == 2


def test_cache_policy_limits_orphans_and_leases(cache):
    import gc
    ctx = _FakeCtx()
    B = _rand(40, 50, 2)
    mats = [_rand(30, 40, 10 + i) for i in range(6)]
    for A in mats:
        la = cache.acquire(ctx, A); lb = cache.acquire(ctx, B); lb.release(); la.release()
    assert len(cache.operands) == 4 and oc._operand_key(B)[0] in cache.operands          # LRU: B was used every time and stays
    # an entry in use is neither evicted nor updated in place
    held = cache.acquire(ctx, mats[5])
    old_values = held.handle.values.copy()
    C = mats[5].copy(); C.data += 1.0
    other = cache.acquire(ctx, C)                                                 # same pattern, other values, entry busy
    assert other.entry is None and np.array_equal(held.handle.values, old_values) and held.handle.updates == 0
    other.release(); held.release()
    # orphans (their arrays are gone) are purged at the next miss, not the operand about to be looked up
    cache.clear_cache()
    T = _rand(30, 40, 99)
    lt = cache.acquire(ctx, T); lt.release()
    pat = oc._operand_key(T)[0]
    T2 = T.copy()                                                               # equal content in other arrays
    del T; gc.collect()
    assert cache.operands[pat].orphaned()
    lx = cache.acquire(ctx, mats[0], protect=(pat,))                             # a miss that protects T's pattern (the call's other operand)
    assert pat in cache.operands
    l2 = cache.acquire(ctx, T2); assert l2.entry is cache.operands[pat] and not l2.entry.orphaned()
    l2.release(); lx.release()
    del T2; gc.collect()
    ly = cache.acquire(ctx, mats[1]); ly.release()                                # no protection now: the orphan goes
    assert pat not in cache.operands
    # byte cap: plans go first, then idle entries
    cache.max_bytes = 1
    lz = cache.acquire(ctx, mats[2]); lz.release()
    assert len(cache.operands) == 0 and len(cache.plans) == 0


# ---- round 4: lock hygiene of the operand cache, unpin while leased, pool release
def test_values_upload_runs_outside_the_cache_lock_and_clear_cache_releases_the_pool(cache):
    """A values-only update (a 200 MB host-to-device copy at BASELINE configs[1]) must not stall callers that need no
    cache state of that entry: while one thread is inside update_values, another thread's acquire / release of a
    different operand completes.  clear_cache() hands the library's pooled scratch back (smm_ctx_release_pool)."""
    import threading
    gate, inside = threading.Event(), threading.Event()

    class SlowHandle(_FakeHandle):
        def update_values(self, data):
            inside.set()
            assert gate.wait(20), "the other thread never got through: the cache lock was held across the upload"
            super().update_values(data)

    class Ctx(_FakeCtx):
        released = 0

        def csr_from_scipy(self, m):
            self.uploads += 1
            return SlowHandle(self, m)

        def release_pool(self):
            Ctx.released += 1

    ctx = Ctx()
    ctx.handle = object()
    B, other = _rand(40, 50, 2), _rand(30, 40, 3)
    cache.acquire(ctx, B).release()
    B2 = B.copy(); B2.data += 1.0
    done = []

    def updater():
        lease = cache.acquire(ctx, B2)                  # same pattern, new values: update path
        done.append(np.array_equal(lease.handle.values, B2.data))
        lease.release()

    t = threading.Thread(target=updater); t.start()
    assert inside.wait(20)
    # the entry is busy: the same pattern with yet other values gets a private upload instead of waiting
    B3 = B.copy(); B3.data += 2.0
    l3 = cache.acquire(ctx, B3); assert l3.entry is None; l3.release()
    lo = cache.acquire(ctx, other); lo.release()        # an unrelated operand goes straight through
    gate.set(); t.join(20)
    assert done == [True] and cache.stats["values_update"] == 1
    cache.clear_cache()
    assert Ctx.released >= 1 and len(cache.operands) == 0


def test_unpin_while_leased_defers_the_close_and_gc_only_leaves_a_note(cache):
    import gc
    ctx = _FakeCtx()
    P = oc.PinnedOperand(ctx, _rand(30, 40, 5), cache)
    B = _rand(40, 50, 6)
    lp = cache.acquire(ctx, P); lb = cache.acquire(ctx, B)
    handle = lp.handle
    P.unpin()                                         # a product is running with it
    assert handle.handle is not None                  # ... so the device handle is still alive
    lb.release(); lp.release()
    assert handle.handle is None                      # closed by the lease that held it
    with pytest.raises(ValueError):
        cache.acquire(ctx, P)
    # garbage collection of a pinned operand never touches the cache structures itself
    Q = oc.PinnedOperand(ctx, _rand(30, 40, 7), cache)
    qh = Q._handle
    del Q; gc.collect()
    assert qh.handle is not None and len(cache.graveyard) == 1
    cache.acquire(ctx, B).release()                     # the next trim buries it
    assert qh.handle is None and not cache.graveyard


# ---- one retire routine behind eviction, collection and unpin(); the graveyard is swept wherever the cache is entered
def _entry_with_an_idle_plan_and_one_in_use(cache, ctx, A, B1, B2, pinned):
    """Operand E (pinned, or a cache entry) with a cached plan that is idle and one that a call is still running:
    (E or None, its lease, its handle, the idle plan, the plan in use, that plan's release)."""
    E = oc.PinnedOperand(ctx, A, cache) if pinned else A
    la = cache.acquire(ctx, E); l1 = cache.acquire(ctx, B1); l2 = cache.acquire(ctx, B2)
    idle, release_idle = cache.plan_for(ctx, la, l1, False, False)
    release_idle()
    busy, release_busy = cache.plan_for(ctx, la, l2, False, False)
    l2.release(); l1.release()
    assert len(cache.plans) == 2 and idle.closes == 0 and busy.closes == 0
    return (E if pinned else None), la, la.handle, idle, busy, release_busy


@pytest.mark.parametrize("door,leased", [("evict", False), ("collect", False), ("collect", True), ("unpin", False), ("unpin", True)])
def test_one_retire_rule_behind_eviction_collection_and_unpin(cache, door, leased):
    """However an entry leaves: its idle plan is closed at once, its plan in use by that plan's release and not before,
    its handle at once when no call holds it and otherwise by the last lease -- and each of them exactly once.  (The entry
    limit never evicts an entry in use, so eviction has no leased case.)"""
    import gc
    ctx = _FakeCtx()
    mats = _rand(30, 40, 21), _rand(40, 50, 22), _rand(40, 60, 23)         # (alive to the end: entries whose arrays are gone are orphans)
    E, la, handle, idle, busy, release_busy = _entry_with_an_idle_plan_and_one_in_use(cache, ctx, *mats, pinned=door != "evict")
    if not leased:
        la.release()
    assert handle.closes == 0 and len(cache.plans) == 2
    if door == "evict":
        cache.entries = 2                                  # E is the least recently used of three idle entries
        cache.acquire(ctx, mats[2]).release()              # a hit on B2: the trim behind it enforces the limit
        assert len(cache.operands) == 2
    elif door == "collect":
        del E; gc.collect()
        assert len(cache.graveyard) == 1 and handle.closes == 0 and idle.closes == 0      # __del__ closed nothing
        cache.sweep()
    else:
        E.unpin()
    assert not cache.plans and not cache.graveyard
    assert idle.closes == 1 and idle.handle is None
    assert busy.closes == 0 and busy.handle is not None    # a call is still running it
    if leased:
        assert handle.closes == 0 and handle.handle is not None
        la.release()
    assert handle.closes == 1 and handle.handle is None
    release_busy()
    assert busy.closes == 1 and busy.handle is None
    cache.clear_cache()                                    # nothing of it is left to close a second time
    assert (handle.closes, idle.closes, busy.closes) == (1, 1, 1)


@pytest.mark.parametrize("point", ["pin", "with_leases_pinned", "with_leases_cache_off", "lease_release"])
def test_every_entry_into_the_cache_buries_what_was_collected(cache, point):
    """A collected PinnedOperand with a cached plan: __del__ closes nothing, and each way into the cache on its own
    closes the handle and the plan -- also the ways that never reach the trim."""
    import gc
    ctx = _FakeCtx()
    P, B = oc.PinnedOperand(ctx, _rand(30, 40, 31), cache), _rand(40, 50, 32)
    handle = P._handle
    lp = cache.acquire(ctx, P); lb = cache.acquire(ctx, B)
    plan, release = cache.plan_for(ctx, lp, lb, False, False)
    release(); lb.release(); lp.release()
    assert list(cache.plans.values())[0].plan is plan
    R1, R2 = oc.PinnedOperand(ctx, _rand(20, 30, 33), cache), oc.PinnedOperand(ctx, _rand(30, 20, 34), cache)
    lr = cache.acquire(ctx, R1)
    if point == "with_leases_cache_off":
        cache.entries = 0
    del P; gc.collect()
    assert len(cache.graveyard) == 1 and handle.handle is not None and handle.closes == 0 and plan.closes == 0

    def body(*leases):                                     # swept before the operands are leased, not by their release
        assert handle.handle is None and plan.handle is None
        return len(leases)

    if point == "pin":
        other = oc.PinnedOperand(ctx, _rand(20, 20, 35), cache)
        assert other._handle.handle is not None
    elif point == "with_leases_pinned":
        assert cache.with_leases(ctx, (R1, R2), body) == 2
    elif point == "with_leases_cache_off":
        assert cache.with_leases(ctx, (_rand(20, 30, 36), _rand(30, 20, 37)), body) == 2
        assert len(cache.operands) == 1                    # (B, from before the switch: nothing was added)
    else:
        lr.release()
    assert handle.handle is None and plan.handle is None and (handle.closes, plan.closes) == (1, 1)
    assert not cache.graveyard and not cache.plans


def test_the_settings_live_on_the_cache_object(cache, monkeypatch):
    from sparse_matrix_mult_amd import matrix_ops
    ctx = _FakeCtx()
    cache.max_bytes = 1
    lease = cache.acquire(ctx, _rand(30, 40, 41)); lease.release()
    assert len(cache.operands) == 0 and len(cache.plans) == 0 and ctx.uploads == 1
    for name in ("_cache", "_plans", "_graveyard", "_cache_entries", "_cache_max_bytes", "_plan_entries"):
        assert not hasattr(matrix_ops, name), name
    # the package's names are the default cache's own
    assert matrix_ops.cache_stats is oc.default_cache.stats and matrix_ops.PinnedOperand is oc.PinnedOperand
    assert matrix_ops.clear_cache == oc.default_cache.clear_cache and matrix_ops.clear_cache is oc.clear_cache
    assert matrix_ops.set_operand_cache is oc.set_operand_cache
    assert cache.set_operand_cache(3) == 4 and cache.entries == 3
    # the limits come from the environment, with the defaults 4 entries, 16 GB, 2 plans
    for var in ("SMM_OPERAND_CACHE", "SMM_OPERAND_CACHE_GB", "SMM_PLAN_CACHE"):
        monkeypatch.delenv(var, raising=False)
    c = oc.OperandCache()
    assert (c.entries, c.max_bytes, c.plan_entries) == (4, 16 << 30, 2)
    monkeypatch.setenv("SMM_OPERAND_CACHE", "7"); monkeypatch.setenv("SMM_OPERAND_CACHE_GB", "0.5"); monkeypatch.setenv("SMM_PLAN_CACHE", "0")
    c = oc.OperandCache()
    assert (c.entries, c.max_bytes, c.plan_entries) == (7, 1 << 29, 0)


def test_operand_cache_loads_without_matrix_ops():
    """operand_cache imports nothing from matrix_ops when it loads.  A fresh interpreter, because this one has the package
    imported; the package's __init__ -- which imports matrix_ops for the public names -- is kept from running by a bare
    package module with the same __path__, so that what is loaded is what operand_cache itself asks for."""
    import os
    import subprocess
    import sys
    child = ("import sys, types\n"
             "pkg = types.ModuleType('sparse_matrix_mult_amd'); pkg.__path__ = [sys.argv[1]]\n"
             "sys.modules['sparse_matrix_mult_amd'] = pkg\n"
             "import sparse_matrix_mult_amd.operand_cache as oc\n"
             "assert 'sparse_matrix_mult_amd.matrix_ops' not in sys.modules, 'operand_cache imported matrix_ops'\n"
             "assert oc.default_cache.stats is oc.cache_stats\n"
             "print('loaded')\n")
    out = subprocess.run([sys.executable, "-c", child, os.path.dirname(oc.__file__)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "loaded", out.stderr[-2000:]
