"""The cache of device operands and symbolic plans behind the entry points of matrix_ops.py.

The reference re-marshals both operands from the caller's CURRENT arrays on every call (matrix_ops.py:339-340,
:187-202); its README's use case is many products on one sparsity pattern (README.md:5,13: covariance matrices).
Here an uploaded operand stays resident in HBM together with what the kernels derive from it (validation, tile
index, packed payload, 16-bit columns, the sliced-ELL copy of H), and the symbolic phase of a product stays
resident as a plan:
  * an operand is recognised by the CONTENT of its three arrays -- a 64-bit hash of every byte
    (smm_host_hash64: a chain of bijective steps, so a change of any one element changes it), taken on
    every call.  An operand edited in place between two calls is therefore never served stale, and an
    equal matrix in other arrays is a hit.  Nothing is assumed from object identity;
  * same indptr/indices hashes, other data hash: only the values travel (smm_csr_update_values: the value
    array and the value halves of the cached copies are rewritten in place), and
  * a product whose two patterns and mode were seen before re-runs only the numeric phase of its cached
    plan: no smm_symbolic / smm_runs / smm_segptr launch at all.
Entries are dropped when the arrays they were made from have been garbage-collected, least recently used
first beyond SMM_OPERAND_CACHE entries (default 4; 0 = marshal afresh on every call, exactly as the
reference) or SMM_OPERAND_CACHE_GB of HBM (default 16; what the library reports for each handle and plan,
derived copies included), and all at once when an allocation fails (the product is then retried once).
pin_operand() is the explicit alternative: a handle the caller owns, no hashing at all.

All of it is one OperandCache: its state, its lock and its three limits.  The package uses `default_cache`; a test
makes a fresh one.  matrix_ops imports from this module, never the other way round.
"""
import collections
import ctypes
import os
import threading
import weakref

import numpy as np
from scipy.sparse import csr_matrix

from ._lib import SMM_ERR_ALLOC, SmmError, SmmLibrary


def _hash(a):
    a = np.ascontiguousarray(a)
    return int(SmmLibrary().get_lib().smm_host_hash64(ctypes.c_void_p(a.ctypes.data), a.nbytes))


def _operand_key(m):
    """(pattern key, data key) of a scipy CSR matrix: full-content hashes of indptr / indices and of data.
    Any in-place edit of any element changes the part it belongs to."""
    nnz = int(m.indptr[-1]) if len(m.indptr) else 0
    idx, dat = m.indices[:nnz], m.data[:nnz]
    pattern = (tuple(m.shape), nnz, m.indptr.dtype.str, idx.dtype.str, _hash(m.indptr), _hash(idx))
    return pattern, (dat.dtype.str, _hash(dat))


class _Entry:
    # nbytes: HBM of the handle and its cached copies as of its last use (refreshed OUTSIDE the cache's lock: the query
    # takes the context's lock and would wait for a running product); dead: retired while leased, the last lease closes it
    __slots__ = ("handle", "pattern", "data_key", "users", "refs", "nbytes", "dead")

    def __init__(self, handle, pattern, data_key):
        self.handle, self.pattern, self.data_key, self.users, self.refs = handle, pattern, data_key, 0, []
        self.nbytes, self.dead = 0, False

    def remember(self, arr):
        self.refs = [r for r in self.refs if r() is not None]
        if not any(r() is arr for r in self.refs):
            try:
                self.refs.append(weakref.ref(arr))
            except TypeError:
                pass

    def orphaned(self):
        return bool(self.refs) and all(r() is None for r in self.refs)


class _PlanEntry:
    __slots__ = ("plan", "a", "b", "users", "nbytes")

    def __init__(self, plan, a, b, nbytes=0):
        self.plan, self.a, self.b, self.users, self.nbytes = plan, a, b, 0, nbytes


class _Lease:
    """One call's hold on a device operand: .handle for the engine, .entry when it is a cache entry."""
    __slots__ = ("cache", "handle", "entry", "_transient")

    def __init__(self, cache, handle, entry=None, transient=False):
        self.cache, self.handle, self.entry, self._transient = cache, handle, entry, transient

    def release(self):
        cache = self.cache
        cache.sweep()
        if self.entry is not None:
            ent = self.entry
            nbytes = ent.handle.device_bytes() if ent.handle is not None else 0      # (library call: before taking the lock)
            close = None
            with cache.lock:
                ent.nbytes = nbytes
                ent.users -= 1
                if ent.users == 0 and ent.dead:
                    close = ent.handle               # retired while this call was using it
                elif ent.users == 0 and ent.pattern in cache.operands:
                    cache._trim_locked()             # what had to stay while it was in use may go now
            if close is not None:
                close.close()
            self.entry = None
        elif self._transient and self.handle is not None:
            self.handle.close()
        self.handle = None


class OperandCache:
    """.operands: pattern key -> _Entry, most recently used last; .plans: (pattern key A, pattern key B, symmetric, exact)
    -> _PlanEntry; .graveyard: the entries of PinnedOperands dropped by the garbage collector, retired by the next sweep().
    The limits are plain attributes: .entries (SMM_OPERAND_CACHE, 4), .max_bytes (SMM_OPERAND_CACHE_GB, 16) and
    .plan_entries (SMM_PLAN_CACHE, 2); an argument overrides the environment.  .stats counts 'upload', 'hit',
    'values_update', 'plan_hit', 'plan_miss' (tests, diagnostics)."""

    def __init__(self, entries=None, max_bytes=None, plan_entries=None):
        env = os.environ.get
        self.entries = int(env("SMM_OPERAND_CACHE", "4") if entries is None else entries)
        self.max_bytes = int(float(env("SMM_OPERAND_CACHE_GB", "16")) * (1 << 30) if max_bytes is None else max_bytes)
        self.plan_entries = int(env("SMM_PLAN_CACHE", "2") if plan_entries is None else plan_entries)
        self.lock = threading.RLock()
        self.operands = collections.OrderedDict()
        self.plans = collections.OrderedDict()
        self.graveyard = []                      # (list.append and list.pop are atomic: PinnedOperand.__del__ takes no lock)
        self.stats = collections.Counter()

    def _retire_locked(self, ent):
        """The one way an entry leaves, evicted, collected or unpinned: the plans made on it leave the cache -- an idle one is
        closed now, one in use by _release_plan when its call ends -- and the handle is closed now, or by the last lease."""
        for pk in [pk for pk, pe in self.plans.items() if pe.a is ent or pe.b is ent]:
            pe = self.plans.pop(pk)
            if pe.users == 0:
                pe.plan.close()
        if ent.users > 0:
            ent.dead = True
        elif ent.handle is not None:             # (a PinnedOperand without entries holds none)
            ent.handle.close()

    def sweep(self):
        """Retire what the garbage collector left in the graveyard.  Called wherever the cache is entered; with nothing to
        bury it is one truth test of the list, without the lock."""
        if self.graveyard:
            with self.lock:
                while self.graveyard:
                    self._retire_locked(self.graveyard.pop())

    def _drop_entry_locked(self, key):
        ent = self.operands.pop(key, None)
        if ent is not None:
            self._retire_locked(ent)

    def _cached_bytes_locked(self):
        # (byte counts recorded on the entries: no library call -- it would take the context's lock -- under the cache's lock)
        return sum(e.nbytes for e in self.operands.values()) + sum(pe.nbytes for pe in self.plans.values())

    def _trim_locked(self, keep=(), reserve=0, protect=()):
        """Enforce the limits (entries idle and not in `keep` only); reserve = entries about to be added; protect =
        pattern keys this call is about to look up (its other operand)."""
        operands, plans = self.operands, self.plans
        self.sweep()
        for key in [k for k, e in operands.items() if e.users == 0 and e.orphaned() and e not in keep and k not in protect]:
            self._drop_entry_locked(key)             # the arrays it was made from are gone

        def idle_plan():
            return next((k for k, pe in plans.items() if pe.users == 0), None)

        def idle_entry():
            return next((k for k, e in operands.items() if e.users == 0 and e not in keep and k not in protect), None)

        while len(plans) > max(self.plan_entries, 0) and idle_plan() is not None:
            plans.pop(idle_plan()).plan.close()
        while len(operands) + reserve > self.entries and idle_entry() is not None:
            self._drop_entry_locked(idle_entry())
        while self._cached_bytes_locked() > self.max_bytes:
            if idle_plan() is not None:              # plans (the symbolic phase's lists) go first
                plans.pop(idle_plan()).plan.close()
            elif idle_entry() is not None:
                self._drop_entry_locked(idle_entry())
            else:
                break

    def acquire(self, ctx, m, key=None, protect=()):
        """Device operand for one call (a _Lease).  m: scipy CSR matrix, or a PinnedOperand; key = its
        _operand_key when the caller has it already."""
        if isinstance(m, PinnedOperand):
            return m._lease(ctx)
        if self.entries <= 0:
            self.stats["upload"] += 1
            return _Lease(self, ctx.csr_from_scipy(m), transient=True)
        operands, stats = self.operands, self.stats
        pattern, data_key = key if key is not None else _operand_key(m)
        with self.lock:
            ent = operands.get(pattern)
            if ent is not None and (not ent.handle.handle or ent.handle.ctx is not ctx):
                self._drop_entry_locked(pattern)
                ent = None
            update = False
            if ent is not None:
                if ent.data_key != data_key:
                    if ent.users > 0:                # another call is multiplying with (or uploading) other values right now
                        ent = None
                    else:
                        update = True
                        ent.data_key = None          # in flux: nobody else may take it for a hit until the values are in HBM
                else:
                    stats["hit"] += 1
                if ent is not None:
                    ent.users += 1
                    ent.remember(m.data)
                    operands.move_to_end(pattern)
                    if not update:
                        self._trim_locked(keep=(ent,), protect=protect)
                        return _Lease(self, ent.handle, entry=ent)
            elif pattern not in operands:
                self._trim_locked(reserve=1, protect=protect)     # make room before the upload
            busy = ent is None and pattern in operands
        if update:
            # the host-to-device copy (200 MB at BASELINE configs[1]) runs WITHOUT the lock: the entry is marked in use
            try:
                ent.handle.update_values(m.data[:ent.handle.nnz])
            except BaseException:
                with self.lock:
                    ent.users -= 1
                    if operands.get(pattern) is ent:
                        self._drop_entry_locked(pattern)
                raise
            with self.lock:
                ent.data_key = data_key
                stats["values_update"] += 1
                self._trim_locked(keep=(ent,), protect=protect)
            return _Lease(self, ent.handle, entry=ent)
        h = ctx.csr_from_scipy(m)
        stats["upload"] += 1
        if busy:
            return _Lease(self, h, transient=True)
        nbytes = h.device_bytes()
        with self.lock:
            if pattern in operands:                  # another thread was faster: use ours for this call only
                return _Lease(self, h, transient=True)
            ent = _Entry(h, pattern, data_key)
            ent.nbytes = nbytes
            ent.users = 1
            ent.remember(m.data)
            operands[pattern] = ent
            self._trim_locked(keep=(ent,), protect=protect)
            if pattern not in operands:              # does not fit the cache at all
                ent.users = 0
                return _Lease(self, h, transient=True)
        return _Lease(self, h, entry=ent)

    def plan_for(self, ctx, la, lb, symmetric, exact):
        """(plan, release) for the product of two leased operands: the cached plan of this pair of patterns when
        there is one (numeric phase only), else a fresh symbolic phase, cached when both operands are."""
        plans = self.plans
        key = None
        if la.entry is not None and lb.entry is not None and self.plan_entries > 0:
            key = (la.entry.pattern, lb.entry.pattern, bool(symmetric), bool(exact))
            with self.lock:
                pe = plans.get(key)
                if pe is not None and pe.a is la.entry and pe.b is lb.entry and pe.plan.handle:
                    pe.users += 1
                    plans.move_to_end(key)
                    self.stats["plan_hit"] += 1
                    return pe.plan, lambda: self._release_plan(pe)
        self.stats["plan_miss"] += 1
        plan = ctx.spgemm_plan(la.handle, lb.handle, symmetric=symmetric, exact=exact)
        if key is None:
            return plan, plan.close
        nbytes = plan.device_bytes()
        with self.lock:
            old = plans.pop(key, None)
            if old is not None and old.users == 0:
                old.plan.close()
            pe = _PlanEntry(plan, la.entry, lb.entry, nbytes)
            pe.users = 1
            plans[key] = pe
            self._trim_locked(keep=(la.entry, lb.entry))
        return plan, lambda: self._release_plan(pe)

    def _release_plan(self, pe):
        with self.lock:
            pe.users -= 1
            if pe.users == 0 and not any(v is pe for v in self.plans.values()):
                pe.plan.close()                      # evicted while in use

    def clear_cache(self):
        """Forget every cached operand and plan and return their HBM to the device: the handles are destroyed, and the
        scratch of the closed plans -- which the library keeps pooled for reuse -- is released too (smm_ctx_release_pool).
        Handles in use by a running call are released when that call ends."""
        ctxs = {}
        with self.lock:
            self.sweep()
            for pk in list(self.plans):
                pe = self.plans.pop(pk)
                ctxs[id(getattr(pe.plan, "ctx", None))] = getattr(pe.plan, "ctx", None)
                if pe.users == 0:
                    pe.plan.close()
            for key, ent in list(self.operands.items()):
                ctxs[id(getattr(ent.handle, "ctx", None))] = getattr(ent.handle, "ctx", None)
                self._drop_entry_locked(key)         # (an entry still leased is closed by that lease's release)
        for c in ctxs.values():
            release = getattr(c, "release_pool", None)
            if release is not None and getattr(c, "handle", None):
                release()

    def set_operand_cache(self, entries):
        """Number of operands kept resident between calls (0 switches the cache off: every call marshals both
        operands afresh, as the reference does); returns the old value."""
        old, self.entries = self.entries, int(entries)
        if self.entries <= 0:
            self.clear_cache()
        return old

    def with_leases(self, ctx, mats, body):
        """body(*leases) with every operand of `mats` leased (the operand cache applies to each), retried once after
        clear_cache() when the device ran out of memory while resident operands / plans were in the way."""
        self.sweep()

        def product():
            cached = self.entries > 0
            keys = [_operand_key(m) if cached and not isinstance(m, PinnedOperand) else None for m in mats]
            leases = []
            try:
                for i, m in enumerate(mats):
                    protect = tuple(k[0] for k in keys[i + 1:] if k is not None)
                    leases.append(self.acquire(ctx, m, keys[i], protect=protect))
                return body(*leases)
            finally:
                for lease in reversed(leases):
                    lease.release()

        try:
            return product()
        except SmmError as e:
            if e.code != SMM_ERR_ALLOC or not (self.operands or self.plans):
                raise
            self.clear_cache()
            return product()


class PinnedOperand:
    """An operand the caller keeps resident explicitly (no hashing, no look-up): pass it to
    sparse_matrix_multiply() in place of the matrix.  update_values() replaces the values on the same
    sparsity pattern; unpin() releases the HBM -- at once, or when the call that is running with it ends.
    Garbage collection of an operand that was not unpinned only leaves a note: the next call into the package
    (any product, pin_operand, clear_cache, the end of a running call) frees the HBM.  `matrix` is a scipy CSR
    matrix (pin_operand() coerces); an operand belongs to one OperandCache, the package's unless `cache` is given."""

    def __init__(self, ctx, matrix, cache=None):
        self._cache = default_cache if cache is None else cache
        self._cache.sweep()
        self.shape, self.nnz = tuple(matrix.shape), int(matrix.nnz)
        self._ctx = ctx
        self._handle = ctx.csr_from_scipy(matrix) if self.nnz else None
        self._entry = _Entry(self._handle, ("pinned", id(self)), None)

    @classmethod
    def _adopt(cls, ctx, handle, shape=None):
        """The second way of making one: around an operand that is in HBM already (a DeviceCSR the library owns, or one
        that borrows device tensors and keeps them alive).  No copy, no hash; the handle belongs to the PinnedOperand
        from here on.  handle None (with shape): an operand without entries, which holds nothing."""
        self = cls.__new__(cls)
        self._cache = default_cache
        self._cache.sweep()
        if handle is not None and handle.nnz == 0:
            shape = (handle.rows, handle.cols)
            handle.close()
            handle = None
        self.shape = (handle.rows, handle.cols) if handle is not None else tuple(int(n) for n in shape)
        self.nnz = handle.nnz if handle is not None else 0
        self._ctx = ctx
        self._handle = handle
        self._entry = _Entry(handle, ("pinned", id(self)), None)
        return self

    def update_values(self, data):
        if self._handle is not None:
            self._handle.update_values(data)

    def to_scipy(self):
        """The operand's own arrays downloaded as a scipy CSR (int32 indices), whatever it was made from."""
        if self._handle is None or not self._handle.handle:
            if self.nnz:
                raise ValueError("PinnedOperand: unpinned")
            return csr_matrix(self.shape, dtype=np.float64)
        from .matrix_ops import _result_csr              # (the entry points' result constructor; not needed to load this module)
        return _result_csr(*self._handle.to_host(), self.shape)

    def _lease(self, ctx):
        if ctx is not self._ctx or self._handle is None or not self._handle.handle:
            raise ValueError("PinnedOperand: unpinned, or pinned on another context")
        with self._cache.lock:
            self._entry.users += 1
        return _Lease(self._cache, self._handle, entry=self._entry)

    def unpin(self):
        """Release the operand.  Plans made on it leave the cache (one that a running call is using is closed when that
        call ends); the handle is closed now, or -- while a call still multiplies with it -- by that call's release."""
        with self._cache.lock:
            if self._handle is not None:
                self._cache._retire_locked(self._entry)
            self._handle = None

    def __del__(self):
        # (may run inside any allocation, also while _trim_locked walks the plans: only leave a note for sweep())
        if getattr(self, "_handle", None) is not None:
            self._cache.graveyard.append(self._entry)


default_cache = OperandCache()
cache_stats = default_cache.stats
clear_cache = default_cache.clear_cache
set_operand_cache = default_cache.set_operand_cache
with_leases = default_cache.with_leases
plan_for = default_cache.plan_for
