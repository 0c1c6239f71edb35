"""Every entry of the library on a caller's stream, as bench.py runs it ("Streams").

All other GPU tests use a stream the library created.  Here a context launches on a stream it does not own, in the two
modes a caller has: `null` -- Context(0, 0), the device's null stream, which is torch's default stream -- and `side` --
Context(0, s.cuda_stream) for one torch.cuda.Stream() s of the module, the test body running under torch.cuda.stream(s).
With the session context's private stream that is three queues in the process.

1. Parity: the smallest case per entry family that passes through the family's host sequencing (pooled scratch, the
   pinned download ring, the CG's event pair, the flush-and-retry of a failed allocation), against the references of the
   sibling tests: bit for bit under exact=True, the sibling's bound elsewhere.
2. Lifetime: what smm_ctx_create maps a stream to, and that smm_ctx_destroy leaves a caller's stream alive.
3. The ordering contract.  A late producer (tests/stream_cases.py; proved on the CPU by tests/test_stream_cases_cpu.py)
   leaves a sentinel in one buffer of VALUES, and queues on torch's current stream a delay, the copy of the final
   values and an event.  The call is issued while the event is still pending (asserted: "delay too short"), under three
   pairings: `shared` (context on s, torch on s: stream order alone must give the right result, and a call documented not
   to synchronise must return with the event still pending), `private` (the session context, torch on s) and
   `null-vs-side` (Context(0, 0), torch on s: side streams do not block on the null stream); in the last two the wrapper
   must wait for torch.  The consumer direction clones a wrapper's torch results on torch's stream as soon as the call
   returns, and the allocator case makes spgemm_torch's result reuse a block that torch's stream still fills.

The delay, sized on an MI355X: between queuing the producer and issuing the call the host spends 0.021 ms (median; 0.036 ms
at most over the 27 late cases of one run); the delay is 100 ms of torch.cuda._sleep, calibrated by events at the start of
the module -- some five thousand times the latency, and far longer than any of these calls runs (a late case takes 0.11 s,
the delay included)."""
import contextlib
import functools
import time
import types

import numpy as np
import pytest
import scipy.sparse as sp

import stream_cases
from cg_restatement import restate_cg, rhs
from helpers import arrays, assert_csr_equal, check_masked_values, check_triple_masked, check_triple_sparse, masked_want, signed, upper_mask
from interp_restatement import restate as restate_interp
from kron_restatement import restate_cg_kron, restate_kron_apply, restate_kron_build, restate_triple_kron
from sddmm_restatement import entries, restate_exact
from slq_restatement import restate_cg_coef, restate_probes, slq
from spmm_restatement import restate_spmm, restate_triple
from taper_restatement import restate as restate_taper

pytestmark = [pytest.mark.gpu]

DELAY_MS = 100.0
TOL = stream_cases.TOL
PAIRINGS = ("shared", "private", "null-vs-side")
INFO = ("iterations", "status", "residual_sq", "rhs_sq")
LATENCIES = []                       # (case, pairing, host milliseconds between queuing the producer and issuing the call)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if want.dtype.kind != "f":
        assert np.array_equal(got, want), what
        return
    same = _bits(got) == _bits(want)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} values differ, by at most {np.abs(got - want).max():.3e}"


def _dense_of(res, n):
    return sp.csr_matrix((res[2], res[1], res[0]), shape=(n, n)).toarray()


def _restore(c):
    """Every knob a test of this module turns, back to its default."""
    c.tune_shared(20000, 16); c.tune(18000, 8); c.tune_symbolic(0); c.tune_hash(256, 2048); c.tune_slab(0, 0, 0)
    c.tune_stage2(False); c.tune_triple_sparse(0); c.tune_masked(0); c.tune_spmm(0, 0); c.timing(False)
    c.inject_alloc_failure(0)


# ------------------------------------------------------------------------------ fixtures (all of the module)
class _Streams:
    """The module's only side stream, the two contexts on a caller's stream and the session's private one.  Each context
    is made when a test first asks for it: a selection of tests opens no queue it does not use (a process has four)."""

    def __init__(self, request):
        import torch
        self.torch, self.dev, self.request = torch, torch.device("cuda", 0), request
        assert torch.cuda.current_stream(self.dev).cuda_stream == 0, "the module starts on torch's default stream"
        self.side = torch.cuda.Stream(self.dev)
        self.made = []

    def _make(self, stream):
        from sparse_matrix_mult_amd.engine import Context
        self.made.append(Context(0, stream))
        return self.made[-1]

    @functools.cached_property
    def null(self):
        return self._make(0)

    @functools.cached_property
    def on_side(self):
        return self._make(self.side.cuda_stream)

    @functools.cached_property
    def private(self):
        return self.request.getfixturevalue("ctx")

    def close(self):
        self.torch.cuda.synchronize()
        for c in self.made:
            c.close()


@pytest.fixture(scope="module")
def streams(request):
    s = _Streams(request)
    yield s
    s.close()


class _Operands:
    """The handles of stream_cases' operands, uploaded once per context: a handle belongs to its context."""

    def __init__(self):
        self.by_ctx = {}

    def of(self, c):
        if id(c) not in self.by_ctx:
            A, B = stream_cases.product_operands()
            H, Q, L, M = stream_cases.triple_operands()
            sH, sQ, sR = stream_cases.solve_system()
            kH, kD, kE, kR = stream_cases.kron_factors()
            mats = dict(a=A, b=B, bu=stream_cases.unsorted_b(), h=H, q=Q, lm=L, mk=M, sh=sH, sq=sQ, sr=sR, kh=kH, kd=kD, ke=kE, kr=kR)
            self.by_ctx[id(c)] = types.SimpleNamespace(**{k: c.csr_from_scipy(v) for k, v in mats.items()})
        return self.by_ctx[id(c)]

    def close(self):
        for ns in self.by_ctx.values():
            for hd in vars(ns).values():
                hd.close()


@pytest.fixture(scope="module")
def operands(streams):
    ops = _Operands()
    yield ops
    ops.close()


@pytest.fixture(params=["null", "side"])
def mode(request, streams):
    """(context, its operands' owner) with torch's current stream the one the context launches on."""
    c = streams.null if request.param == "null" else streams.on_side
    with (streams.torch.cuda.stream(streams.side) if request.param == "side" else contextlib.nullcontext()):
        assert streams.torch.cuda.current_stream(streams.dev).cuda_stream == c.stream
        try:
            yield c
        finally:
            _restore(c)


@pytest.fixture(scope="module")
def want(oracle):
    """The references of the parity tests, computed once."""
    A, B = stream_cases.product_operands()
    H, Q, L, M = stream_cases.triple_operands()
    w = types.SimpleNamespace()
    w.sparse = oracle.sparse(arrays(A), arrays(B), 300)
    w.sym = oracle.sparse(arrays(A), arrays(B), 300, symmetric=True)
    w.unsorted = oracle.sparse(arrays(A), arrays(stream_cases.unsorted_b()), 300)
    w.dense = oracle.dense(arrays(A), arrays(B), 300)
    w.triple = oracle.triple(arrays(H), arrays(Q), 300, 0)
    w.triple_full = np.triu(w.triple) + np.triu(w.triple, 1).T
    up = sp.csr_matrix((w.sym[2], w.sym[1], w.sym[0]), shape=(300, 300))
    w.mirror = (up + sp.triu(up, 1).T).toarray()
    w.masked = masked_want(oracle, A, B)
    return w


@pytest.fixture(scope="module")
def delay(streams):
    """queue(): a delay of DELAY_MS on torch's current stream -- torch.cuda._sleep where torch has it, else a chain of
    dependent element-wise kernels on a large tensor --, calibrated with events."""
    torch = streams.torch
    if hasattr(torch.cuda, "_sleep"):
        unit, run = 2_000_000, lambda n: torch.cuda._sleep(int(n))
    else:
        big = torch.zeros(1 << 26, dtype=torch.float64, device=streams.dev)

        def run(n):
            for _ in range(int(n)):
                big.add_(1.0)
        unit = 8
    run(unit)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); run(4 * unit); t1.record()
    torch.cuda.synchronize()
    per_ms = 4 * unit / max(t0.elapsed_time(t1), 1e-6)
    amount = max(int(per_ms * DELAY_MS), 1)
    t0.record(); run(amount); t1.record()
    torch.cuda.synchronize()
    print(f"delay: {amount} units run {t0.elapsed_time(t1):.1f} ms (wanted {DELAY_MS} ms)")
    assert t0.elapsed_time(t1) >= 0.5 * DELAY_MS, "the calibrated delay is shorter than half of what was asked for"
    return types.SimpleNamespace(queue=lambda: run(amount))


def _settled(streams, c, call):
    """An entry that takes raw device addresses: ordering is the caller's, so torch's stream first, the context after."""
    streams.torch.cuda.current_stream(streams.dev).synchronize()
    out = call()
    c.synchronize()
    return out


def _to_dev(streams, x):
    return streams.torch.from_numpy(np.ascontiguousarray(x)).to(streams.dev)


def _nan(streams, *shape):
    return streams.torch.full(shape, float("nan"), dtype=streams.torch.float64, device=streams.dev)


# ------------------------------------------------------------------------------ 1a. parity in both modes
def test_csr_product(mode, streams, operands, want):
    c, o = mode, operands.of(mode)
    A, B = stream_cases.product_operands()
    assert_csr_equal(c.spgemm_host(o.a, o.b), want.sparse, values="tol")
    assert_csr_equal(c.spgemm_host(o.a, o.b, exact=True), want.sparse, values="bits")
    assert_csr_equal(c.spgemm_host(o.a, o.bu, exact=True), want.unsorted, values="bits")         # the general path
    assert_csr_equal(c.spgemm_host(o.a, o.bu), want.unsorted, values="tol")
    # symmetric, the rows from 100 on as a shard of their own
    p, i, v = want.sym
    shard = (p[100:] - p[100], i[p[100]:], v[p[100]:])
    a2 = c.csr_from_scipy(A[100:])
    try:
        assert_csr_equal(c.spgemm_host(a2, o.b, symmetric=True, row_offset=100, exact=True), shard, values="bits")
        assert_csr_equal(c.spgemm_host(a2, o.b, symmetric=True, row_offset=100), shard, values="tol")
    finally:
        a2.close()
    c.tune_shared(64, 4); c.tune(64, 4); c.tune_symbolic(200)                                       # B is walked slab by slab
    try:
        assert_csr_equal(c.spgemm_host(o.a, o.b, exact=True), want.sparse, values="bits")
        assert_csr_equal(c.spgemm_host(o.a, o.b), want.sparse, values="tol")
    finally:
        c.tune_shared(20000, 16); c.tune(18000, 8); c.tune_symbolic(0)


@pytest.mark.parametrize("exact", [False, True])
def test_one_plan_replayed_after_update_values(mode, operands, oracle, want, exact):
    c = mode
    A, B = stream_cases.product_operands()
    A2, B2 = signed(A, 181), signed(B, 182)
    a, b = c.csr_from_scipy(A), c.csr_from_scipy(B)
    c.tune_hash(0, 0)                               # dense LDS tiles: the walk that reads B's cached copies
    try:
        plan = c.spgemm_plan(a, b, exact=exact)
        assert_csr_equal(plan.numeric_host(), want.sparse, values="bits" if exact else "tol")
        a.update_values(A2.data); b.update_values(B2.data)
        assert_csr_equal(plan.numeric_host(), oracle.sparse(arrays(A2), arrays(B2), 300), values="bits" if exact else "tol")
        plan.close()
    finally:
        c.tune_hash(256, 2048)
        a.close(); b.close()


def test_wide_index_download_goes_through_the_pinned_ring(mode, operands, want):
    got = mode.spgemm_host(operands.of(mode).a, operands.of(mode).b, exact=True, index_dtype=np.int64)
    assert got[1].dtype == np.int64
    assert_csr_equal(got, (want.sparse[0], want.sparse[1].astype(np.int64), want.sparse[2]), values="bits")


def test_mirrors(mode, streams, operands, want):
    c, o = mode, operands.of(mode)
    for exact in (True, False):
        host = c.spgemm_host_mirrored(o.a, o.b, exact=exact)
        dev = tuple(t.cpu().numpy() for t in c.spgemm_mirrored_torch(o.a, o.b, exact=exact))
        for res, what in ((host, "host"), (dev, "torch")):
            assert np.array_equal(res[0], host[0]) and np.array_equal(res[1], host[1]), what
            if exact:
                _assert_bits(_dense_of(res, 300), want.mirror, f"mirror {what}")
            else:
                assert np.allclose(_dense_of(res, 300), want.mirror, rtol=1e-10, atol=0), what


def test_dense_outputs(mode, streams, operands, want):
    c, o = mode, operands.of(mode)
    _assert_bits(c.dense_host(o.a, o.b, exact=True), want.dense, "dense_host")
    assert np.allclose(c.dense_host(o.a, o.b), want.dense, rtol=1e-10, atol=1e-13)
    out = _nan(streams, 300, 300)
    _settled(streams, c, lambda: c.dense_into(o.a, o.b, out.data_ptr(), exact=True))
    _assert_bits(out.cpu().numpy(), want.dense, "dense_into")
    for ring in (False, True):
        c.tune_stage2(ring)
        try:
            _assert_bits(c.triple_host(o.h, o.q, exact=True), want.triple, f"triple_host ring={ring}")
            assert np.allclose(c.triple_host(o.h, o.q), want.triple, rtol=1e-10, atol=1e-12)
            out = _nan(streams, 200, 200)
            _settled(streams, c, lambda: c.triple_into(o.h, o.q, out.data_ptr(), exact=True))
            _assert_bits(out.cpu().numpy(), want.triple, f"triple_into ring={ring}")
        finally:
            c.tune_stage2(False)


def test_sparse_triple_product(mode, streams, operands, want):
    c, o = mode, operands.of(mode)
    H, Q, L, M = stream_cases.triple_operands()
    T_nnz = int((abs(H) @ abs(Q)).nnz)
    c.tune_triple_sparse(max(T_nnz // 4, 1))         # H in at least three row blocks: the blocks' results are joined
    try:
        for exact in (True, False):
            check_triple_sparse(c.triple_sparse_host(o.h, o.q, exact=exact), H, Q, want.triple, exact)
            res = tuple(t.cpu().numpy() for t in c.triple_sparse_torch(o.h, o.q, exact=exact))
            check_triple_sparse(res, H, Q, want.triple, exact)
            U = upper_mask(L)
            check_triple_masked(c.triple_sparse_host(o.h, o.q, exact=exact, mask=o.lm), U, want.triple, H, Q, exact)
            res = tuple(t.cpu().numpy() for t in c.triple_sparse_torch(o.h, o.q, exact=exact, mask=o.lm))
            check_triple_masked(res, U, want.triple, H, Q, exact)
        full = c.triple_sparse_host(o.h, o.q, full=True, exact=True)
        _assert_bits(_dense_of(full, 200), want.triple_full, "full")
    finally:
        c.tune_triple_sparse(0)
    A, B = stream_cases.product_operands()
    W, S = want.masked
    for masked_mode in (1, 2):
        c.tune_masked(masked_mode)
        try:
            for exact in (True, False):
                check_masked_values(c.spgemm_masked_host(o.a, o.b, o.mk, exact=exact), M, A, B, W, S, exact)
        finally:
            c.tune_masked(0)


@pytest.mark.parametrize("k", [1, 8])
def test_sparse_times_dense(mode, streams, operands, k):
    c, o = mode, operands.of(mode)
    A, _ = stream_cases.product_operands()
    H, Q, _, _ = stream_cases.triple_operands()
    rng = np.random.default_rng(190 + k)
    for transpose in (False, True):
        kx, m = (300, 400) if transpose else (400, 300)
        X = rng.standard_normal((kx, k))
        ref = restate_spmm(A, X, transpose)
        _assert_bits(c.spmm_host(o.a, X, transpose=transpose, exact=True), ref, f"spmm_host T={transpose}")
        got = c.spmm_host(o.a, X, transpose=transpose)
        mag = np.asarray((abs(A).T if transpose else abs(A)) @ np.abs(X))
        assert np.all(np.abs(got - ref) <= 1e-10 * mag)
        ldx, ldy = k + 3, k + 2                          # padding on both sides, left as it was
        Xp = np.concatenate([X, np.full((kx, ldx - k), np.nan)], axis=1)
        dx, dy = _to_dev(streams, Xp), streams.torch.full((m, ldy), -7.25, dtype=streams.torch.float64, device=streams.dev)
        c.spmm_into(o.a, dx, ldx, k, dy, ldy, transpose=transpose, exact=True)
        Y = dy.cpu().numpy()
        assert np.all(Y[:, k:] == -7.25)
        _assert_bits(Y[:, :k], ref, f"spmm_into T={transpose}")
    X = rng.standard_normal((200, k))
    c.tune_spmm(0, 1)                                    # one byte of budget: triple_apply works in column blocks
    try:
        _assert_bits(c.triple_apply_host(o.h, o.q, X, exact=True), restate_triple(H, Q, X), "triple_apply_host")
        assert np.allclose(c.triple_apply_host(o.h, o.q, X), H @ (Q @ (H.T @ X)), rtol=1e-9, atol=1e-12)
    finally:
        c.tune_spmm(0, 0)


def test_builders(mode, streams, operands):
    c, o = mode, operands.of(mode)
    A, _ = stream_cases.product_operands()
    made = []

    def host_arrays(h):
        made.append(h)
        return h.to_host()

    try:
        # (X Y^T) on A's pattern
        rows, cols, w = entries(A)
        rng = np.random.default_rng(195)
        X, Y = rng.standard_normal((300, 8)), rng.standard_normal((400, 8))
        for scale in (False, True):
            ref = restate_exact(X, Y, rows, cols, w if scale else None)
            _assert_bits(c.sddmm_host(o.a, X, Y, scale=scale, exact=True), ref, f"sddmm_host scale={scale}")
            dx, dy = _to_dev(streams, X), _to_dev(streams, Y)
            out = _nan(streams, A.nnz)
            c.sddmm_into(o.a, dx, 8, dy, 8, 8, out, scale=scale, exact=True)
            _assert_bits(out.cpu().numpy(), ref, f"sddmm_into scale={scale}")
        # taper and interpolation from coordinates
        P = stream_cases.taper_restatement.uniform(300, 2, 5)
        ref = restate_taper(P, None, stream_cases.TAPER_CUTOFF, "gaspari_cohn")
        dp = _to_dev(streams, P)
        for got, what in ((host_arrays(c.taper_host(P, None, stream_cases.TAPER_CUTOFF)), "taper_host"),
                          (host_arrays(c.taper_into(dp, 2, dp, 2, 300, 300, 2, stream_cases.TAPER_CUTOFF)), "taper_into")):
            for g, r, part in zip(got, ref, ("indptr", "indices", "data")):
                _assert_bits(g, r, f"{what} {part}")
        axes = stream_cases.interp_axes()
        pts = stream_cases.interp_restatement.inside(300, axes, 174)
        ref = restate_interp(pts, axes, "linear", "error")
        for got, what in ((host_arrays(c.interp_host(pts, axes)), "interp_host"),
                          (host_arrays(c.interp_into(_to_dev(streams, pts), 2, 300, 2, axes)), "interp_into")):
            for g, r, part in zip(got, ref, ("indptr", "indices", "data")):
                _assert_bits(g, r, f"{what} {part}")
        # Kronecker operand, matrix-free apply, transpose
        kH, kD, kE, _ = stream_cases.kron_factors()
        for g, r, part in zip(host_arrays(c.kron_build(o.kd, o.ke)), restate_kron_build(kD, kE), ("indptr", "indices", "data")):
            _assert_bits(g, r, f"kron_build {part}")
        X = rng.standard_normal((300, 3))
        _assert_bits(c.kron_apply_host(o.kd, o.ke, X, exact=True), restate_kron_apply(kD, kE, X), "kron_apply_host")
        W = rng.standard_normal((200, 3))
        _assert_bits(c.triple_apply_kron_host(o.kh, o.kd, o.ke, W, exact=True), restate_triple_kron(kH, kD, kE, W), "triple_apply_kron_host")
        C = A.tocsc()
        for g, r, part in zip(host_arrays(c.transpose(o.a)), (C.indptr, C.indices, C.data), ("indptr", "indices", "data")):
            _assert_bits(g, np.asarray(r, g.dtype), f"transpose {part}")
    finally:
        for h in made:
            h.close()


def _assert_solve(got, ref, what, fields=INFO):
    (Z, info), (wz, winfo) = got, ref
    for f in fields:
        _assert_bits(getattr(info, f), getattr(winfo, f), f"{what}: info.{f}")
    _assert_bits(Z, wz, f"{what}: Z")


@pytest.mark.parametrize("k", [1, 8])
def test_innovation_solve(mode, streams, operands, k):
    c, o = mode, operands.of(mode)
    H, Q, R = stream_cases.solve_system()
    D = rhs(200, k, 200 + k)
    ref = restate_cg(H, Q, R, D, TOL)
    assert ref[1].iterations.max() >= 3 and np.all(ref[1].status == 0)
    _assert_solve(c.innovation_solve_host(o.sh, o.sq, o.sr, D, TOL, exact=True), ref, f"host k={k}")
    db, dz = _to_dev(streams, D), _nan(streams, 200, k)
    info = c.innovation_solve_into(o.sh, o.sq, o.sr, db, k, k, dz, k, TOL, exact=True)
    _assert_solve((dz.cpu().numpy(), info), ref, f"device k={k}")
    Z, info = c.innovation_solve_host(o.sh, o.sq, o.sr, D, TOL)                     # default mode: the sibling's bound
    W = H @ (Q @ (H.T @ Z)) + R @ Z
    res = np.linalg.norm(W - D, axis=0) / np.linalg.norm(D, axis=0)
    Wr = H @ (Q @ (H.T @ ref[0])) + R @ ref[0]
    res_ref = np.linalg.norm(Wr - D, axis=0) / np.linalg.norm(D, axis=0)
    assert np.all(res <= 2 * np.maximum(TOL, res_ref)) and np.all(np.abs(info.iterations - ref[1].iterations) <= 2)


def test_kronecker_solve_and_log_determinant(mode, streams, operands):
    c, o = mode, operands.of(mode)
    kH, kD, kE, kR = stream_cases.kron_factors()
    D = rhs(200, 3, 205)
    _assert_solve(c.innovation_solve_kron_host(o.kh, o.kd, o.ke, o.kr, D, TOL, exact=True), restate_cg_kron(kH, kD, kE, kR, D, TOL), "kron")
    # log det(H Q H^T + R) by stochastic Lanczos quadrature: the probes and the recorded CG coefficients
    H, Q, R = stream_cases.solve_system()
    probes = restate_probes(200, 4, 12345)
    db, dz = _nan(streams, 200, 4), _nan(streams, 200, 4)
    c.probe_fill_into(db, 4, 200, 4, 12345)
    _assert_bits(db.cpu().numpy(), probes, "probes")
    info = c.innovation_solve_coef_into(o.sh, o.sq, o.sr, db, 4, 4, dz, 4, TOL, 100, exact=True)
    ref = restate_cg_coef(H, Q, R, probes, TOL, 100)
    _assert_solve((dz.cpu().numpy(), info), ref, "coefficients", INFO + ("alpha", "beta"))
    got, wanted = slq(info, 200), slq(ref[1], 200)
    assert got[1] == wanted[1] and np.array_equal(got[0], wanted[0])
    sign, logdet = np.linalg.slogdet((H @ Q @ H.T + R).toarray())
    assert sign > 0 and abs(got[1] - logdet) <= 3 * got[2] + 1e-9 * abs(logdet)


def test_a_failed_allocation_is_retried_and_a_hard_one_leaves_nothing_behind(mode, operands, want):
    from sparse_matrix_mult_amd.engine import SmmError
    c, o = mode, operands.of(mode)
    try:
        c.release_pool()                                   # the product's scratch comes from the device, not from the pool
        before = c.alloc_retries()
        c.inject_alloc_failure(1)
        assert_csr_equal(c.spgemm_host(o.a, o.b, exact=True), want.sparse, values="bits")
        assert c.alloc_retries() == before + 1
        c.release_pool()
        live = c.live_bytes()
        c.inject_alloc_failure(1, hard=True)
        with pytest.raises(SmmError) as e:
            c.spgemm_host(o.a, o.b, exact=True)
        assert e.value.code == -3 and c.live_bytes() == live
        assert_csr_equal(c.spgemm_host(o.a, o.b, exact=True), want.sparse, values="bits")
    finally:
        c.inject_alloc_failure(0)


def test_kernel_timing(mode, operands, want):
    c, o = mode, operands.of(mode)
    c.tune_hash(0, 0)
    try:
        c.timing(True); c.timing_reset()
        assert_csr_equal(c.spgemm_host(o.a, o.b, exact=True), want.sparse, values="bits")
        ms, launches = c.kernel_time("smm_numeric")
        assert launches >= 1 and ms > 0.0
    finally:
        c.timing(False)
        c.tune_hash(256, 2048)


# ------------------------------------------------------------------------------ 1b. lifetime
def test_what_a_context_reports_as_its_stream(streams):
    assert streams.null.stream == 0 and streams.on_side.stream == streams.side.cuda_stream != 0
    assert streams.private.stream is None


@pytest.mark.parametrize("which", ["null", "side"])
def test_closing_a_context_leaves_the_callers_stream_alive(streams, want, which):
    from sparse_matrix_mult_amd.engine import Context
    torch = streams.torch
    A, B = stream_cases.product_operands()
    with (torch.cuda.stream(streams.side) if which == "side" else contextlib.nullcontext()):
        cur = torch.cuda.current_stream(streams.dev)
        c = Context(0, cur.cuda_stream)
        a, b = c.csr_from_scipy(A), c.csr_from_scipy(B)
        assert_csr_equal(c.spgemm_host(a, b, exact=True), want.sparse, values="bits")
        a.close(); b.close(); c.close()
        t = torch.ones(4096, dtype=torch.float64, device=streams.dev).mul_(3.0)         # a torch kernel queued on the stream
        cur.synchronize()
        assert cur.query() and float(t.sum().item()) == 3.0 * 4096


def test_two_contexts_on_one_stream_and_a_foreign_handle(streams, oracle, want):
    from sparse_matrix_mult_amd.engine import Context, SmmError
    A, B = stream_cases.product_operands()
    A2, B2 = signed(A, 211), signed(B, 212)
    want2 = oracle.sparse(arrays(A2), arrays(B2), 300)
    with streams.torch.cuda.stream(streams.side):
        c1, c2 = streams.on_side, Context(0, streams.side.cuda_stream)
        h = []
        try:
            h += [c1.csr_from_scipy(A), c1.csr_from_scipy(B), c2.csr_from_scipy(A2), c2.csr_from_scipy(B2)]
            for _ in range(3):
                assert_csr_equal(c1.spgemm_host(h[0], h[1], exact=True), want.sparse, values="bits")
                assert_csr_equal(c2.spgemm_host(h[2], h[3], exact=True), want2, values="bits")
            with pytest.raises(SmmError) as e:
                c1.spgemm_host(h[0], h[3], exact=True)
            assert e.value.code == -2 and "another context" in str(e.value)
            with pytest.raises(SmmError):
                c2.spmm_host(h[0], np.ones(400))
            assert_csr_equal(c2.spgemm_host(h[2], h[3], exact=True), want2, values="bits")
        finally:
            for x in h:
                x.close()
            c2.close()


# ------------------------------------------------------------------------------ 1c. the ordering contract
@pytest.fixture(params=PAIRINGS)
def pairing(request, streams):
    """(name, context) with torch's current stream the side stream."""
    c = {"shared": streams.on_side, "private": streams.private, "null-vs-side": streams.null}[request.param]
    with streams.torch.cuda.stream(streams.side):
        try:
            yield request.param, c
        finally:
            streams.torch.cuda.synchronize()
            _restore(c)


def _producer(streams, delay, buf, final, sentinel):
    """buf holds the sentinel, the device is idle; then, on torch's current stream: the delay, the copy of the final
    values (resident and complete) into buf, and the event this returns with the host time of the queuing."""
    torch = streams.torch
    buf.copy_(sentinel)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    delay.queue()
    buf.copy_(final)
    done = torch.cuda.Event()
    done.record()
    return done, t0


class _Late:
    """One late-producer case on one context: buf (the late tensor); call() -- the wrapper under test, issued while the
    producer is pending --; finish(r) -- whatever turns its return value into the arrays reference() names --;
    reset() -- state the call leaves in the library that has to hold the sentinel again --; nosync: the call is
    documented not to synchronise."""
    nosync = False
    values = "bits"

    def reset(self):
        pass

    def close(self):
        for h in self.handles:
            h.close()


def _late_case(name, streams, c, case):
    torch, dev = streams.torch, streams.dev
    A, B = stream_cases.late_operands()
    L = _Late()
    L.handles = []
    L.buf = torch.empty(case.final.shape, dtype=torch.float64, device=dev)

    def keep(h):
        L.handles.append(h)
        return h

    if name in ("csr_from_torch", "values_changed"):
        a = keep(c.csr_from_scipy(A))
        ptr, idx = _to_dev(streams, arrays(B)[0]), _to_dev(streams, arrays(B)[1])
        if name == "csr_from_torch":
            L.call = lambda: c.csr_from_torch(400, 300, ptr, idx, L.buf)

            def finish(b):
                try:
                    return c.spgemm_host(a, b, exact=True)
                finally:
                    b.close()
            L.finish = finish
        else:
            L.buf.copy_(_to_dev(streams, case.sentinel))
            torch.cuda.synchronize()
            c.tune_hash(0, 0)                            # dense LDS tiles: the default walk reads B's packed payload
            b = keep(c.csr_from_torch(400, 300, ptr, idx, L.buf))
            plan = c.spgemm_plan(a, b)
            plan.numeric_host()
            assert b.device_bytes() > 0, "the first product cached no copy of the borrowed B"
            L.handles.insert(0, plan)
            L.nosync, L.values = True, "tol"
            L.call = b.values_changed
            L.finish = lambda _: plan.numeric_host()

            def reset():                                 # the cached payload holds the sentinel again
                b.values_changed()
                c.synchronize()
            L.reset = reset
    elif name.startswith("spmm_into"):
        a, k = keep(c.csr_from_scipy(A)), case.final.shape[1]
        y = _nan(streams, 300, k)
        L.call = lambda: c.spmm_into(a, L.buf, k, k, y, k, exact=True)
        L.finish = lambda _: (y.cpu().numpy(),)
    elif name == "sddmm_into":
        a = keep(c.csr_from_scipy(A))
        y, out = _to_dev(streams, case.other), _nan(streams, A.nnz)
        L.call = lambda: c.sddmm_into(a, L.buf, 8, y, 8, 8, out, exact=True)
        L.finish = lambda _: (out.cpu().numpy(),)
    elif name == "taper_into":
        L.call = lambda: c.taper_into(L.buf, 2, L.buf, 2, 300, 300, 2, stream_cases.TAPER_CUTOFF)
    elif name == "interp_into":
        axes = stream_cases.interp_axes()
        L.call = lambda: c.interp_into(L.buf, 2, 300, 2, axes)
    else:
        H, Q, R = stream_cases.solve_system()
        h, q, r = (keep(c.csr_from_scipy(M)) for M in (H, Q, R))
        k = case.final.shape[1]
        z = _nan(streams, 200, k)
        L.call = lambda: c.innovation_solve_into(h, q, r, L.buf, k, k, z, k, TOL, exact=True)
        L.finish = lambda info: (z.cpu().numpy(),) + tuple(getattr(info, f) for f in INFO)
    if name in ("taper_into", "interp_into"):
        def finish(h):
            try:
                return h.to_host()
            finally:
                h.close()
        L.finish = finish
    return L


def _assert_result(got, ref, values, what):
    assert len(got) == len(ref), what
    if len(ref) == 3 and values == "tol":
        assert_csr_equal(got, ref, values="tol")
        return
    for i, (g, r) in enumerate(zip(got, ref)):
        _assert_bits(g, np.asarray(r, dtype=np.asarray(g).dtype) if np.asarray(r).dtype.kind != "f" else r, f"{what}: array {i}")


@pytest.mark.parametrize("name", stream_cases.LATE_NAMES)
def test_a_late_producer_is_waited_for(pairing, streams, delay, oracle, name):
    pname, c = pairing
    torch = streams.torch
    case = stream_cases.late_cases(oracle)[name]
    final, sentinel = _to_dev(streams, case.final), _to_dev(streams, case.sentinel)
    ref = case.reference(case.final)
    L = _late_case(name, streams, c, case)
    try:
        # the call once on complete values: every kernel is loaded, and the case itself is right
        L.buf.copy_(final)
        torch.cuda.synchronize()
        _assert_result(L.finish(L.call()), ref, L.values, f"{name} on complete values")
        L.buf.copy_(sentinel)
        torch.cuda.synchronize()
        L.reset()
        done, t0 = _producer(streams, delay, L.buf, final, sentinel)
        latency = (time.perf_counter() - t0) * 1e3
        assert not done.query(), "delay too short: the producer finished before the call was issued"
        r = L.call()
        if pname == "shared" and L.nosync:
            assert not done.query(), f"{name} waited on the host although the context launches on torch's stream"
        got = L.finish(r)
        LATENCIES.append((name, pname, latency))
        print(f"{name} [{pname}]: host latency {latency:.3f} ms, delay {DELAY_MS} ms")
        _assert_result(got, ref, L.values, f"{name} [{pname}]")
        assert done.query()
    finally:
        torch.cuda.synchronize()
        L.close()


def _consumers(c, o, want):
    """name -> (call, check(arrays)) of the wrappers that return torch tensors."""
    H, Q, _, _ = stream_cases.triple_operands()
    A, _ = stream_cases.product_operands()
    C = A.tocsc()

    def pattern():
        t = c.transpose(o.a)                              # (a library-made operand: its build was queued just now)
        try:
            return t.pattern_torch()
        finally:
            t.close()

    return {
        "spgemm_torch": (lambda: c.spgemm_torch(o.a, o.b, exact=True), lambda r: assert_csr_equal(r, want.sparse, values="bits")),
        "spgemm_mirrored_torch": (lambda: c.spgemm_mirrored_torch(o.a, o.b, exact=True),
                                  lambda r: _assert_bits(_dense_of(r, 300), want.mirror, "mirror")),
        "triple_sparse_torch": (lambda: c.triple_sparse_torch(o.h, o.q, exact=True),
                                lambda r: check_triple_sparse(r, H, Q, want.triple, True)),
        "pattern_torch": (pattern, lambda r: (_assert_bits(r[0], C.indptr.astype(np.int32), "indptr"),
                                              _assert_bits(r[1], C.indices.astype(np.int32), "indices"))),
    }


@pytest.mark.parametrize("name", ["spgemm_torch", "spgemm_mirrored_torch", "triple_sparse_torch", "pattern_torch"])
def test_returned_tensors_are_ready_for_torchs_stream(pairing, streams, operands, want, name):
    """The results cloned on torch's current stream as soon as the wrapper returns: the clone and the original are right."""
    pname, c = pairing
    call, check = _consumers(c, operands.of(c), want)[name]
    out = call()
    clones = [t.clone() for t in out]
    streams.torch.cuda.synchronize()
    check(tuple(t.cpu().numpy() for t in clones))
    check(tuple(t.cpu().numpy() for t in out))


@pytest.mark.parametrize("pname", ["private", "null-vs-side"])
def test_a_result_in_a_block_torchs_stream_still_fills(streams, operands, delay, want, pname):
    """spgemm_torch's result tensors reuse the blocks a first result has just given back to torch's allocator, while
    torch's stream still has a delayed sentinel fill of them queued: the wrapper has to drain that stream before the
    library writes there.  Inconclusive (a failure, never a pass) when the allocator hands out another block."""
    torch = streams.torch
    c = streams.private if pname == "private" else streams.null
    o = operands.of(c)
    with torch.cuda.stream(streams.side):
        try:
            first = c.spgemm_torch(o.a, o.b, exact=True)
            torch.cuda.synchronize()
            assert first[2].numel() * 8 == want.sparse[2].nbytes
            ptrs = [t.data_ptr() for t in first]
            delay.queue()
            for t in first:
                t.fill_(-7)                                # (a legal value of each of the three arrays)
            done = torch.cuda.Event()
            done.record()
            del first, t
            assert not done.query(), "delay too short: the fill finished before the call was issued"
            res = c.spgemm_torch(o.a, o.b, exact=True)
            assert res[2].data_ptr() == ptrs[2], "inconclusive: the allocator did not hand the freed block out again"
            torch.cuda.synchronize()
            assert_csr_equal(tuple(t.cpu().numpy() for t in res), want.sparse, values="bits")
        finally:
            torch.cuda.synchronize()


def test_report_the_measured_latency():
    """(not a check of the library: prints what the module docstring quotes; it follows the cases it reports)"""
    if LATENCIES:
        ms = sorted(x[2] for x in LATENCIES)
        print(f"host latency over {len(ms)} late cases: median {ms[len(ms) // 2]:.3f} ms, max {ms[-1]:.3f} ms; delay {DELAY_MS} ms")
        assert DELAY_MS >= 100 * ms[len(ms) // 2], "the delay is no longer a hundred times the host latency: raise DELAY_MS"
