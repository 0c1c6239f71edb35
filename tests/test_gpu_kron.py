"""The Kronecker operand Q = D (x) E on the device (smm_kron_build, smm_kron_apply, smm_triple_apply_kron,
smm_innovation_solve_kron; Context.kron_*, kronecker_product, KroneckerOperand).

Contract checked here (include/smm_hip.h): the built CSR equals the nested loop of tests/kron_restatement.py bit for bit in
its three arrays; under SMM_EXACT the matrix-free apply is the E-first two-step recipe bit for bit, for any legal factors,
row length, width, stride, alignment and column blocking; in default mode it is within 1e-10 ((|D| (x) |E|) |X|)[i, c], two
runs agree bit for bit and the column blocking changes no bit either.  The triple apply and the CG solve with the factor
form of Q equal their restatements under SMM_EXACT and meet the criteria of tests/test_gpu_cg.py in default mode."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from cg_restatement import CONVERGED, true_residual
from kron_restatement import (canonical_pair, closed_form_indptr, kron_bound, kron_system, random_csr, restate_cg_kron,
                              restate_kron_apply, restate_kron_build, restate_triple_kron, tridiag)
from spmm_restatement import operands, raw_csr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
RTOL = 1e-10
TOL = 1e-10
FIELDS = ("iterations", "status", "residual_sq", "rhs_sq")
WIDTHS = [1, 2, 3, 8, 17, 64, 130]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def _assert_bits(got, want, what):
    assert got.shape == want.shape, what
    assert _same_bits(got, want), f"{what}: max abs diff {np.nanmax(np.abs(got - want)) if got.size else 0:.3e}"


def _rows(A, rows):
    """The given rows of A as a CSR, entries in A's stored order."""
    lens = np.diff(A.indptr)[rows]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    take = np.concatenate([np.arange(A.indptr[r], A.indptr[r + 1]) for r in rows] + [np.empty(0, np.int64)]).astype(np.int64)
    return raw_csr(ptr, A.indices[take], A.data[take], (len(rows), A.shape[1]))


class _Pair:
    """The two factors uploaded for one test."""

    def __init__(self, ctx, D, E):
        self.ctx, self.D, self.E = ctx, D, E
        self.d, self.e = ctx.csr_from_scipy(D), ctx.csr_from_scipy(E)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.d.close()
        self.e.close()


# ------------------------------------------------------------------------------------------------ build
def _build_cases():
    rng = np.random.default_rng(101)
    D, E = canonical_pair()
    cases = {"canonical 7x5 (x) 33x29": (D, E, True)}
    cases["1x1"] = (sp.csr_matrix([[2.5]]), sp.csr_matrix([[-3.0]]), True)
    De = random_csr(9, 6, 0.4, 102).tolil()
    De[0] = 0; De[4] = 0; De[8] = 0
    cases["D with empty rows"] = (De.tocsr(), random_csr(11, 13, 0.3, 103), True)
    U = operands()["unsorted_dup"]
    cases["unsorted, repeated columns"] = (_rows(U, list(range(6))), _rows(U, list(range(6, 46))), False)
    cases["dense D 40x40 (x) E 3x3"] = (sp.csr_matrix(rng.uniform(-1, 1, (40, 40))), sp.csr_matrix(rng.uniform(-1, 1, (3, 3))), True)
    idx = np.concatenate([np.sort(rng.permutation(400)[:300]), np.sort(rng.permutation(400)[:7])])
    cases["E with a 300-entry row"] = (sp.csr_matrix(rng.uniform(-1, 1, (2, 2))), raw_csr([0, 300, 307], idx, rng.uniform(-1, 1, 307), (2, 400)),
                                       True)
    cases["odd nnz"] = (raw_csr([0, 2, 3], [0, 2, 1], rng.uniform(-1, 1, 3), (2, 3)),
                        raw_csr([0, 3, 3, 7], [0, 1, 4, 0, 2, 3, 4], rng.uniform(-1, 1, 7), (3, 5)), True)
    return cases


@pytest.mark.parametrize("name", list(_build_cases()))
def test_build_is_the_nested_loop_bit_for_bit(ctx, name):
    D, E, canonical = _build_cases()[name]
    ptr, idx, val = restate_kron_build(D, E)
    if name == "odd nnz":
        assert len(idx) % 2 == 1 and len(idx) % 4
    with _Pair(ctx, D, E) as f:
        q = ctx.kron_build(f.d, f.e)
        try:
            assert (q.rows, q.cols, q.nnz) == (D.shape[0] * E.shape[0], D.shape[1] * E.shape[1], D.nnz * E.nnz)
            gp, gi, gv = q.to_host()
            assert np.array_equal(gp, ptr) and np.array_equal(gp, closed_form_indptr(D, E)), f"{name}: indptr"
            assert np.array_equal(gi, idx), f"{name}: indices"
            _assert_bits(gv, val, f"{name}: data")
            assert q.is_canonical() == canonical
            if canonical:
                K = sp.kron(D, E, format="csr")
                assert np.array_equal(gp, K.indptr) and np.array_equal(gi, K.indices) and _same_bits(gv, K.data), f"{name}: scipy.sparse.kron"
        finally:
            q.close()


def test_build_stores_inf_times_zero_as_nan_and_keeps_explicit_zeros(ctx):
    D = raw_csr([0, 2, 3], [0, 1, 1], [np.inf, -0.0, 3.0], (2, 2))
    E = raw_csr([0, 2, 2, 3], [0, 2, 1], [0.0, 2.0, -1.0], (3, 3))
    ptr, idx, val = restate_kron_build(D, E)
    assert np.isnan(val[0]) and (val == 0).sum() >= 2
    with _Pair(ctx, D, E) as f:
        q = ctx.kron_build(f.d, f.e)
        gp, gi, gv = q.to_host()
        q.close()
    assert np.array_equal(gp, ptr) and np.array_equal(gi, idx)
    _assert_bits(gv, val, "special values")
    assert np.isnan(gv[0]) and gv[1] == np.inf


def test_build_refusals_allocate_nothing(ctx):
    lib, vp = ctx.lib, ctypes.c_void_p
    eye = sp.identity(50000, format="csr")
    dense = sp.csr_matrix(np.ones((300, 300)))
    with _Pair(ctx, eye, dense) as f:
        before = ctx.live_bytes()
        out = vp()
        assert lib.smm_kron_build(ctx.handle, f.d.handle, f.d.handle, ctypes.byref(out)) == -2 and not out.value      # 2.5e9 rows
        assert lib.smm_kron_build(ctx.handle, f.e.handle, f.e.handle, ctypes.byref(out)) == -5 and not out.value      # 8.1e9 entries
        assert b"smm_kron_apply" in lib.smm_last_error()
        assert lib.smm_kron_build(ctx.handle, f.d.handle, None, ctypes.byref(out)) == -2
        assert lib.smm_kron_build(ctx.handle, f.d.handle, f.e.handle, None) == -2
        assert ctx.live_bytes() == before
    # a factor without entries: an operand without entries
    Z = sp.csr_matrix((3, 4))
    with _Pair(ctx, Z, tridiag(5)) as f:
        for a, b in ((f.d, f.e), (f.e, f.d)):
            q = ctx.kron_build(a, b)
            assert (q.rows, q.cols, q.nnz) == (a.rows * b.rows, a.cols * b.cols, 0)
            assert not q.to_host()[0].any()
            q.close()


def test_a_pinned_product_is_an_operand_like_any_other():
    import sparse_matrix_mult_amd as smm
    D, E = canonical_pair()
    rng = np.random.default_rng(104)
    X = rng.standard_normal((D.shape[1] * E.shape[1], 5))
    B = random_csr(D.shape[1] * E.shape[1], 40, 0.1, 105)
    old = smm.set_exact(True)
    try:
        Qs = smm.kronecker_product(D, E)
        K = sp.kron(D, E, format="csr")
        assert sp.isspmatrix_csr(Qs) and Qs.indices.dtype == np.int32
        assert np.array_equal(Qs.indptr, K.indptr) and np.array_equal(Qs.indices, K.indices) and _same_bits(Qs.data, K.data)
        P = smm.kronecker_product(D, E, pin=True)
        assert isinstance(P, smm.PinnedOperand) and P.shape == Qs.shape and P.nnz == Qs.nnz
        _assert_bits(smm.sparse_dense_multiply(P, X), smm.sparse_dense_multiply(Qs, X), "sparse_dense_multiply on the pinned product")
        Cp, Cs = smm.sparse_matrix_multiply(P, B), smm.sparse_matrix_multiply(Qs, B)
        assert np.array_equal(Cp.indptr, Cs.indptr) and np.array_equal(Cp.indices, Cs.indices) and _same_bits(Cp.data, Cs.data)
        back = P.to_scipy()
        assert np.array_equal(back.indices, K.indices) and _same_bits(back.data, K.data)
        P.unpin()
    finally:
        smm.set_exact(old)


# ------------------------------------------------------------------------------------------------ apply
def _check_apply(ctx, f, ks, what, seed=7):
    rng = np.random.default_rng(seed)
    for k in ks:
        X = rng.standard_normal((f.D.shape[1] * f.E.shape[1], k))
        want = restate_kron_apply(f.D, f.E, X)
        _assert_bits(ctx.kron_apply_host(f.d, f.e, X, exact=True), want, f"{what} exact k={k}")
        got = ctx.kron_apply_host(f.d, f.e, X, exact=False)
        assert np.all(np.abs(got - want) <= RTOL * kron_bound(f.D, f.E, X)), f"{what} default k={k}: beyond 1e-10 (|D| (x) |E|)|X|"
        _assert_bits(ctx.kron_apply_host(f.d, f.e, X, exact=False), got, f"{what} default run-to-run k={k}")


@pytest.mark.parametrize("pc", [1, 5, 40])
def test_apply_every_width_against_the_restatement(ctx, pc):
    D, E = random_csr(4, pc, 0.6, 200 + pc), random_csr(30, 20, 0.25, 201)
    with _Pair(ctx, D, E) as f:
        _check_apply(ctx, f, WIDTHS, f"p'={pc}")
        X = np.random.default_rng(1).standard_normal((pc * 20, 3))
        two = np.asarray(D @ np.stack([E @ X[t * 20:(t + 1) * 20] for t in range(pc)]).reshape(pc, 30 * 3)).reshape(4 * 30, 3)
        _assert_bits(ctx.kron_apply_host(f.d, f.e, X, exact=True), two, "scipy's two-step recipe")
        x1 = X[:, 0].copy()
        y1 = ctx.kron_apply_host(f.d, f.e, x1, exact=True)
        assert y1.shape == (120,)
        _assert_bits(y1, two[:, 0], "1-D X")


def test_apply_odd_factors(ctx):
    rng = np.random.default_rng(210)
    with _Pair(ctx, random_csr(5, 7, 0.5, 211), random_csr(30, 20, 0.3, 212)) as f:
        _check_apply(ctx, f, [1, 2, 17], "rectangular 5x7 (x) 30x20")
    D = raw_csr([0, 4, 4, 4, 9, 9], [3, 0, 3, 3, 1, 1, 2, 0, 1], rng.uniform(-1, 1, 9), (5, 4))       # empty rows, repeated columns
    U = operands()["unsorted_dup"]
    with _Pair(ctx, D, _rows(U, list(range(40)))) as f:
        _check_apply(ctx, f, [1, 3, 8], "D with empty rows and repeated columns")
    with _Pair(ctx, random_csr(3, 2, 1.0, 213), operands()["boundaries"]) as f:                       # rows of 0 .. 4097 entries
        assert np.diff(f.E.indptr).max() == 4097
        _check_apply(ctx, f, [1, 2, 8], "E with every boundary length")
    with _Pair(ctx, sp.csr_matrix(rng.uniform(-1, 1, (1, 5000))), sp.csr_matrix(rng.uniform(-1, 1, (2, 2)))) as f:
        _check_apply(ctx, f, [1, 4, 17], "D one dense row of 5000")


@pytest.mark.parametrize("shift_x,shift_y", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_strides_alignment_and_padding(ctx, shift_x, shift_y):
    """ldx, ldy > k, and X, Y or both one double into a 16-byte aligned buffer (even k and strides: the 16-byte path must
    not be taken there).  The padding and everything outside the views keep the sentinel."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(220)
    with _Pair(ctx, random_csr(4, 5, 0.6, 221), random_csr(30, 20, 0.25, 222)) as f:
        m, kx = 4 * 30, 5 * 20
        for k, ldx, ldy in ((1, 3, 2), (2, 2, 2), (7, 9, 8), (8, 10, 12), (64, 64, 66)):
            Xp = rng.standard_normal((kx, ldx))
            want = restate_kron_apply(f.D, f.E, Xp[:, :k])
            xbuf = torch.zeros(kx * ldx + 2, dtype=torch.float64, device=dev)
            xbuf[shift_x:shift_x + kx * ldx] = torch.from_numpy(Xp.ravel()).to(dev)
            dx = xbuf[shift_x:shift_x + kx * ldx]
            for exact in (True, False):
                ybuf = torch.full((m * ldy + 2,), -7.25, dtype=torch.float64, device=dev)
                dy = ybuf[shift_y:shift_y + m * ldy]
                assert dx.data_ptr() % 16 == 8 * shift_x and dy.data_ptr() % 16 == 8 * shift_y
                ctx.kron_apply_into(f.d, f.e, dx, ldx, k, dy, ldy, exact=exact)
                flat = ybuf.cpu().numpy()
                what = f"shift {shift_x},{shift_y} k={k} ldx={ldx} ldy={ldy} exact={exact}"
                assert np.all(flat[:shift_y] == -7.25) and np.all(flat[shift_y + m * ldy:] == -7.25), f"outside the view: {what}"
                Y = flat[shift_y:shift_y + m * ldy].reshape(m, ldy)
                assert np.all(Y[:, k:] == -7.25), f"padding written: {what}"
                if exact:
                    _assert_bits(Y[:, :k], want, what)
                else:
                    assert np.all(np.abs(Y[:, :k] - want) <= RTOL * kron_bound(f.D, f.E, Xp[:, :k])), what


def test_inf_and_nan_reach_exactly_the_rows_that_store_the_pair(ctx):
    D = raw_csr([0, 2, 2, 3], [0, 2, 1], [1.0, -2.0, 0.5], (3, 3))
    E = raw_csr([0, 1, 3, 3, 4], [1, 0, 2, 2], [2.0, 1.0, -1.0, 3.0], (4, 3))
    Dd, Ed = D.toarray() != 0, E.toarray() != 0
    with _Pair(ctx, D, E) as f:
        for k in (1, 2, 5):
            for bad in (np.inf, np.nan):
                for tc in range(3):
                    for jc in range(3):
                        X = np.zeros((9, k))
                        X[tc * 3 + jc, :] = bad
                        hit = np.outer(Dd[:, tc], Ed[:, jc]).ravel()             # row (t, j) stores the pair (tc, jc)
                        for exact in (True, False):
                            Y = ctx.kron_apply_host(f.d, f.e, X, exact=exact)
                            assert np.array_equal(~np.isfinite(Y).all(axis=1), hit), f"k={k} bad={bad} ({tc},{jc}) exact={exact}"
                            assert np.array_equal(~np.isfinite(Y).any(axis=1), hit)         # ... in every column
                            assert not Y[~hit].any()


def test_column_blocking_changes_no_bit_in_either_mode(ctx):
    D, E = random_csr(4, 5, 0.6, 230), random_csr(30, 20, 0.25, 231)
    X = np.random.default_rng(232).standard_normal((100, 5))
    with _Pair(ctx, D, E) as f:
        want = restate_kron_apply(D, E, X)
        whole = ctx.kron_apply_host(f.d, f.e, X, exact=False)
        try:
            for budget in (2 * 5 * 30 * 8, 1):                       # U of two columns, of one
                ctx.tune_spmm(0, budget)
                _assert_bits(ctx.kron_apply_host(f.d, f.e, X, exact=True), want, f"exact, budget {budget}")
                _assert_bits(ctx.kron_apply_host(f.d, f.e, X, exact=False), whole, f"default, budget {budget}")
        finally:
            ctx.tune_spmm(0, 0)


def test_bad_arguments_are_refused(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    lib, vp = ctx.lib, ctypes.c_void_p
    with _Pair(ctx, random_csr(4, 5, 0.6, 240), random_csr(30, 20, 0.25, 241)) as f:
        X = torch.zeros((100, 4), dtype=torch.float64, device=dev)
        Y = torch.zeros((120, 4), dtype=torch.float64, device=dev)
        d, e = f.d.handle, f.e.handle
        for flags, k, ldx, ldy in ((1, 4, 4, 4), (16, 4, 4, 4), (4 | 2, 4, 4, 4), (0, 4, 3, 4), (0, 4, 4, 3), (0, -1, 4, 4)):
            assert lib.smm_kron_apply(ctx.handle, d, e, flags, k, vp(X.data_ptr()), ldx, vp(Y.data_ptr()), ldy) == -2
        assert lib.smm_kron_apply(ctx.handle, d, e, 0, 4, vp(0), 4, vp(Y.data_ptr()), 4) == -2
        assert lib.smm_kron_apply(ctx.handle, d, None, 0, 4, vp(X.data_ptr()), 4, vp(Y.data_ptr()), 4) == -2
        B = torch.zeros((220, 4), dtype=torch.float64, device=dev)                          # X and Y inside one buffer
        assert lib.smm_kron_apply(ctx.handle, d, e, 0, 4, vp(B.data_ptr()), 4, vp(B.data_ptr() + 8 * 4 * 10), 4) == -2
        assert lib.smm_kron_apply(ctx.handle, d, e, 0, 0, vp(0), 0, vp(0), 0) == 0          # k = 0: nothing to do
        # the triple forms want square factors with p r == H.cols
        H = ctx.csr_from_scipy(random_csr(10, 120, 0.1, 242))
        sq = _Pair(ctx, tridiag(4), tridiag(30))
        try:
            W = torch.zeros((10, 2), dtype=torch.float64, device=dev)
            V = torch.zeros((10, 2), dtype=torch.float64, device=dev)
            args = (2, vp(W.data_ptr()), 2, vp(V.data_ptr()), 2)
            assert lib.smm_triple_apply_kron(ctx.handle, H.handle, d, e, 0, *args) == -2                    # not square
            assert lib.smm_triple_apply_kron(ctx.handle, H.handle, sq.d.handle, sq.d.handle, 0, *args) == -2  # 16 != 120
            assert lib.smm_triple_apply_kron(ctx.handle, H.handle, sq.d.handle, sq.e.handle, 16, *args) == -2
            assert lib.smm_triple_apply_kron(ctx.handle, H.handle, sq.d.handle, sq.e.handle, 0, *args) == 0
            it, st, rs, bs = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2), np.zeros(2)
            outs = tuple(vp(a.ctypes.data) for a in (it, st, rs, bs))

            def solve(dd, ee, flags, tol):
                return lib.smm_innovation_solve_kron(ctx.handle, H.handle, dd, ee, None, flags, 2, vp(W.data_ptr()), 2, vp(V.data_ptr()), 2,
                                                     tol, 5, *outs)

            assert solve(d, e, 0, 1e-8) == -2 and solve(sq.d.handle, sq.d.handle, 0, 1e-8) == -2
            assert solve(sq.d.handle, sq.e.handle, 1, 1e-8) == -2 and solve(sq.d.handle, sq.e.handle, 0, 0.0) == -2
            assert solve(sq.d.handle, sq.e.handle, 0, 1e-8) == 0
        finally:
            sq.__exit__()
            H.close()


def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_kron_apply_host, smm_triple_apply_kron_host and smm_innovation_solve_kron_host made to fail at their 1st, 2nd, ...
    device allocation (hard) until they succeed: each failure is SMM_ERR_ALLOC with nothing handed out, and the call that
    finally succeeds is exact."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    H, D, E, R, rhs_ = kron_system()
    X = np.random.default_rng(250).standard_normal((300, 3))
    W = np.random.default_rng(251).standard_normal((400, 3))
    handles = [c.csr_from_scipy(M) for M in (H, D, E, R)]
    h, d, e, r = handles
    try:
        c.triple_apply_kron_host(h, d, e, W, exact=True)                  # (H^T is built and cached before the sweep)
        want_cg = restate_cg_kron(H, D, E, R, rhs_[:, :2], 1e-6)
        cases = [
            ("kron_apply_host", lambda: c.kron_apply_host(d, e, X, exact=True), restate_kron_apply(D, E, X), 3),
            ("triple_apply_kron_host", lambda: c.triple_apply_kron_host(h, d, e, W, exact=True), restate_triple_kron(H, D, E, W), 5),
            ("innovation_solve_kron_host", lambda: c.innovation_solve_kron_host(h, d, e, r, rhs_[:, :2], 1e-6, exact=True)[0], want_cg[0], 8),
        ]
        for name, call, want, least in cases:
            failures = 0
            for nth in range(1, 65):
                c.release_pool()
                c.inject_alloc_failure(nth, hard=True)
                try:
                    res = call()
                except SmmError as err:
                    assert err.code == -3, f"{name}, allocation {nth}: {err}"
                    assert c.live_bytes() == 0, f"{name}, allocation {nth}: {c.live_bytes()} bytes still handed out"
                    failures += 1
                    continue
                finally:
                    c.inject_alloc_failure(0)
                _assert_bits(res, want, f"{name} after {failures} failed allocations")
                assert c.live_bytes() == 0
                break
            else:
                pytest.fail(f"{name} never succeeded")
            assert failures >= least, f"{name}: only {failures} allocations failed"
    finally:
        for hd in handles:
            hd.close()
        c.close()


def test_large_output_beyond_2_31_elements(ctx):
    """Y with 2^25 x 65 > 2^31 elements (17 GB, on the device only): E has one entry per row, U exceeds the default apply
    budget, so X goes in column blocks.  Sampled rows and the last rows against the restatement."""
    import torch
    dev = torch.device("cuda", ctx.device)
    r, rc, k = 1 << 24, 1024, 65
    rng = np.random.default_rng(260)
    E = raw_csr(np.arange(r + 1, dtype=np.int32), rng.integers(0, rc, r).astype(np.int32), rng.uniform(-1, 1, r), (r, rc))
    D = sp.csr_matrix(rng.uniform(-1, 1, (2, 2)))
    X = rng.standard_normal((2 * rc, k))
    dx = torch.from_numpy(X).to(dev)
    dy = torch.empty((2 * r, k), dtype=torch.float64, device=dev)
    try:
        with _Pair(ctx, D, E) as f:
            js = np.concatenate([rng.integers(0, r, 1000), np.arange(r - 32, r)])
            sub = _rows(E, js)
            want = restate_kron_apply(D, sub, X)                         # rows (t, s) of the sampled rows js[s]
            pick = np.concatenate([t * r + js for t in range(2)])
            for exact in (True, False):
                ctx.kron_apply_into(f.d, f.e, dx, k, k, dy, k, exact=exact)
                got = dy[torch.from_numpy(pick).to(dev)].cpu().numpy()
                if exact:
                    _assert_bits(got, want, "large exact")
                else:
                    assert np.all(np.abs(got - want) <= RTOL * kron_bound(D, sub, X)), "large default"
    finally:
        del dy
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ triple apply
@pytest.mark.parametrize("budget", [0, 1])
def test_triple_apply_exact_and_blocked(ctx, budget):
    H, D, E, _, _ = kron_system()
    rng = np.random.default_rng(270)
    hs = [ctx.csr_from_scipy(M) for M in (H, D, E)]
    ctx.tune_spmm(0, budget)
    try:
        for k in (1, 5, 16):
            X = rng.standard_normal((400, k))
            want = restate_triple_kron(H, D, E, X)
            _assert_bits(ctx.triple_apply_kron_host(*hs, X, exact=True), want, f"k={k} budget={budget}")
            got = ctx.triple_apply_kron_host(*hs, X, exact=False)
            assert np.allclose(got, want, rtol=1e-9, atol=1e-12), f"default k={k}"
    finally:
        ctx.tune_spmm(0, 0)
        for hd in hs:
            hd.close()


# ------------------------------------------------------------------------------------------------ solve
@pytest.fixture(scope="module")
def solved():
    H, D, E, R, rhs_ = kron_system()
    want = restate_cg_kron(H, D, E, R, rhs_, TOL)
    assert np.all(want[1].status == CONVERGED) and want[1].iterations[2] == 0 and 15 <= want[1].iterations.max() <= 30
    return want


@pytest.fixture(scope="module")
def system_handles(ctx):
    hs = [ctx.csr_from_scipy(M) for M in kron_system()[:4]]
    yield hs
    for hd in hs:
        hd.close()


@pytest.mark.parametrize("budget", [0, 2 * (5 * 400 + 3 * 300) * 8, 1])
def test_solve_exact_is_the_restatement(ctx, system_handles, solved, budget):
    h, d, e, r = system_handles
    rhs_ = kron_system()[4]
    ctx.tune_spmm(0, budget)
    try:
        Z, info = ctx.innovation_solve_kron_host(h, d, e, r, rhs_, TOL, exact=True)
    finally:
        ctx.tune_spmm(0, 0)
    print("iterations", info.iterations.tolist(), "status", info.status.tolist())
    for fld in FIELDS:
        assert _same_bits(getattr(info, fld), getattr(solved[1], fld)), f"info.{fld}: {getattr(info, fld)} != {getattr(solved[1], fld)}"
    _assert_bits(Z, solved[0], "Z")
    assert info.iterations[2] == 0 and not Z[:, 2].any()


def test_solve_default_mode_against_the_restatement(ctx, system_handles, solved):
    h, d, e, r = system_handles
    H, D, E, R, rhs_ = kron_system()
    Q = sp.kron(D, E, format="csr")
    wres = true_residual(H, Q, R, solved[0], rhs_)
    Z, info = ctx.innovation_solve_kron_host(h, d, e, r, rhs_, TOL)
    res = true_residual(H, Q, R, Z, rhs_)
    print("iterations", info.iterations.tolist(), "restatement", solved[1].iterations.tolist())
    print("true residual / tol", (res / TOL).tolist(), "restatement", (wres / TOL).tolist())
    assert np.all(info.status == CONVERGED)
    assert np.all(res <= 2 * np.maximum(TOL, wres))
    assert np.all(np.abs(info.iterations.astype(int) - solved[1].iterations) <= 2)
    assert info.iterations[2] == 0 and not Z[:, 2].any()
    Z2, info2 = ctx.innovation_solve_kron_host(h, d, e, r, rhs_, TOL)
    assert _same_bits(Z, Z2) and all(_same_bits(getattr(info, fld), getattr(info2, fld)) for fld in FIELDS), "run to run"


def test_solve_with_the_factors_and_with_the_built_matrix(solved):
    import sparse_matrix_mult_amd as smm
    H, D, E, R, rhs_ = kron_system()
    Q = sp.kron(D, E, format="csr")
    wres = true_residual(H, Q, R, solved[0], rhs_)
    for q in (smm.KroneckerOperand(D, E), smm.kronecker_product(D, E)):
        Z, info = smm.innovation_solve(H, q, R, rhs_, tol=TOL)
        assert info.converged
        assert np.all(true_residual(H, Q, R, Z, rhs_) <= 2 * np.maximum(TOL, wres))


# ------------------------------------------------------------------------------------------------ public interface
def test_public_interfaces():
    import torch
    import sparse_matrix_mult
    from sparse_matrix_mult_amd import DeviceCSRResult, pin_operand, set_exact, set_result_device
    dev = torch.device("cuda", 0)
    H, D, E, R, rhs_ = kron_system()
    Dr, Er = canonical_pair()
    rng = np.random.default_rng(280)
    X = rng.standard_normal((Dr.shape[1] * Er.shape[1], 5))
    W = rng.standard_normal((400, 4))
    mul, tri, solve = sparse_matrix_mult.sparse_dense_multiply, sparse_matrix_mult.triple_product_apply, sparse_matrix_mult.innovation_solve
    Qr, Qs = sparse_matrix_mult.KroneckerOperand(Dr, Er), sparse_matrix_mult.KroneckerOperand(D, E)
    want_y, want_w = restate_kron_apply(Dr, Er, X), restate_triple_kron(H, D, E, W)
    want_z = restate_cg_kron(H, D, E, R, rhs_, TOL)
    old = set_exact(True)
    try:
        Y = mul(Qr, X)
        assert isinstance(Y, np.ndarray)
        _assert_bits(Y, want_y, "numpy")
        _assert_bits(mul(Qr, X[:, 0].copy()), want_y[:, 0], "1-D")
        _assert_bits(mul(Qr, X.tolist()), want_y, "list input")
        Yt = mul(Qr, torch.from_numpy(X).to(dev))
        assert torch.is_tensor(Yt) and Yt.is_cuda
        _assert_bits(Yt.cpu().numpy(), want_y, "torch")
        wide = torch.from_numpy(np.concatenate([X, np.full((X.shape[0], 3), np.nan)], axis=1)).to(dev)
        _assert_bits(mul(Qr, wide[:, :5]).cpu().numpy(), want_y, "torch, a strided view")
        _assert_bits(tri(H, Qs, W), want_w, "triple_product_apply")
        _assert_bits(tri(H, Qs, torch.from_numpy(W).to(dev)).cpu().numpy(), want_w, "triple_product_apply torch")
        Z, info = solve(H, Qs, R, rhs_, tol=TOL)
        _assert_bits(Z, want_z[0], "innovation_solve")
        assert all(_same_bits(getattr(info, fld), getattr(want_z[1], fld)) for fld in FIELDS)
        Zt, info = solve(H, Qs, R, torch.from_numpy(rhs_).to(dev), tol=TOL)
        assert torch.is_tensor(Zt) and Zt.is_cuda
        _assert_bits(Zt.cpu().numpy(), want_z[0], "innovation_solve torch")
        pins = [pin_operand(M) for M in (Dr, Er, D, E, H, R)]
        Qp = sparse_matrix_mult.KroneckerOperand(pins[2], pins[3])
        assert Qp.shape == (300, 300) and (abs(Qp.to_scipy() - sp.kron(D, E))).nnz == 0
        _assert_bits(mul(sparse_matrix_mult.KroneckerOperand(pins[0], pins[1]), X), want_y, "PinnedOperand factors")
        _assert_bits(tri(pins[4], Qp, W), want_w, "triple_product_apply, PinnedOperands")
        _assert_bits(solve(pins[4], Qp, pins[5], rhs_, tol=TOL)[0], want_z[0], "innovation_solve, PinnedOperands")
        for p in pins:
            p.unpin()
        old_dev = set_result_device(True)
        try:
            Yd = mul(Qr, X)
            assert torch.is_tensor(Yd) and Yd.is_cuda
            _assert_bits(Yd.cpu().numpy(), want_y, "set_result_device")
            Zd, _ = solve(H, Qs, R, rhs_, tol=TOL)
            assert torch.is_tensor(Zd) and Zd.is_cuda
            _assert_bits(Zd.cpu().numpy(), want_z[0], "innovation_solve, set_result_device")
            Kd = sparse_matrix_mult.kronecker_product(Dr, Er)
            K = sp.kron(Dr, Er, format="csr")
            assert isinstance(Kd, DeviceCSRResult) and Kd.shape == K.shape and Kd.indptr.dtype == torch.int64
            back = Kd.to_scipy()
            assert np.array_equal(back.indptr, K.indptr) and np.array_equal(back.indices, K.indices) and _same_bits(back.data, K.data)
        finally:
            set_result_device(old_dev)
    finally:
        set_exact(old)
