"""innovation_solve on the device (smm_innovation_solve; Context.innovation_solve_*, innovation_solve).

Contract checked here: under SMM_EXACT, Z and the four info arrays are bit-identical to the numpy restatement
(tests/cg_restatement.py) -- for every width, input kind, stride, form of R, kernel class and column blocking, with columns
that freeze early, break down or hit the iteration limit.  In default mode the true residual (scipy, float64) is within
2 x max(tol, the restatement's true residual) per column, the iteration counts within +-2 of the restatement's, and two
runs agree bit for bit: default mode differs from the restatement only by fusion and the products' summation order,
perturbations of order eps * cond(S + R), far below tol = 1e-8 on these operands."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from cg_restatement import (BREAKDOWN, CASES, CONVERGED, LANES, LIMIT, diag_csr, dominant_diagonal, gaussian_band, local_h,
                            random_band, restate_cg, rhs, system, true_residual)
from spmm_restatement import raw_csr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
TOL = 1e-8
FIELDS = ("iterations", "status", "residual_sq", "rhs_sq")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def _assert_exact(got, want, what):
    (Z, info), (wz, winfo) = got, want
    print(what, "iterations", info.iterations.tolist(), "status", info.status.tolist())
    for f in FIELDS:
        assert _same_bits(getattr(info, f), getattr(winfo, f)), f"{what}: info.{f} {getattr(info, f)} != {getattr(winfo, f)}"
    assert _same_bits(Z, wz), f"{what}: Z differs, max abs {np.nanmax(np.abs(np.asarray(Z) - wz)) if wz.size else 0:.3e}"


@functools.lru_cache(maxsize=None)
def _want(name, k, seed, zero_column, with_r=True, maxiter=None):
    H, Q, r = system(name)
    D = rhs(H.shape[0], k, seed, zero_column)
    return D, restate_cg(H, Q, diag_csr(r) if with_r else None, D, TOL, maxiter)


@pytest.fixture(scope="module")
def small(ctx):
    H, Q, r = system("small")
    hs = [ctx.csr_from_scipy(M) for M in (H, Q, diag_csr(r))]
    yield hs
    for hd in hs:
        hd.close()


@functools.lru_cache(maxsize=None)
def _eigen(shift):
    """Eigen-decomposition of the dense S + shift * I of the small system."""
    H, Q, r = system("small")
    return np.linalg.eigh((H @ Q @ H.T).toarray() + shift * np.eye(H.shape[0]))


@pytest.mark.parametrize("k", [1, 2, 5, 16, 65])
def test_exact_is_the_restatement_at_every_width(ctx, small, k):
    h, q, r = small
    D, want = _want("small", k, 30 + k, 2 if k >= 5 else None)
    _assert_exact(ctx.innovation_solve_host(h, q, r, D, TOL, exact=True), want, f"k={k}")
    assert np.all(want[1].status == CONVERGED) and want[1].iterations.max() > 30
    if k >= 5:
        assert want[1].iterations[2] == 0


@pytest.mark.parametrize("n", [1, LANES - 1, LANES, LANES + 1])
def test_exact_is_the_restatement_around_the_lane_count(ctx, n):
    """dot(u, v) keeps LANES partial sums: systems of 1, LANES - 1, LANES and LANES + 1 rows leave all but one partial
    empty, the last one empty, none empty, and give the first one a second term."""
    K = max(64, 3 * n)
    H, Q = local_h(n, K, 300 + n % 7), gaussian_band(K, 8)
    R = diag_csr(dominant_diagonal(H, Q, 301))
    h, q, r = (ctx.csr_from_scipy(M) for M in (H, Q, R))
    try:
        for k in (1, 5):
            D = rhs(n, k, 302 + k, 2 if k >= 5 else None)
            want = restate_cg(H, Q, R, D, TOL)
            _assert_exact(ctx.innovation_solve_host(h, q, r, D, TOL, exact=True), want, f"n={n} k={k}")
            assert np.all(want[1].status == CONVERGED) and want[1].iterations.max() >= 1
    finally:
        for hd in (h, q, r):
            hd.close()


def test_public_interface_exact():
    import torch
    import sparse_matrix_mult
    from sparse_matrix_mult_amd import pin_operand, set_exact, set_result_device
    from sparse_matrix_mult_amd.engine import SolveInfo
    f = sparse_matrix_mult.innovation_solve
    dev = torch.device("cuda", 0)
    H, Q, r = system("small")
    R = diag_csr(r)
    D, want = _want("small", 5, 35, 2)
    old = set_exact(True)
    try:
        Z, info = f(H, Q, R, D, tol=TOL)
        assert isinstance(Z, np.ndarray) and isinstance(info, SolveInfo) and info.converged
        _assert_exact((Z, info), want, "numpy D, CSR R")
        _assert_exact(f(H, Q, r, D, tol=TOL), want, "diagonal vector R")
        _assert_exact(f(H, Q, r.tolist(), D.tolist(), tol=TOL), want, "lists")
        Zt, info = f(H, Q, R, torch.from_numpy(D).to(dev), tol=TOL)
        assert torch.is_tensor(Zt) and Zt.is_cuda
        _assert_exact((Zt.cpu().numpy(), info), want, "torch D")
        wide = torch.from_numpy(np.concatenate([D, np.full((D.shape[0], 3), np.nan)], axis=1)).to(dev)
        Zt, info = f(H, Q, R, wide[:, :5], tol=TOL)
        _assert_exact((Zt.cpu().numpy(), info), want, "torch D, a strided view")
        d1, want1 = _want("small", 1, 31, None)
        z1, info1 = f(H, Q, R, d1[:, 0].copy(), tol=TOL)
        assert z1.shape == (H.shape[0],)
        _assert_exact((z1[:, None], info1), want1, "1-D D")
        ph, pq, pr = pin_operand(H), pin_operand(Q), pin_operand(R)
        _assert_exact(f(ph, pq, pr, D, tol=TOL), want, "PinnedOperands")
        for p in (ph, pq, pr):
            p.unpin()
        old_dev = set_result_device(True)
        try:
            Zd, info = f(H, Q, R, D, tol=TOL)
            assert torch.is_tensor(Zd) and Zd.is_cuda
            _assert_exact((Zd.cpu().numpy(), info), want, "set_result_device")
        finally:
            set_result_device(old_dev)
        # S alone (the truncated band leaves it slightly indefinite) and the iteration limit: whatever happens is the restatement's
        Dn, wantn = _want("small", 5, 36, 1, with_r=False, maxiter=40)
        _assert_exact(f(H, Q, None, Dn, tol=TOL, maxiter=40), wantn, "R = None, maxiter = 40")
        assert LIMIT in wantn[1].status.tolist()
        Dl, wantl = _want("small", 3, 37, None, maxiter=3)
        _assert_exact(f(H, Q, r, Dl, tol=TOL, maxiter=3), wantl, "maxiter = 3")
        assert wantl[1].status.tolist() == [LIMIT] * 3 and wantl[1].iterations.tolist() == [3] * 3
        _, want0 = _want("small", 3, 37, None, maxiter=0)
        _assert_exact(f(H, Q, r, Dl, tol=TOL, maxiter=0), want0, "maxiter = 0")
    finally:
        set_exact(old)


def test_strided_device_buffers_keep_their_padding(ctx, small):
    import torch
    dev = torch.device("cuda", ctx.device)
    h, q, r = small
    n = h.rows
    for k, ldb, ldx in ((5, 8, 7), (4, 6, 8), (1, 3, 2)):
        D, want = _want("small", k, 40 + k, None)
        Bp = np.full((n, ldb), np.inf)
        Bp[:, :k] = D
        for exact in (True, False):
            db = torch.from_numpy(Bp).to(dev)
            dx = torch.full((n, ldx), -7.25, dtype=torch.float64, device=dev)
            info = ctx.innovation_solve_into(h, q, r, db, ldb, k, dx, ldx, TOL, exact=exact)
            X = dx.cpu().numpy()
            assert np.all(X[:, k:] == -7.25), f"padding written: k={k} ldx={ldx}"
            assert np.array_equal(db.cpu().numpy(), Bp), "B written"
            if exact:
                _assert_exact((X[:, :k], info), want, f"strided k={k}")
            else:
                assert np.all(info.status == CONVERGED)


def test_unsorted_rows_and_repeated_columns(ctx):
    H0, Q, r = system("small")
    rng = np.random.default_rng(51)
    cols = H0.indices.reshape(-1, 8).copy()
    cols[:, 1] = cols[:, 0]                                       # a repeated column in every row
    perm = np.argsort(rng.random(cols.shape), axis=1)
    cols = np.take_along_axis(cols, perm, axis=1)                 # in any order
    H = raw_csr(H0.indptr, cols.ravel(), H0.data, H0.shape)
    D = rhs(H.shape[0], 5, 52, 3)
    want = restate_cg(H, Q, diag_csr(r), D, TOL)
    h, q, rr = (ctx.csr_from_scipy(M) for M in (H, Q, diag_csr(r)))
    try:
        _assert_exact(ctx.innovation_solve_host(h, q, rr, D, TOL, exact=True), want, "raw_csr H")
        assert np.all(want[1].status == CONVERGED)
    finally:
        for hd in (h, q, rr):
            hd.close()


def test_frozen_columns_stay_frozen_and_harm_nobody(ctx, small):
    """Columns: random, a combination of three dominant eigenvectors (converges tens of iterations early), zero, one with a
    NaN (breaks down at once; its NaN direction keeps going through every product), random."""
    h, q, r = small
    H, Q, rv = system("small")
    lam, V = np.linalg.eigh((H @ Q @ H.T + diag_csr(rv)).toarray())
    D = rhs(H.shape[0], 5, 61, 2)
    D[:, 1] = V[:, -3:] @ np.array([1.0, -2.0, 0.5])
    D[7, 3] = np.nan
    want = restate_cg(H, Q, diag_csr(rv), D, TOL)
    it = want[1].iterations
    assert want[1].status.tolist() == [CONVERGED, CONVERGED, CONVERGED, BREAKDOWN, CONVERGED]
    assert it[2] == 0 and it[3] == 0 and it[1] + 20 <= min(it[0], it[4]), it
    got = ctx.innovation_solve_host(h, q, r, D, TOL, exact=True)
    _assert_exact(got, want, "early, zero and NaN columns")
    assert np.all(np.isfinite(got[0][:, [0, 1, 2, 4]])) and not got[0][:, 3].any()
    Z, info = ctx.innovation_solve_host(h, q, r, D, TOL, exact=False)
    assert info.status.tolist() == want[1].status.tolist() and np.all(np.isfinite(Z[:, [0, 1, 2, 4]]))


def test_indefinite_system_breaks_down_without_harming_the_rest(ctx, small):
    """R = -10 I makes S + R indefinite.  Random columns break down; a column spanned by eigenvectors of positive
    eigenvalues converges next to them."""
    h, q, _ = small
    H, Q, _ = system("small")
    n = H.shape[0]
    lam, V = _eigen(-10.0)
    assert lam[0] < 0 < lam[-1]
    D = rhs(n, 3, 62)
    D[:, 1] = V[:, -2:] @ np.array([1.0, 3.0])
    R = diag_csr(np.full(n, -10.0))
    want = restate_cg(H, Q, R, D, TOL, 200)
    assert want[1].status.tolist() == [BREAKDOWN, CONVERGED, BREAKDOWN], want[1].status
    rr = ctx.csr_from_scipy(R)
    try:
        got = ctx.innovation_solve_host(h, q, rr, D, TOL, 200, exact=True)
        _assert_exact(got, want, "indefinite")
        assert true_residual(H, Q, R, got[0], D)[1] <= 2 * TOL
    finally:
        rr.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_every_forced_class_and_column_blocks(ctx, small, mode):
    h, q, r = small
    n, K = h.rows, h.cols
    try:
        for k in (1, 5):
            D, want = _want("small", k, 30 + k, 2 if k >= 5 else None)
            ctx.tune_spmm(mode)
            _assert_exact(ctx.innovation_solve_host(h, q, r, D, TOL, exact=True), want, f"mode={mode} k={k}")
        # a budget for two columns per block (5 -> 2, 2, 1), then one byte (one column per block)
        for budget in (2 * (5 * n + 2 * K) * 8, 1):
            ctx.tune_spmm(mode, budget)
            _assert_exact(ctx.innovation_solve_host(h, q, r, D, TOL, exact=True), want, f"mode={mode} budget={budget}")
    finally:
        ctx.tune_spmm(0, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_default_mode_against_the_restatement(ctx, name):
    H, Q, r = system(name)
    R = diag_csr(r)
    D, want = _want(name, 5, 70, 2)
    wres = true_residual(H, Q, R, want[0], D)
    h, q, rr = (ctx.csr_from_scipy(M) for M in (H, Q, R))
    try:
        Z, info = ctx.innovation_solve_host(h, q, rr, D, TOL)
        res = true_residual(H, Q, R, Z, D)
        print(name, "iterations", info.iterations.tolist(), "restatement", want[1].iterations.tolist())
        print(name, "true residual / tol", (res / TOL).tolist(), "restatement", (wres / TOL).tolist())
        assert np.all(info.status == CONVERGED) and np.all(want[1].status == CONVERGED)
        assert np.all(res <= 2 * np.maximum(TOL, wres))
        assert np.all(np.abs(info.iterations.astype(int) - want[1].iterations) <= 2)
        assert info.iterations[2] == 0 and not Z[:, 2].any()
        assert np.all(info.residual_sq <= TOL * TOL * info.rhs_sq)
        Z2, info2 = ctx.innovation_solve_host(h, q, rr, D, TOL)
        assert _same_bits(Z, Z2) and all(_same_bits(getattr(info, f), getattr(info2, f)) for f in FIELDS), "run to run"
    finally:
        for hd in (h, q, rr):
            hd.close()


def test_bad_arguments_are_refused(ctx, small):
    import torch
    dev = torch.device("cuda", ctx.device)
    h, q, r = small
    n = h.rows
    B = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    X = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    it, st = np.zeros(4, np.int32), np.zeros(4, np.int32)
    rs, bs = np.zeros(4), np.zeros(4)
    vp = ctypes.c_void_p
    outs = [vp(a.ctypes.data) for a in (it, st, rs, bs)]

    def call(flags=0, k=4, b=B.data_ptr(), ldb=4, x=X.data_ptr(), ldx=4, tol=1e-8, maxiter=10, rr=r.handle, o=outs, qq=q.handle):
        return ctx.lib.smm_innovation_solve(ctx.handle, h.handle, qq, rr, flags, k, vp(b), ldb, vp(x), ldx, tol, maxiter, *o)
    assert call() == 0 and call(rr=None) == 0 and call(k=0) == 0
    for kw in ({"flags": 16}, {"flags": 1}, {"k": -1}, {"ldb": 3}, {"ldx": 3}, {"b": 0}, {"x": 0}, {"tol": 0.0}, {"tol": float("nan")},
               {"tol": float("inf")}, {"maxiter": -1}, {"x": B.data_ptr() + 8 * 4 * 10}, {"rr": q.handle}, {"qq": h.handle},
               {"o": [outs[0], vp(0), outs[2], outs[3]]}):
        assert call(**kw) == -2, kw


def test_value_updates_reach_the_next_solve(ctx):
    H, Q, r = system("small")
    H, Q = H.copy(), Q.copy()
    R = diag_csr(r)
    D = rhs(H.shape[0], 2, 81)
    h, q, rr = (ctx.csr_from_scipy(M) for M in (H, Q, R))
    try:
        _assert_exact(ctx.innovation_solve_host(h, q, rr, D, TOL, exact=True), restate_cg(H, Q, R, D, TOL), "before")
        H.data = H.data * np.random.default_rng(82).uniform(0.5, 1.5, H.nnz)
        h.update_values(H.data)                                   # (drops the cached H^T)
        _assert_exact(ctx.innovation_solve_host(h, q, rr, D, TOL, exact=True), restate_cg(H, Q, R, D, TOL), "H updated")
        Q.data = Q.data * 0.5
        q.update_values(Q.data)
        _assert_exact(ctx.innovation_solve_host(h, q, rr, D, TOL, exact=True), restate_cg(H, Q, R, D, TOL), "Q updated")
    finally:
        for hd in (h, q, rr):
            hd.close()


def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_innovation_solve_host (H^T built inside the call) made to fail at its 1st, 2nd, ... device allocation (hard)
    until it succeeds: each failure is SMM_ERR_ALLOC with nothing handed out, and the call that succeeds is exact."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    H, Q, r = system("small")
    D, want = _want("small", 2, 32, None)
    handles = [c.csr_from_scipy(M) for M in (H, Q, diag_csr(r))]
    try:
        failures = 0
        for nth in range(1, 65):
            c.release_pool()
            c.inject_alloc_failure(nth, hard=True)
            try:
                res = c.innovation_solve_host(*handles, D, TOL, exact=True)
            except SmmError as e:
                assert e.code == -3, f"allocation {nth}: {e}"
                assert c.live_bytes() == 0, f"allocation {nth}: {c.live_bytes()} bytes still handed out"
                failures += 1
                continue
            finally:
                c.inject_alloc_failure(0)
            _assert_exact(res, want, f"after {failures} failed allocations")
            assert c.live_bytes() == 0
            break
        else:
            pytest.fail("never succeeded")
        assert failures >= 10, f"only {failures} allocations failed"
    finally:
        for hd in handles:
            hd.close()
        c.close()


def test_large_system_by_true_residual(ctx):
    """n = 200 000, K = 1 000 000: H with 8 entries per row, Q a random band of half-width 32 (indefinite), R the diagonal
    that makes S + R strictly diagonally dominant; k = 16, default mode, tol = 1e-8."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n, K, k = 200000, 1000000, 16
    H, Q = local_h(n, K, 1), random_band(K, 32, 2)
    R = diag_csr(dominant_diagonal(H, Q, 3))
    D = rhs(n, k, 4, 5)
    h, q, r = (ctx.csr_from_scipy(M) for M in (H, Q, R))
    try:
        dz = torch.empty((n, k), dtype=torch.float64, device=dev)
        info = ctx.innovation_solve_into(h, q, r, torch.from_numpy(D).to(dev), k, k, dz, k, TOL)
        res = true_residual(H, Q, R, dz.cpu().numpy(), D)
        print("large: iterations", info.iterations.tolist(), "true residual / tol", (res / TOL).tolist())
        assert np.all(info.status == CONVERGED) and info.iterations[5] == 0 and info.iterations.max() >= 3
        assert np.all(res <= 2 * TOL)
    finally:
        for hd in (h, q, r):
            hd.close()
