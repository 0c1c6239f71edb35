"""log det(H Q H^T + R) on the device: smm_probe_fill, smm_innovation_solve_coef[_kron] and innovation_logdet.

Contract checked here: the probes are the hash of include/smm_hip.h bit for bit, for every layout; under SMM_EXACT alpha,
beta, X and the four info arrays are bit-identical to the numpy restatement (tests/slq_restatement.py) for every width,
kernel class and column blocking, with zero columns, breakdown and the iteration limit; the right-hand sides that ride in
front of the probes get the bits of innovation_solve; in default mode every sample is within a relative 1e-9 of the dense
eigen-decomposition's value, the estimate within three standard errors of slogdet, and two runs agree bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

from cg_restatement import BREAKDOWN, CONVERGED, LIMIT, diag_csr, rhs, system
from kron_restatement import kron_system, restate_triple_kron
from slq_restatement import dense_log, exact_samples, restate_cg_coef, restate_probes
from spmm_restatement import restate_spmm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
TOL = 1e-8
SEED = 12345
FIELDS = ("iterations", "status", "residual_sq", "rhs_sq")
HIST = ("alpha", "beta")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def _assert_exact(got, want, what, fields=FIELDS + HIST):
    (Z, info), (wz, winfo) = got, want
    print(what, "iterations", info.iterations.tolist(), "status", info.status.tolist())
    for f in fields:
        assert _same_bits(getattr(info, f), getattr(winfo, f)), f"{what}: info.{f} differs"
    assert _same_bits(Z, wz), f"{what}: X differs"


def _solve(ctx, handles, D, maxiter, exact=True, tol=TOL):
    """(X, info) of the recording solve on device copies of D; handles: (h, q, r) or (h, d, e, r)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    D = np.ascontiguousarray(D, dtype=np.float64)
    n, k = D.shape
    b = torch.from_numpy(D).to(dev)
    x = torch.full((n, k), np.nan, dtype=torch.float64, device=dev)
    if len(handles) == 4:
        h, d, e, r = handles
        info = ctx.innovation_solve_coef_kron_into(h, d, e, r, b, k, k, x, k, tol, maxiter, exact=exact)
    else:
        h, q, r = handles
        info = ctx.innovation_solve_coef_into(h, q, r, b, k, k, x, k, tol, maxiter, exact=exact)
    return x.cpu().numpy(), info


def _history_counts(info):
    return [int(np.count_nonzero(info.alpha[:, j])) for j in range(len(info.status))], \
           [int(np.count_nonzero(info.beta[:, j])) for j in range(len(info.status))]


@functools.lru_cache(maxsize=None)
def _want(k, seed, zero_column, maxiter):
    H, Q, r = system("small")
    D = rhs(H.shape[0], k, seed, zero_column)
    return D, restate_cg_coef(H, Q, diag_csr(r), D, TOL, maxiter)


@pytest.fixture(scope="module")
def small(ctx):
    H, Q, r = system("small")
    hs = [ctx.csr_from_scipy(M) for M in (H, Q, diag_csr(r))]
    yield hs
    for hd in hs:
        hd.close()


# ------------------------------------------------------------------ probes
@pytest.mark.parametrize("n,k", [(1, 1), (5, 3), (2049, 2), (4097, 65)])
def test_probe_fill_is_the_hash_bit_for_bit(ctx, n, k):
    import torch
    dev = torch.device("cuda", ctx.device)
    for seed in (0, (1 << 63) + 5):
        want = restate_probes(n, k, seed)
        x = torch.full((n, k), np.nan, dtype=torch.float64, device=dev)
        ctx.probe_fill_into(x, k, n, k, seed)
        assert _same_bits(x.cpu().numpy(), want), f"packed n={n} k={k} seed={seed}"
        ld = k + 3                                                  # padding poisoned, and left as it was
        x = torch.full((n, ld), -7.25, dtype=torch.float64, device=dev)
        ctx.probe_fill_into(x, ld, n, k, seed)
        got = x.cpu().numpy()
        assert _same_bits(got[:, :k], want) and np.all(got[:, k:] == -7.25), f"ldx={ld} n={n} k={k} seed={seed}"
        flat = torch.full((n * k + 2,), -7.25, dtype=torch.float64, device=dev)   # a base 8 bytes off a 16-byte boundary
        assert flat.data_ptr() % 16 == 0
        ctx.probe_fill_into(flat.data_ptr() + 8, k, n, k, seed)
        got = flat.cpu().numpy()
        assert got[0] == -7.25 and got[-1] == -7.25 and _same_bits(got[1:-1].reshape(n, k), want), f"offset n={n} k={k} seed={seed}"
    # the probes of a batch: columns m .. m + k of a wider block are the same probes (what innovation_logdet does)
    x = torch.full((n, k + 1), -7.25, dtype=torch.float64, device=dev)
    ctx.probe_fill_into(x.data_ptr() + 8, k + 1, n, k, SEED)
    got = x.cpu().numpy()
    assert np.all(got[:, 0] == -7.25) and _same_bits(got[:, 1:], restate_probes(n, k, SEED))


def test_probe_fill_refuses_bad_arguments(ctx):
    import torch
    x = torch.zeros((4, 4), dtype=torch.float64, device=torch.device("cuda", ctx.device))
    vp = ctypes.c_void_p
    f = ctx.lib.smm_probe_fill
    assert f(ctx.handle, 4, 4, 1, vp(x.data_ptr()), 4) == 0
    assert f(ctx.handle, 0, 4, 1, vp(0), 4) == 0 and f(ctx.handle, 4, 0, 1, vp(0), 0) == 0
    for n, k, p, ld in ((4, 4, 0, 4), (4, 4, x.data_ptr(), 3), (-1, 4, x.data_ptr(), 4), (4, -1, x.data_ptr(), 4)):
        assert f(ctx.handle, n, k, 1, vp(p), ld) == -2, (n, k, p, ld)
    ctx.synchronize()


# ------------------------------------------------------------------ recorded coefficients
@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_exact_coefficients_at_every_width(ctx, small, k):
    zero = {1: None, 2: 1, 5: 2, 16: 2}[k]
    D, want = _want(k, 30 + k, zero, 200)
    got = _solve(ctx, small, D, 200)
    _assert_exact(got, want, f"k={k}")
    info = got[1]
    assert info.alpha.shape == (200, k) and info.beta.shape == (200, k)
    na, nb = _history_counts(info)
    for j in range(k):
        m = int(info.iterations[j])
        assert info.status[j] == CONVERGED and na[j] == m and nb[j] == max(m - 1, 0), (j, m, na[j], nb[j])
        assert not info.alpha[m:, j].any() and not info.beta[max(m - 1, 0):, j].any()
        assert not np.signbit(info.alpha[m:, j]).any() and not np.signbit(info.beta[max(m - 1, 0):, j]).any()     # +0.0
    if zero is not None:
        assert info.iterations[zero] == 0 and na[zero] == 0 and nb[zero] == 0
    assert max(info.iterations) > 30


def test_iteration_limit_keeps_every_coefficient(ctx, small):
    D, want = _want(5, 35, 2, 5)
    got = _solve(ctx, small, D, 5)
    _assert_exact(got, want, "maxiter=5")
    info = got[1]
    assert info.status.tolist() == [LIMIT, LIMIT, CONVERGED, LIMIT, LIMIT] and info.iterations.tolist() == [5, 5, 0, 5, 5]
    assert _history_counts(info) == ([5, 5, 0, 5, 5], [5, 5, 0, 5, 5])


def test_breakdown_ends_the_history_where_the_contract_says(ctx, small):
    """R = -10 I (test_indefinite_system_breaks_down_without_harming_the_rest of test_gpu_cg.py): random columns break down
    in iteration m + 1 after m alphas and m betas; the column between them converges and equals its own solve."""
    h, q, _ = small
    H, Q, _ = system("small")
    n = H.shape[0]
    lam, V = np.linalg.eigh((H @ Q @ H.T).toarray() - 10.0 * np.eye(n))
    assert lam[0] < 0 < lam[-1]
    D = rhs(n, 3, 62)
    D[:, 1] = V[:, -2:] @ np.array([1.0, 3.0])
    R = diag_csr(np.full(n, -10.0))
    want = restate_cg_coef(H, Q, R, D, TOL, 200)
    assert want[1].status.tolist() == [BREAKDOWN, CONVERGED, BREAKDOWN]
    rr = ctx.csr_from_scipy(R)
    try:
        got = _solve(ctx, (h, q, rr), D, 200)
        _assert_exact(got, want, "indefinite")
        info = got[1]
        na, nb = _history_counts(info)
        it = info.iterations.tolist()
        assert na == it and nb == [it[0], it[1] - 1, it[2]], (it, na, nb)
        for j in range(3):
            alone = _solve(ctx, (h, q, rr), D[:, j:j + 1], 200)
            assert _same_bits(alone[0][:, 0], got[0][:, j]), j
            for f in FIELDS + HIST:
                a, b = getattr(alone[1], f), getattr(info, f)
                assert _same_bits(a[..., 0], b[..., j]), (j, f)
    finally:
        rr.close()
    # R = -0.3 I: the same columns get five iterations in before p^T (S + R) p turns negative in the sixth
    R, D = diag_csr(np.full(n, -0.3)), rhs(n, 3, 62)
    want = restate_cg_coef(H, Q, R, D, TOL, 200)
    assert want[1].status.tolist() == [BREAKDOWN] * 3 and want[1].iterations.tolist() == [5, 5, 5]
    rr = ctx.csr_from_scipy(R)
    try:
        got = _solve(ctx, (h, q, rr), D, 200)
        _assert_exact(got, want, "indefinite, late")
        assert _history_counts(got[1]) == ([5, 5, 5], [5, 5, 5])
    finally:
        rr.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_column_blocks_and_forced_classes(ctx, small, mode):
    h, q, r = small
    n, K = h.rows, h.cols
    D, want = _want(5, 35, 2, 200)
    try:
        ctx.tune_spmm(mode)
        _assert_exact(_solve(ctx, small, D, 200), want, f"mode={mode}")
        # a budget for two columns per block (5 -> 2, 2, 1), then one byte (one column per block)
        for budget in (2 * (5 * n + 2 * K) * 8, 1):
            ctx.tune_spmm(mode, budget)
            _assert_exact(_solve(ctx, small, D, 200), want, f"mode={mode} budget={budget}")
    finally:
        ctx.tune_spmm(0, 0)


@pytest.mark.parametrize("k", [1, 5])
def test_kronecker_q(ctx, k):
    H, D, E, R, rhs_ = kron_system()
    B = rhs_[:, :k]
    want = restate_cg_coef(H, None, R, B, TOL, 300, apply=lambda P: restate_triple_kron(H, D, E, P) + restate_spmm(R, P))
    hs = [ctx.csr_from_scipy(M) for M in (H, D, E, R)]
    try:
        _assert_exact(_solve(ctx, hs, B, 300), want, f"kron k={k}")
        assert want[1].iterations.max() >= 3 and np.count_nonzero(want[1].alpha) == want[1].iterations.sum()
        if k == 5:
            try:
                ctx.tune_spmm(0, 1)                                 # one column per block
                _assert_exact(_solve(ctx, hs, B, 300), want, "kron, one column per block")
            finally:
                ctx.tune_spmm(0, 0)
    finally:
        for hd in hs:
            hd.close()


# ------------------------------------------------------------------ the public function
def test_right_hand_sides_in_the_batch_get_the_bits_of_innovation_solve():
    import torch
    from sparse_matrix_mult import innovation_logdet, innovation_solve
    from sparse_matrix_mult_amd import KroneckerOperand, pin_operand, set_exact, set_result_device
    dev = torch.device("cuda", 0)
    H, Q, r = system("small")
    D = rhs(H.shape[0], 5, 35, 2)
    Hk, Dk, Ek, Rk, rhs_k = kron_system()
    old = set_exact(True)
    try:
        def check(ops, d, what):
            Z, info = innovation_solve(*ops, d, tol=TOL)
            res = innovation_logdet(*ops, probes=3, seed=SEED, tol=TOL, d=d, return_solutions=True)
            print(what, res)
            assert type(res.Z) is type(Z) and tuple(res.Z.shape) == tuple(Z.shape), what
            a, b = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (res.Z, Z))
            assert _same_bits(a, b), f"{what}: Z differs"
            for f in FIELDS:
                assert _same_bits(getattr(res.info_d, f), getattr(info, f)), (what, f)
            assert res.info.converged and res.positive_definite and np.all(np.isfinite(res.samples))
            return res

        res = check((H, Q, r), D, "numpy d")
        assert isinstance(res.solutions, np.ndarray) and res.solutions.shape == (H.shape[0], 3)
        # Psi times the solutions gives the probes back
        back = H @ (Q @ (H.T @ res.solutions)) + r[:, None] * res.solutions
        assert np.max(np.abs(back - restate_probes(H.shape[0], 3, SEED))) <= 1e-6
        check((H, Q, r), D[:, 0].copy(), "1-D numpy d")
        ph, pq, pr = pin_operand(H), pin_operand(Q), pin_operand(diag_csr(r))
        check((ph, pq, pr), D, "PinnedOperands")
        for p in (ph, pq, pr):
            p.unpin()
        check((Hk, KroneckerOperand(Dk, Ek), Rk), rhs_k, "KroneckerOperand")
        old_dev = set_result_device(True)
        try:
            res = check((H, Q, r), torch.from_numpy(D).to(dev), "tensor d, set_result_device")
            assert torch.is_tensor(res.Z) and res.Z.is_cuda and torch.is_tensor(res.solutions) and res.solutions.is_cuda
            check((Hk, KroneckerOperand(Dk, Ek), Rk), torch.from_numpy(rhs_k).to(dev), "KroneckerOperand, tensor d")
        finally:
            set_result_device(old_dev)
    finally:
        set_exact(old)


@pytest.mark.parametrize("name,probes", [("small", 32), ("stiff", 8)])
def test_default_mode_against_the_dense_eigendecomposition(name, probes):
    """Every sample within a relative 1e-9 of z_c^T ln(Psi) z_c, the estimate within 3 standard errors of slogdet, and two
    runs with the same bits.  The restatement alone (CPU, tests/slq_restatement.py, tol 1e-8, seed 12345) gives:
      small, 32 probes: 54 iterations, largest relative error of a sample 2.1e-15, 1907.060 +- 6.820 against 1899.214 (1.15 se)
      stiff,  8 probes: 186-187 iterations, largest relative error 1.8e-14, -1164.268 +- 44.485 against -1207.423 (0.97 se)
    Default mode differs from it by fusion and the products' summation order, a perturbation of order eps * cond."""
    from sparse_matrix_mult import innovation_logdet
    H, Q, r = system(name)
    n = H.shape[0]
    lam, _, logdet = dense_log(name)
    want = exact_samples(name, restate_probes(n, probes, SEED))
    res = innovation_logdet(H, Q, r, probes=probes, seed=SEED, tol=TOL)
    rel = np.abs(res.samples - want) / np.abs(want)
    print(name, res, "iterations", res.info.iterations.min(), "..", res.info.iterations.max())
    print(name, "largest relative error of a sample", rel.max(), "logdet", logdet, "error in standard errors", (res.logdet - logdet) / res.stderr)
    assert res.info.converged and res.positive_definite
    assert np.all(rel <= 1e-9)
    assert abs(res.logdet - logdet) <= 3 * res.stderr
    assert res.logdet == float(np.mean(res.samples)) and res.stderr == float(np.std(res.samples, ddof=1) / np.sqrt(probes))
    assert lam[0] * (1 - 1e-8) <= res.lambda_min and abs(res.lambda_max - lam[-1]) <= 1e-8 * lam[-1]
    again = innovation_logdet(H, Q, r, probes=probes, seed=SEED, tol=TOL)
    for f in HIST + FIELDS:
        assert _same_bits(getattr(again.info, f), getattr(res.info, f)), f"run to run: {f}"
    assert _same_bits(again.samples, res.samples), "run to run: samples"


# ------------------------------------------------------------------ failures
def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_innovation_solve_coef (H^T built inside the call) made to fail at its 1st, 2nd, ... device allocation (hard) until
    it succeeds -- the two histories are the last pool blocks it takes: each failure is SMM_ERR_ALLOC with nothing handed
    out, and the call that succeeds is exact."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    H, Q, r = system("small")
    D, want = _want(2, 32, 1, 200)
    handles = [c.csr_from_scipy(M) for M in (H, Q, diag_csr(r))]
    try:
        failures = 0
        for nth in range(1, 65):
            c.release_pool()
            c.inject_alloc_failure(nth, hard=True)
            try:
                res = _solve(c, handles, D, 200)
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
        # r, p, w, R p, two intermediates, partials, scalars and the two histories alone are ten pool blocks
        assert failures >= 10, f"only {failures} allocations failed"
    finally:
        for hd in handles:
            hd.close()
        c.close()


def test_bad_arguments_are_refused(ctx, small):
    import torch
    dev = torch.device("cuda", ctx.device)
    h, q, r = small
    n = h.rows
    B = torch.ones((n, 4), dtype=torch.float64, device=dev)
    X = torch.full((n, 4), -7.25, dtype=torch.float64, device=dev)
    it, st = np.zeros(4, np.int32), np.zeros(4, np.int32)
    rs, bs = np.zeros(4), np.zeros(4)
    al, be = np.full((10, 4), -7.25), np.full((10, 4), -7.25)
    vp = ctypes.c_void_p
    outs = [vp(a.ctypes.data) for a in (it, st, rs, bs, al, be)]

    def call(k=4, b=B.data_ptr(), ldb=4, x=X.data_ptr(), ldx=4, tol=1e-8, maxiter=10, o=outs, flags=0):
        return ctx.lib.smm_innovation_solve_coef(ctx.handle, h.handle, q.handle, r.handle, flags, k, vp(b), ldb, vp(x), ldx, tol, maxiter, *o)
    for kw in ({"maxiter": 0}, {"maxiter": 65537}, {"maxiter": -1}, {"o": outs[:4] + [vp(0), outs[5]]}, {"o": outs[:5] + [vp(0)]},
               {"ldb": 3}, {"ldx": 3}, {"tol": float("nan")}, {"tol": float("inf")}, {"tol": 0.0}, {"x": 0}, {"b": 0}, {"flags": 16},
               {"k": -1}):
        assert call(**kw) == -2, kw
    ctx.synchronize()
    assert np.all(al == -7.25) and np.all(be == -7.25) and np.all(X.cpu().numpy() == -7.25), "a refused call wrote something"
    assert call() == 0 and np.all(it == 10) and np.all(al > 0)          # (and the same arguments, legal, run)
    H, D, E, R, _ = kron_system()
    hs = [ctx.csr_from_scipy(M) for M in (H, D, E, R)]
    try:
        Bk = torch.ones((H.shape[0], 4), dtype=torch.float64, device=dev)
        Xk = torch.zeros((H.shape[0], 4), dtype=torch.float64, device=dev)

        def callk(maxiter=10, o=outs, ldx=4, tol=1e-8):
            return ctx.lib.smm_innovation_solve_coef_kron(ctx.handle, *[t.handle for t in hs], 0, 4, vp(Bk.data_ptr()), 4, vp(Xk.data_ptr()),
                                                          ldx, tol, maxiter, *o)
        for kw in ({"maxiter": 0}, {"maxiter": 65537}, {"o": outs[:4] + [vp(0), outs[5]]}, {"o": outs[:5] + [vp(0)]}, {"ldx": 3},
                   {"tol": float("inf")}):
            assert callk(**kw) == -2, kw
        assert callk() == 0
    finally:
        for hd in hs:
            hd.close()
