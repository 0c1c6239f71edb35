"""Sparse x dense products on the device (smm_spmm, smm_triple_apply; Context.spmm_*, Context.triple_apply_*,
sparse_dense_multiply, triple_product_apply).

Contract checked here: under SMM_EXACT, Y = op(A) X is bit-identical to the stored-order loop (tests/spmm_restatement.py)
and to scipy, for every kernel class forced and for auto; in default mode it is within 1e-10 of (|A||X|)[i,j] and two runs
agree bit for bit.  +0.0 for empty rows and lone -0.0 products, no inf through a missing entry, padding columns untouched,
value updates reach the cached transpose, and H (Q (H^T X)) equals scipy bit for bit under any column blocking."""
import numpy as np
import pytest
import scipy.sparse as sp

from spmm_restatement import op_rows, operands, raw_csr, restate_spmm, restate_triple

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
RTOL = 1e-10
MODES = [0, 1, 2, 3]          # auto, tiny, group, long
WIDTHS = [0, 1, 2, 3, 7, 8, 63, 64, 65, 130, 256, 1000]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _assert_bits(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max abs diff {np.max(np.abs(got - want)) if got.size else 0:.3e}"


def _abs(A):
    """|A| on A's own arrays (scipy's abs() would merge repeated columns of A in place)."""
    return raw_csr(A.indptr, A.indices, np.abs(A.data), A.shape)


def _rows(A, rows):
    """The given rows of A as a CSR, entries in A's stored order (built by hand: scipy's indexing may reorder)."""
    lens = np.diff(A.indptr)[rows]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    take = np.concatenate([np.arange(A.indptr[r], A.indptr[r + 1]) for r in rows])
    return raw_csr(ptr, A.indices[take], A.data[take], (len(rows), A.shape[1]))


def _assert_close(got, want, A, X, transpose, what):
    op = _abs(A).T if transpose else _abs(A)
    mag = np.asarray(op @ np.abs(X))
    assert np.all(np.abs(got - want) <= RTOL * mag), f"{what}: beyond 1e-10 (|A||X|)"


def _widths(name):
    return WIDTHS if name in ("uniform", "unsorted_dup", "empty_rows", "boundaries") else [0, 1, 3, 8, 65]


@pytest.mark.parametrize("name", list(operands()))
def test_every_class_and_width_against_the_restatement(ctx, name):
    A = operands()[name]
    a = ctx.csr_from_scipy(A)
    rng = np.random.default_rng(11)
    try:
        for transpose in (False, True):
            kx = op_rows(A, not transpose)
            for k in _widths(name):
                X = rng.standard_normal((kx, k))
                want = restate_spmm(A, X, transpose)
                for mode in MODES:
                    if name == "power_law" and mode == 1 and k > 8:
                        continue                  # (a 100 000-entry row on 4 lanes: correct, just slow; k <= 8 covers it)
                    ctx.tune_spmm(mode)
                    try:
                        got = ctx.spmm_host(a, X, transpose=transpose, exact=True)
                        _assert_bits(got, want, f"{name} exact T={transpose} k={k} mode={mode}")
                        got = ctx.spmm_host(a, X, transpose=transpose, exact=False)
                        _assert_close(got, want, A, X, transpose, f"{name} default T={transpose} k={k} mode={mode}")
                        again = ctx.spmm_host(a, X, transpose=transpose, exact=False)
                        _assert_bits(again, got, f"{name} default run-to-run T={transpose} k={k} mode={mode}")
                    finally:
                        ctx.tune_spmm(0)
            if k:
                want = (A.T @ X) if transpose else (A @ X)      # scipy itself, last width
                _assert_bits(ctx.spmm_host(a, X, transpose=transpose, exact=True), np.asarray(want), f"{name} scipy T={transpose}")
    finally:
        a.close()


def test_exact_equals_the_sparse_sparse_dense_product(ctx):
    """On an X without zeros: bit-identical to sparse_matrix_multiply(A, csr_matrix(X), 'dense') under set_exact."""
    from sparse_matrix_mult_amd import set_exact, sparse_matrix_multiply
    A = operands()["uniform"]
    X = np.random.default_rng(3).uniform(0.5, 1.5, (A.shape[1], 17))
    old = set_exact(True)
    try:
        want = sparse_matrix_multiply(A, sp.csr_matrix(X), output_format="dense")
        a = ctx.csr_from_scipy(A)
        _assert_bits(ctx.spmm_host(a, X, exact=True), want, "spmm vs dense SpGEMM")
        a.close()
    finally:
        set_exact(old)


def test_signed_zeros_and_infinities(ctx):
    # row 0: -1 x 0.0 alone; row 1: empty; row 2: stores column 1 only, while X[0, :] holds inf
    A = raw_csr([0, 1, 1, 2], [0, 1], [-1.0, 2.0], (3, 2))
    for k in (1, 2, 5, 64):
        X = np.zeros((2, k))
        a = ctx.csr_from_scipy(A)
        for mode in MODES:
            ctx.tune_spmm(mode)
            for exact in (False, True):
                Y = ctx.spmm_host(a, X, exact=exact)
                assert np.array_equal(_bits(Y), np.zeros((3, k), dtype=np.int64)), f"k={k} mode={mode}: not +0.0"
                Xi = X.copy()
                Xi[0, :] = np.inf
                Xi[1, :] = 1.5
                Y = ctx.spmm_host(a, Xi, exact=exact)
                assert np.all(np.isinf(Y[0])) and np.all(Y[1] == 0.0) and np.all(Y[2] == 3.0), f"k={k} mode={mode}"
        ctx.tune_spmm(0)
        a.close()


def test_strides_leave_the_padding_untouched(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    A = operands()["unsorted_dup"]
    a = ctx.csr_from_scipy(A)
    rng = np.random.default_rng(5)
    try:
        for transpose in (False, True):
            m, kx = op_rows(A, transpose), op_rows(A, not transpose)
            for k, ldx, ldy in ((1, 3, 2), (7, 9, 8), (8, 11, 10), (64, 64, 67), (65, 70, 66)):
                Xp = rng.standard_normal((kx, ldx))
                want = restate_spmm(A, Xp[:, :k], transpose)
                for mode in MODES:
                    ctx.tune_spmm(mode)
                    for exact in (True, False):
                        dx = torch.from_numpy(Xp).to(dev)
                        dy = torch.full((m, ldy), -7.25, dtype=torch.float64, device=dev)
                        ctx.spmm_into(a, dx, ldx, k, dy, ldy, transpose=transpose, exact=exact)
                        Y = dy.cpu().numpy()
                        assert np.all(Y[:, k:] == -7.25), f"padding written: k={k} ldy={ldy} mode={mode}"
                        if exact:
                            _assert_bits(Y[:, :k], want, f"strided k={k} mode={mode}")
                        else:
                            _assert_close(Y[:, :k], want, A, Xp[:, :k], transpose, f"strided k={k} mode={mode}")
                ctx.tune_spmm(0)
    finally:
        a.close()


@pytest.mark.parametrize("shift_x,shift_y", [(1, 0), (0, 1), (1, 1)])
def test_views_one_double_into_an_aligned_buffer(ctx, shift_x, shift_y):
    """X, Y or both start 8 bytes into a 16-byte aligned buffer, with even k, ldx and ldy: the 16-byte path must not be
    taken on them.  Bits against the restatement under exact; the padding, the element before the view and the tail
    keep the sentinel."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(6)
    for name in ("unsorted_dup", "boundaries"):
        A = operands()[name]
        a = ctx.csr_from_scipy(A)
        try:
            for transpose in (False, True):
                m, kx = op_rows(A, transpose), op_rows(A, not transpose)
                for k, ldx, ldy in ((2, 2, 2), (8, 10, 12), (64, 64, 66)):
                    Xp = rng.standard_normal((kx, ldx))
                    want = restate_spmm(A, Xp[:, :k], transpose)
                    xbuf = torch.zeros(kx * ldx + 2, dtype=torch.float64, device=dev)
                    xbuf[shift_x:shift_x + kx * ldx] = torch.from_numpy(Xp.ravel()).to(dev)
                    dx = xbuf[shift_x:shift_x + kx * ldx]
                    for mode in MODES:
                        ctx.tune_spmm(mode)
                        for exact in (True, False):
                            ybuf = torch.full((m * ldy + 2,), -7.25, dtype=torch.float64, device=dev)
                            dy = ybuf[shift_y:shift_y + m * ldy]
                            assert xbuf.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0
                            assert dx.data_ptr() % 16 == 8 * shift_x and dy.data_ptr() % 16 == 8 * shift_y
                            ctx.spmm_into(a, dx, ldx, k, dy, ldy, transpose=transpose, exact=exact)
                            flat = ybuf.cpu().numpy()
                            what = f"{name} T={transpose} k={k} ldy={ldy} mode={mode}"
                            assert np.all(flat[:shift_y] == -7.25) and np.all(flat[shift_y + m * ldy:] == -7.25), f"outside the view: {what}"
                            Y = flat[shift_y:shift_y + m * ldy].reshape(m, ldy)
                            assert np.all(Y[:, k:] == -7.25), f"padding written: {what}"
                            if exact:
                                _assert_bits(Y[:, :k], want, what)
                            else:
                                _assert_close(Y[:, :k], want, A, Xp[:, :k], transpose, what)
                    ctx.tune_spmm(0)
        finally:
            ctx.tune_spmm(0)
            a.close()


def test_bad_arguments_are_refused(ctx):
    import torch
    from sparse_matrix_mult_amd.engine import SmmError
    dev = torch.device("cuda", ctx.device)
    A = operands()["uniform"]
    a = ctx.csr_from_scipy(A)
    X = torch.zeros((A.shape[1], 4), dtype=torch.float64, device=dev)
    Y = torch.zeros((A.shape[0], 4), dtype=torch.float64, device=dev)
    lib = ctx.lib
    import ctypes
    vp = ctypes.c_void_p
    try:
        for flags, k, ldx, ldy in ((1, 4, 4, 4), (4 | 2, 4, 4, 4), (0, 4, 3, 4), (0, 4, 4, 3), (0, -1, 4, 4)):
            assert lib.smm_spmm(ctx.handle, a.handle, flags, k, vp(X.data_ptr()), ldx, vp(Y.data_ptr()), ldy) == -2
        assert lib.smm_spmm(ctx.handle, a.handle, 0, 4, vp(0), 4, vp(Y.data_ptr()), 4) == -2
        B = torch.zeros((A.shape[0] + A.shape[1], 4), dtype=torch.float64, device=dev)      # X and Y inside one buffer
        assert lib.smm_spmm(ctx.handle, a.handle, 0, 4, vp(B.data_ptr()), 4, vp(B.data_ptr() + 8 * 4 * 10), 4) == -2
        assert lib.smm_spmm(ctx.handle, a.handle, 0, 0, vp(0), 0, vp(0), 0) == 0                  # k = 0: nothing to do
        assert lib.smm_triple_apply(ctx.handle, a.handle, a.handle, 16, 1, vp(X.data_ptr()), 1, vp(Y.data_ptr()), 1) == -2
        with pytest.raises(SmmError):
            ctx.tune_spmm(4)
    finally:
        a.close()


def test_value_update_reaches_the_transposed_product(ctx):
    A = operands()["unsorted_dup"].copy()
    a = ctx.csr_from_scipy(A)
    X = np.random.default_rng(8).standard_normal((A.shape[0], 6))
    try:
        _assert_bits(ctx.spmm_host(a, X, transpose=True, exact=True), restate_spmm(A, X, True), "before update")
        A.data = np.random.default_rng(9).uniform(-2, 2, A.nnz)
        a.update_values(A.data)
        _assert_bits(ctx.spmm_host(a, X, transpose=True, exact=True), restate_spmm(A, X, True), "after update")
    finally:
        a.close()


def test_public_interfaces(ctx):
    import torch
    import sparse_matrix_mult
    from sparse_matrix_mult_amd import pin_operand, set_exact, set_result_device
    dev = torch.device("cuda", 0)
    A = operands()["empty_rows"]
    rng = np.random.default_rng(12)
    X = rng.standard_normal((A.shape[1], 5))
    x1 = rng.standard_normal(A.shape[1])
    old = set_exact(True)
    try:
        f = sparse_matrix_mult.sparse_dense_multiply
        Y = f(A, X)
        assert isinstance(Y, np.ndarray)
        _assert_bits(Y, np.asarray(A @ X), "numpy")
        y = f(A, x1)
        assert y.shape == (A.shape[0],)
        _assert_bits(y, np.asarray(A @ x1), "1-D")
        Yt = f(A, torch.from_numpy(X).to(dev))
        assert torch.is_tensor(Yt) and Yt.is_cuda
        _assert_bits(Yt.cpu().numpy(), np.asarray(A @ X), "torch")
        Z = rng.standard_normal((A.shape[0], 3))
        _assert_bits(f(A, Z, transpose=True), np.asarray(A.T @ Z), "transpose")
        _assert_bits(f(A, Z.tolist(), transpose=True), np.asarray(A.T @ Z), "list input")
        assert f(A, np.zeros((A.shape[1], 0))).shape == (A.shape[0], 0)
        p = pin_operand(A)
        _assert_bits(f(p, X), np.asarray(A @ X), "PinnedOperand")
        _assert_bits(f(p, Z, transpose=True), np.asarray(A.T @ Z), "PinnedOperand transposed")
        p.unpin()
        old_dev = set_result_device(True)
        try:
            Yd = f(A, X)
            assert torch.is_tensor(Yd) and Yd.is_cuda
            _assert_bits(Yd.cpu().numpy(), np.asarray(A @ X), "set_result_device")
        finally:
            set_result_device(old_dev)
        H = operands()["uniform"]
        K = H.shape[1]
        Q = sp.random(K, K, density=0.05, format="csr", random_state=np.random.default_rng(13))
        W = rng.standard_normal((H.shape[0], 4))
        g = sparse_matrix_mult.triple_product_apply
        _assert_bits(g(H, Q, W), H @ (Q @ (H.T @ W)), "triple_product_apply")
        _assert_bits(g(H, Q, torch.from_numpy(W).to(dev)).cpu().numpy(), H @ (Q @ (H.T @ W)), "triple_product_apply torch")
        w1 = W[:, 0].copy()
        _assert_bits(g(H, Q, w1), H @ (Q @ (H.T @ w1)), "triple_product_apply 1-D")
    finally:
        set_exact(old)


@pytest.mark.parametrize("budget", [0, 1])
def test_triple_apply_exact_and_blocked(ctx, budget):
    """Exact: bit-identical to scipy's H @ (Q @ (H.T @ X)) (Q not symmetric); a budget that forces column blocks of one
    column (budget 1 byte) changes no bit."""
    rng = np.random.default_rng(21)
    for hname in ("uniform", "unsorted_dup", "empty_rows"):
        H = operands()[hname]
        K = H.shape[1]
        Q = sp.random(K, K, density=0.04, format="csr", random_state=rng)
        Q.data = rng.uniform(-1, 1, Q.nnz)
        h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
        ctx.tune_spmm(0, budget)
        try:
            for k in (1, 3, 8, 65):
                X = rng.standard_normal((H.shape[0], k))
                want = H @ (Q @ (H.T @ X))
                _assert_bits(ctx.triple_apply_host(h, q, X, exact=True), want, f"{hname} k={k}")
                _assert_bits(restate_triple(H, Q, X), want, "restatement")
                got = ctx.triple_apply_host(h, q, X, exact=False)
                assert np.allclose(got, want, rtol=1e-9, atol=1e-12), f"{hname} default k={k}"
        finally:
            ctx.tune_spmm(0, 0)
            h.close(); q.close()


def test_large_output_beyond_2_31_elements(ctx):
    """Y with 2^25 x 65 > 2^31 elements (17 GB, on the device only), 2 entries per row: sampled rows and the last rows
    against the restatement."""
    import torch
    dev = torch.device("cuda", ctx.device)
    m, K, k = 1 << 25, 1024, 65
    rng = np.random.default_rng(31)
    idx = rng.integers(0, K, 2 * m).astype(np.int32)
    val = rng.uniform(-1, 1, 2 * m)
    ptr = np.arange(0, 2 * m + 1, 2, dtype=np.int32)
    A = raw_csr(ptr, idx, val, (m, K))
    X = rng.standard_normal((K, k))
    a = ctx.csr_from_scipy(A)
    dx = torch.from_numpy(X).to(dev)
    dy = torch.empty((m, k), dtype=torch.float64, device=dev)
    try:
        sample = np.concatenate([rng.integers(0, m, 2000), np.arange(m - 64, m)])
        sub = _rows(A, sample)
        want = restate_spmm(sub, X)
        for exact in (True, False):
            ctx.spmm_into(a, dx, k, k, dy, k, exact=exact)
            got = dy[torch.from_numpy(sample).to(dev)].cpu().numpy()
            if exact:
                _assert_bits(got, want, "large exact")
            else:
                _assert_close(got, want, sub, X, False, "large default")
    finally:
        del dy
        torch.cuda.empty_cache()
        a.close()


def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_spmm_host (plain and transposed, the transpose built inside the call) and smm_triple_apply_host, made to fail
    at their 1st, 2nd, ... device allocation (hard) until they succeed: each failure is SMM_ERR_ALLOC with nothing handed
    out, and the call that finally succeeds is exact."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    A = operands()["unsorted_dup"]
    K = A.shape[1]
    Q = sp.random(K, K, density=0.05, format="csr", random_state=np.random.default_rng(41))
    rng = np.random.default_rng(42)
    X, Xt, W = rng.standard_normal((A.shape[1], 6)), rng.standard_normal((A.shape[0], 6)), rng.standard_normal((A.shape[0], 3))
    handles = []
    try:
        a_plain, a_tr, h_tr, q = (c.csr_from_scipy(M) for M in (A, A, A, Q))       # (uploads allocate too: before the sweep)
        handles += [a_plain, a_tr, h_tr, q]
        cases = [
            ("spmm_host", lambda: c.spmm_host(a_plain, X, exact=True), restate_spmm(A, X)),
            ("spmm_host transposed", lambda: c.spmm_host(a_tr, Xt, transpose=True, exact=True), restate_spmm(A, Xt, True)),
            ("triple_apply_host", lambda: c.triple_apply_host(h_tr, q, W, exact=True), A @ (Q @ (A.T @ W))),
        ]
        for name, call, want in cases:
            failures = 0
            for nth in range(1, 65):
                c.release_pool()
                c.inject_alloc_failure(nth, hard=True)
                try:
                    res = call()
                except SmmError as e:
                    assert e.code == -3, f"{name}, allocation {nth}: {e}"
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
            assert failures >= 3, f"{name}: only {failures} allocations failed"
    finally:
        for hd in handles:
            hd.close()
        c.close()
