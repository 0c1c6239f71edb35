"""The sampled dense product on the GPU against its numpy restatement (tests/sddmm_restatement.py): every mask shape,
every width at which the lane-group size or the number of tiles changes, both kernel classes, both modes.

Bounds.  SMM_EXACT is compared bit for bit.  The default mode is held to the contract's 1e-10 (|X| |Y|^T)[i,j] (times |w|)
around the exact restatement, whose own rounding error is at most k u (|X| |Y|^T)[i,j] < 3e-14 of that scale at k = 257,
and -- beyond the contract's bound -- to the bits of the documented summation order."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from sddmm_restatement import KS, bound, dense, entries, masks, operands, raw_csr, restate_default, restate_exact

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

CLASSES = (0, 1, 2)          # smm_ctx_tune_sddmm: auto, interleaved entries, runs of entries


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert np.all(same), f"{what}: {int((~same).sum())} of {same.size} values differ, first at {int(np.flatnonzero(~same.ravel())[0])}"


@functools.lru_cache(maxsize=None)
def _reference(name, k):
    """(rows, cols, w, exact, exact scaled, default, default scaled, bound, bound scaled), computed once."""
    M, X, Y = operands(name, k)
    rows, cols, w = entries(M)
    return (rows, cols, w, restate_exact(X, Y, rows, cols), restate_exact(X, Y, rows, cols, w), restate_default(X, Y, rows, cols),
            restate_default(X, Y, rows, cols, w), bound(X, Y, rows, cols), bound(X, Y, rows, cols, w))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(masks()))
def test_every_mask_width_class_and_mode(ctx, name, k):
    M, X, Y = operands(name, k)
    rows, cols, w, ex, ex_w, df, df_w, bd, bd_w = _reference(name, k)
    y_arg = None if Y is X else Y                    # Y = X goes in as the same buffer
    mask = ctx.csr_from_scipy(M)
    try:
        for scale, want_exact, want_default, bnd in ((False, ex, df, bd), (True, ex_w, df_w, bd_w)):
            first = None
            for cls in CLASSES:
                ctx.tune_sddmm(cls)
                got = ctx.sddmm_host(mask, X, y_arg, scale=scale, exact=True)
                _assert_bits(got, want_exact, f"{name} k={k} scale={scale} class {cls} exact")
                got = ctx.sddmm_host(mask, X, y_arg, scale=scale)
                err = np.abs(got - want_exact)
                print(name, k, scale, cls, "max error / bound", float(np.max(err / np.maximum(bnd, 1e-300))) if err.size else 0.0)
                assert np.all(err <= 1e-10 * bnd), f"{name} k={k} scale={scale} class {cls} default"
                if first is None:
                    first = got
                    _assert_bits(ctx.sddmm_host(mask, X, y_arg, scale=scale), first, "two calls")
                _assert_bits(got, first, f"{name} k={k} scale={scale}: class {cls} against class 0")
            _assert_bits(first, want_default, f"{name} k={k} scale={scale}: the documented order")
    finally:
        ctx.tune_sddmm(0)
        mask.close()


@pytest.mark.parametrize("k", [3, 64, 130])
def test_a_position_shared_by_two_masks_has_the_same_bits(ctx, k):
    """Default mode: the order depends on k only -- not on the mask, the row's length or the entry's place in its row."""
    A, B = masks()["arrow"], masks()["band"][:300, :300].tocsr()
    X, Y = dense(300, k, 31), dense(300, k, 32)
    found = {}
    for M in (A, B):
        h = ctx.csr_from_scipy(M)
        try:
            rows, cols, _ = entries(M)
            for cls in (1, 2):
                ctx.tune_sddmm(cls)
                got = ctx.sddmm_host(h, X, Y)
                for key, v in zip(zip(rows.tolist(), cols.tolist()), _bits(got).tolist()):
                    assert found.setdefault(key, v) == v, f"position {key} differs between masks / classes"
        finally:
            ctx.tune_sddmm(0)
            h.close()
    assert len(found) < A.nnz + B.nnz, "the two masks share positions"


@pytest.mark.parametrize("layout", ["column_slice", "odd_ld", "offset_one_double", "same_buffer"])
@pytest.mark.parametrize("k", [8, 63, 130])
def test_device_layouts(ctx, layout, k):
    """Torch operands used in place: a column slice of a wider tensor (ld > k), an odd leading dimension, a base one
    double into an aligned buffer -- every branch of the 16-byte load rule -- and Y = X as one buffer."""
    import torch
    dev = torch.device("cuda", ctx.device)
    M = masks()["band" if layout == "same_buffer" else "random"]
    m, n = M.shape
    X, Y = dense(m, k, 51), dense(n, k, 52)
    if layout == "same_buffer":
        Y = X

    def place(A):
        r = A.shape[0]
        if layout == "column_slice":
            W = torch.full((r, k + 6), float("nan"), dtype=torch.float64, device=dev)
            V = W[:, 2:2 + k]
        elif layout == "odd_ld":
            ld = k + 1 if k % 2 == 0 else k + 2
            W = torch.full((r, ld), float("nan"), dtype=torch.float64, device=dev)
            V = W[:, :k]
        elif layout == "offset_one_double":
            W = torch.full((r * k + 1,), float("nan"), dtype=torch.float64, device=dev)
            V = W[1:].view(r, k)
        else:
            V = torch.empty((r, k), dtype=torch.float64, device=dev)
        V.copy_(torch.from_numpy(A).to(dev))
        return V

    dX = place(X)
    dY = dX if Y is X else place(Y)
    rows, cols, w = entries(M)
    h = ctx.csr_from_scipy(M)
    out = torch.empty(M.nnz, dtype=torch.float64, device=dev)
    try:
        for scale in (False, True):
            ww = w if scale else None
            for cls in (1, 2):
                ctx.tune_sddmm(cls)
                ctx.sddmm_into(h, dX, dX.stride(0), dY, dY.stride(0), k, out, scale=scale, exact=True)
                _assert_bits(out.cpu().numpy(), restate_exact(X, Y, rows, cols, ww), f"{layout} k={k} exact class {cls}")
                ctx.sddmm_into(h, dX, dX.stride(0), dY, dY.stride(0), k, out, scale=scale)
                _assert_bits(out.cpu().numpy(), restate_default(X, Y, rows, cols, ww), f"{layout} k={k} default class {cls}")
    finally:
        ctx.tune_sddmm(0)
        h.close()


@pytest.mark.parametrize("exact", [True, False])
def test_inf_and_nan_reach_exactly_the_entries_that_name_them(ctx, exact):
    M = masks()["two_per_row"]
    m, n = M.shape
    rows, cols, w = entries(M)
    unnamed = np.setdiff1d(np.arange(n), cols)
    assert unnamed.size, "a row of Y that no entry names"
    for k in (3, 64, 130):
        X, Y = dense(m, k, 61), dense(n, k, 62)
        X[X == 0] = 1.0                                   # (0 * inf would be NaN of its own)
        jinf, inan = int(cols[7]), int(rows[100])
        Y[jinf, k // 2] = np.inf
        X[inan, 0] = np.nan
        Y[unnamed] = np.nan
        h = ctx.csr_from_scipy(M)
        try:
            for cls in (1, 2):
                ctx.tune_sddmm(cls)
                got = ctx.sddmm_host(h, X, Y, exact=exact)
                hit = (cols == jinf) | (rows == inan)
                assert np.all(~np.isfinite(got[hit])) and np.all(np.isfinite(got[~hit])), (k, cls)
                assert np.all(np.isnan(got[rows == inan]))
                if exact:
                    _assert_bits(got, restate_exact(X, Y, rows, cols), f"k={k} class {cls}")
        finally:
            ctx.tune_sddmm(0)
            h.close()


def test_signed_zeros(ctx):
    """A lone -0.0 product gives +0.0; zero weight times an infinite sum gives NaN; a negative weight on +0.0 gives -0.0."""
    M = raw_csr([0, 3], [0, 1, 2], [1.0, 0.0, -2.0], (1, 3))
    X = np.array([[-1.0, 1.0]])
    Y = np.array([[0.0, 0.0], [np.inf, 1.0], [0.0, 0.0]])
    h = ctx.csr_from_scipy(M)
    try:
        for exact in (True, False):
            got = ctx.sddmm_host(h, X, Y, exact=exact)
            assert _bits(got)[0] == 0 and got[1] == -np.inf and _bits(got)[2] == 0
            got = ctx.sddmm_host(h, X, Y, scale=True, exact=exact)
            assert _bits(got)[0] == 0 and np.isnan(got[1]) and _bits(got)[2] == _bits(np.array([-0.0]))[0]
    finally:
        h.close()


def test_bad_arguments_are_refused(ctx):
    import torch
    from sparse_matrix_mult_amd.engine import SmmError
    dev = torch.device("cuda", ctx.device)
    M = masks()["random"]
    m, n = M.shape
    h = ctx.csr_from_scipy(M)
    X = torch.zeros((m, 4), dtype=torch.float64, device=dev)
    Y = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    C = torch.zeros(M.nnz, dtype=torch.float64, device=dev)
    big = torch.zeros(m * 4 + M.nnz, dtype=torch.float64, device=dev)
    vp = ctypes.c_void_p
    lib = ctx.lib
    try:
        for flags in (1, 2, 8, 16, 4 | 16, 32 | 64):
            assert lib.smm_sddmm(ctx.handle, h.handle, flags, 4, vp(X.data_ptr()), 4, vp(Y.data_ptr()), 4, vp(C.data_ptr())) == -2
        bad = [dict(k=-1), dict(ldx=3), dict(ldy=3), dict(d_x=0), dict(d_y=0), dict(d_c=0),
               dict(d_x=big.data_ptr(), d_c=big.data_ptr() + 8 * (m * 4 - 1)),          # the output starts on X's last element
               dict(d_y=big.data_ptr() + 8 * 10, d_c=big.data_ptr())]                   # Y starts inside the output
        for change in bad:
            args = dict(d_x=X.data_ptr(), ldx=4, d_y=Y.data_ptr(), ldy=4, k=4, d_c=C.data_ptr())
            args.update(change)
            with pytest.raises(SmmError) as e:
                ctx.sddmm_into(h, args["d_x"], args["ldx"], args["d_y"], args["ldy"], args["k"], args["d_c"])
            assert e.value.code == -2, change
        with pytest.raises(SmmError):
            ctx.tune_sddmm(3)
        with pytest.raises(SmmError):
            ctx.tune_sddmm(-1)
        ctx.sddmm_into(h, X, 4, Y, 4, 4, C)                    # and the call itself is fine
        ctx.sddmm_into(h, 0, 0, 0, 0, 0, C)                    # k = 0: X and Y hold nothing
        assert not C.cpu().numpy().any()
    finally:
        h.close()


def test_every_allocation_fails_in_turn():
    """smm_sddmm_host made to fail at its 1st, 2nd, ... device allocation: a soft failure (the first attempt only) still
    succeeds, a hard one is SMM_ERR_ALLOC, and nothing stays handed out either way."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    M, X, Y = operands("noncanonical", 8)
    rows, cols, w = entries(M)
    want = restate_exact(X, Y, rows, cols, w)
    h = None
    try:
        h = c.csr_from_scipy(M)                                # (uploads allocate too: before the sweep)
        start = c.live_bytes()
        for hard in (False, True):
            failures = 0
            for nth in range(1, 9):
                c.release_pool()
                c.inject_alloc_failure(nth, hard=hard)
                try:
                    got = c.sddmm_host(h, X, Y, scale=True, exact=True)
                except SmmError as e:
                    assert hard and e.code == -3, f"allocation {nth}, hard={hard}: {e}"
                    assert c.live_bytes() == start
                    failures += 1
                    continue
                finally:
                    c.inject_alloc_failure(0)
                _assert_bits(got, want, f"hard={hard}, allocation {nth}")
                assert c.live_bytes() == start
                if hard:
                    break
            assert failures == (3 if hard else 0), f"hard={hard}: {failures} allocations failed (X, Y and the output)"
    finally:
        if h is not None:
            h.close()
        c.close()


def test_public_surface(ctx):
    import torch
    import sparse_matrix_mult
    from sparse_matrix_mult_amd import DeviceCSRResult, pin_operand, set_exact, set_result_device
    f = sparse_matrix_mult.sampled_dense_product
    dev = torch.device("cuda", 0)
    M, X, Y = operands("random", 8)
    rows, cols, w = entries(M)
    old = set_exact(True)
    try:
        C = f(X, Y, M)
        assert sp.isspmatrix_csr(C) and C.shape == M.shape
        assert np.array_equal(C.indptr, M.indptr) and np.array_equal(C.indices, M.indices)
        _assert_bits(C.data, restate_exact(X, Y, rows, cols), "numpy in, scipy out")
        C = f(X.tolist(), Y, M.toarray() != 0)
        P = sp.csr_matrix(M.toarray() != 0)
        pr, pc, _ = entries(P)
        _assert_bits(C.data, restate_exact(X, Y, pr, pc), "list and dense mask")
        C = f(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), M, scale_by_mask=True)
        assert sp.isspmatrix_csr(C)
        _assert_bits(C.data, restate_exact(X, Y, rows, cols, w), "torch in, scipy out")
        wide = torch.from_numpy(np.hstack([X, X])).to(dev)
        C = f(wide[:, :8], Y, M)                               # a strided tensor, used in place
        _assert_bits(C.data, restate_exact(X, Y, rows, cols), "column slice")
        old_dev = set_result_device(True)
        try:
            D = f(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), M, scale_by_mask=True)
            assert isinstance(D, DeviceCSRResult) and D.data.is_cuda and D.shape == M.shape
            S = D.to_scipy()
            assert np.array_equal(S.indptr, M.indptr) and np.array_equal(S.indices, M.indices)
            _assert_bits(S.data, restate_exact(X, Y, rows, cols, w), "set_result_device")
            D = f(X, Y, M)
            assert isinstance(D, DeviceCSRResult)
            _assert_bits(D.to_scipy().data, restate_exact(X, Y, rows, cols), "numpy in, device out")
        finally:
            set_result_device(old_dev)
        p = pin_operand(M)
        try:
            _assert_bits(f(X, Y, p, scale_by_mask=True).data, restate_exact(X, Y, rows, cols, w), "PinnedOperand")
        finally:
            p.unpin()
        # a mask that is not canonical: canonical result, merged duplicates carry the summed weight
        N, Xn, Yn = operands("noncanonical", 8)
        C = f(Xn, Yn, N, scale_by_mask=True)
        canon = N.copy()
        canon.sum_duplicates()
        assert C.has_canonical_format and np.array_equal(C.indptr, canon.indptr) and np.array_equal(C.indices, canon.indices)
        cr, cc, cw = entries(canon)
        _assert_bits(C.data, restate_exact(Xn, Yn, cr, cc, cw), "summed weights")
        # the covariance case: y=None
        B = masks()["band"]
        E = dense(B.shape[0], 12, 71)
        br, bc, bw = entries(B)
        _assert_bits(f(E, None, B, scale_by_mask=True).data, restate_exact(E, E, br, bc, bw), "y=None")
        set_exact(False)
        got = f(E, None, B, scale_by_mask=True).data
        _assert_bits(got, restate_default(E, E, br, bc, bw), "default mode through the public function")
    finally:
        set_exact(old)


def test_localised_covariance_feeds_the_apply_and_the_solve(ctx):
    """Ensemble -> localised Q -> triple_product_apply and innovation_solve, all on the device."""
    from sparse_matrix_mult_amd import innovation_solve, sampled_dense_product, set_exact, triple_product_apply
    K, k, n, hw = 400, 12, 150, 6
    rng = np.random.default_rng(81)
    E = rng.standard_normal((K, k))
    offs = list(range(-hw, hw + 1))
    L = sp.diags([np.full(K - abs(d), 1.0 - abs(d) / (hw + 1.0)) for d in offs], offs, format="csr")     # a triangular taper
    H = sp.random(n, K, density=0.03, format="csr", random_state=rng)
    x = rng.standard_normal((n, 3))
    rows, cols, w = entries(L)
    Q_ref = sp.csr_matrix((restate_exact(E, E, rows, cols, w), L.indices, L.indptr), shape=(K, K))
    old = set_exact(True)
    try:
        Q = sampled_dense_product(E, None, L, scale_by_mask=True)
        _assert_bits(Q.data, Q_ref.data, "Q")
        _assert_bits(triple_product_apply(H, Q, x), H @ (Q_ref @ (H.T @ x)), "H Q H^T x")
        Z, info = innovation_solve(H, Q, np.full(n, 0.5), x, tol=1e-8, maxiter=2000)
        assert info.converged, info
        S = (H @ Q_ref @ H.T).toarray() + 0.5 * np.eye(n)
        assert np.all(np.linalg.norm(S @ Z - x, axis=0) <= 1e-6 * np.linalg.norm(x, axis=0))
    finally:
        set_exact(old)
