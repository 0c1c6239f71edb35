"""Masked SpGEMM C = (A B) on the pattern of a mask (smm_spgemm_masked, Context.spgemm_masked_*, masked_matrix_multiply).

Contract checked here: C's pattern is the mask's; at every mask position the oracle's unmasked product stores, the
SMM_EXACT value is bit-identical to it (default: within 1e-10 relative to (|A||B|)[i,j]); every other mask position holds
+0.0.  Both evaluation paths are forced (dot, row) and the cost model (auto) runs too, on the same inputs."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import check_masked_values as _check_values, masked_want as _want, rand_csr, rel_err, shuffle_rows, signed

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1200)]
RTOL = 1e-10
MODES = [0, 1, 2]          # auto, dot, row


def _canon(M):
    M = M.tocsr().copy()
    M.sum_duplicates()
    return M


def _run(ctx, A, B, M, mode, exact):
    a, b, mk = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B), ctx.csr_from_scipy(M)
    ctx.tune_masked(mode)
    try:
        return ctx.spgemm_masked_host(a, b, mk, exact=exact)
    finally:
        ctx.tune_masked(0)
        a.close(); b.close(); mk.close()


def _all_modes(ctx, oracle, A, B, M):
    M = _canon(M)
    W, S = _want(oracle, A, B)
    for exact in (False, True):
        for mode in MODES:
            _check_values(_run(ctx, A, B, M, mode, exact), M, A, B, W, S, exact)


def _band(m, n, w):
    return sp.diags([np.ones(m)] * (2 * w + 1), list(range(-w, w + 1)), shape=(m, n), format="csr")


def _class_case():
    """Rows of A long enough for every dot class (<= 256, <= 4096, > 4096 entries) and mask rows for every row class
    (<= 256, <= 4096, a full-width row of 20 000 columns)."""
    rng = np.random.default_rng(21)
    m, K, n = 40, 9000, 20000
    lens = np.array([0, 3, 100, 250, 300, 1000, 4000, 5000, 8000] + [50] * (m - 9))
    ind, ptr = [], [0]
    for L in lens:
        ind.append(np.sort(rng.choice(K, size=L, replace=False)))
        ptr.append(ptr[-1] + L)
    A = sp.csr_matrix((rng.uniform(-1, 1, ptr[-1]), np.concatenate(ind).astype(np.int32), np.array(ptr)), shape=(m, K))
    B = signed(rand_csr(K, n, 0.0003, 22), 23)
    mlens = [0, 5, 200, 300, 3000, 5000, n, n] + list(rng.integers(0, 40, m - 8))
    mi, mp = [], [0]
    for i, L in enumerate(mlens):
        mi.append(np.sort(rng.choice(n, size=int(L), replace=False)))
        mp.append(mp[-1] + int(L))
    M = sp.csr_matrix((np.ones(mp[-1]), np.concatenate(mi).astype(np.int32), np.array(mp)), shape=(m, n))
    return A, B, M


@pytest.mark.parametrize("case", ["square", "rect", "empty_rows", "explicit_zeros", "band", "identity", "classes"])
def test_masked_matches_oracle(ctx, oracle, case):
    if case == "square":
        A, B = signed(rand_csr(400, 400, 0.05, 1), 2), signed(rand_csr(400, 400, 0.05, 3), 4)
        M = rand_csr(400, 400, 0.05, 5)
    elif case == "rect":
        A, B = signed(rand_csr(300, 700, 0.03, 6), 7), signed(rand_csr(700, 200, 0.04, 8), 9)
        M = rand_csr(300, 200, 0.2, 10)
    elif case == "empty_rows":
        A = signed(rand_csr(300, 250, 0.04, 11), 12)
        A = sp.csr_matrix(A.multiply((np.arange(300) % 4 != 0)[:, None]))
        B = signed(rand_csr(250, 280, 0.04, 13), 14)
        B = sp.csr_matrix(B.multiply((np.arange(250) % 3 != 0)[:, None]))
        M = sp.csr_matrix(rand_csr(300, 280, 0.1, 15).multiply((np.arange(300) % 5 != 1)[:, None]))
    elif case == "explicit_zeros":
        A, B = signed(rand_csr(200, 300, 0.05, 16), 17), signed(rand_csr(300, 150, 0.05, 18), 19)
        M = rand_csr(200, 150, 0.1, 20)
        M.data[::2] = 0.0                                   # stored zeros are positions too
    elif case == "band":
        A, B = signed(rand_csr(500, 500, 0.02, 24), 25), signed(rand_csr(500, 500, 0.02, 26), 27)
        M = _band(500, 500, 8)
    elif case == "identity":
        A, B = signed(rand_csr(600, 600, 0.02, 28), 29), signed(rand_csr(600, 600, 0.02, 30), 31)
        M = sp.identity(600, format="csr")
    else:
        A, B, M = _class_case()
    _all_modes(ctx, oracle, A, B, M)


def _repeat_cols(X, seed):
    """X with every row's entries stored twice (the second copy with other values), shuffled: repeated columns."""
    rng = np.random.default_rng(seed)
    X = X.tocsr()
    ind, dat, ptr = [], [], [0]
    for i in range(X.shape[0]):
        s, e = X.indptr[i], X.indptr[i + 1]
        ci = np.concatenate([X.indices[s:e], X.indices[s:e][: (e - s) // 2]])
        cv = np.concatenate([X.data[s:e], rng.uniform(-1, 1, (e - s) // 2)])
        p = rng.permutation(len(ci))
        ind.append(ci[p]); dat.append(cv[p]); ptr.append(ptr[-1] + len(ci))
    return sp.csr_matrix((np.concatenate(dat), np.concatenate(ind).astype(np.int32), np.array(ptr)), shape=X.shape)


@pytest.mark.parametrize("which", ["shuffled", "repeated_a", "repeated_b", "repeated_both"])
def test_non_canonical_operands_exact(ctx, oracle, which):
    A0, B0, M = _class_case()
    A = shuffle_rows(A0, 40) if which in ("shuffled",) else (_repeat_cols(A0, 41) if which in ("repeated_a", "repeated_both") else A0)
    B = shuffle_rows(B0, 42) if which == "shuffled" else (_repeat_cols(B0, 43) if which in ("repeated_b", "repeated_both") else B0)
    M = _canon(M)
    W, S = _want(oracle, A, B)
    for mode in MODES:                                    # forced dot with a non-canonical A still takes the row path
        _check_values(_run(ctx, A, B, M, mode, True), M, A, B, W, S, True)
    _check_values(_run(ctx, A, B, M, 0, False), M, A, B, W, S, False)


def test_negative_zero_keeps_its_sign(ctx, oracle):
    A = sp.csr_matrix((np.array([-1.0, 2.0, -3.0]), np.array([0, 1, 1]), np.array([0, 2, 3])), shape=(2, 2))
    B = sp.csr_matrix((np.array([0.0, -0.0, 5.0]), np.array([0, 0, 1]), np.array([0, 1, 3])), shape=(2, 3))
    # C[0,0] = (-1)(0) + (2)(-0) = -0 + -0 = -0.0; C[1,0] = (-3)(-0) = +0.0; column 2 is reached by no product: +0.0
    M = sp.csr_matrix(np.ones((2, 3)))
    W, S = _want(oracle, A, B)
    assert np.signbit(W[0, 0]) and S[0, 0] and not S[0, 2]
    for exact in (False, True):
        for mode in MODES:
            got = _run(ctx, A, B, M, mode, exact)
            assert np.signbit(got[0]) and got[0] == 0.0, f"mode {mode} exact {exact}: -0.0 lost its sign"
            for q in (2, 3, 5):
                assert not np.signbit(got[q]) and got[q] == 0.0, f"mode {mode} exact {exact}: position {q} is not +0.0"
            _check_values(got, M, A, B, W, S, True)


def test_unstored_a_never_multiplies_an_inf(ctx, oracle):
    A = signed(rand_csr(50, 60, 0.1, 50), 51)
    B = signed(rand_csr(60, 40, 0.1, 52), 53).tolil()
    i, j = 7, 11
    k = next(k for k in range(60) if A[i, k] == 0)
    B[k, j] = np.inf
    B = B.tocsr()
    M = sp.csr_matrix(np.ones((50, 40)))
    W, S = _want(oracle, A, B)
    assert np.isfinite(W[i, j])
    for exact in (False, True):
        for mode in MODES:
            got = _run(ctx, A, B, M, mode, exact)
            assert np.isfinite(got[i * 40 + j])
            _check_values(got[i * 40:(i + 1) * 40], sp.csr_matrix(np.ones((1, 40))), A[i], B, W[i:i + 1], S[i:i + 1], exact)


def test_update_values_then_forced_dot(ctx, oracle):
    A, B = signed(rand_csr(300, 400, 0.03, 60), 61), signed(rand_csr(400, 250, 0.03, 62), 63)
    M = _canon(rand_csr(300, 250, 0.1, 64))
    a, b, mk = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B), ctx.csr_from_scipy(M)
    ctx.tune_masked(1)
    try:
        W, S = _want(oracle, A, B)
        _check_values(ctx.spgemm_masked_host(a, b, mk, exact=True), M, A, B, W, S, True)     # B^T cached here
        B2 = B.copy(); B2.data = np.random.default_rng(65).uniform(-2, 2, B.nnz)
        b.update_values(B2.data)
        W, S = _want(oracle, A, B2)
        _check_values(ctx.spgemm_masked_host(a, b, mk, exact=True), M, A, B2, W, S, True)
        A2 = A.copy(); A2.data = np.random.default_rng(66).uniform(-2, 2, A.nnz)
        a.update_values(A2.data)
        W, S = _want(oracle, A2, B2)
        _check_values(ctx.spgemm_masked_host(a, b, mk, exact=True), M, A2, B2, W, S, True)
    finally:
        ctx.tune_masked(0)
        a.close(); b.close(); mk.close()


def test_c_layer_refuses_a_non_canonical_mask_and_other_flags(ctx):
    from sparse_matrix_mult_amd._lib import SmmError
    SMM_ERR_INVALID = -2                                 # (include/smm_hip.h)
    A, B = rand_csr(20, 30, 0.2, 70), rand_csr(30, 25, 0.2, 71)
    M = shuffle_rows(rand_csr(20, 25, 0.4, 72), 73)
    a, b, mk = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B), ctx.csr_from_scipy(M)
    try:
        with pytest.raises(SmmError) as e:
            ctx.spgemm_masked_host(a, b, mk)
        assert e.value.code == SMM_ERR_INVALID
        Mc = ctx.csr_from_scipy(_canon(M))
        out = np.empty(Mc.nnz)
        from sparse_matrix_mult_amd.engine import SMM_SYMMETRIC, _ptr
        assert ctx.lib.smm_spgemm_masked_host(ctx.handle, a.handle, b.handle, Mc.handle, SMM_SYMMETRIC, _ptr(out)) == SMM_ERR_INVALID
        Mc.close()
    finally:
        a.close(); b.close(); mk.close()


# ------------------------------------------------------------------------------ public function
def test_public_function_exact_default_device_and_pinned(oracle):
    import torch

    from sparse_matrix_mult_amd import (DeviceCSRResult, masked_matrix_multiply, pin_operand, set_exact,
                                        set_result_device)
    A, B = signed(rand_csr(250, 300, 0.04, 80), 81), signed(rand_csr(300, 220, 0.04, 82), 83)
    Mraw = shuffle_rows(rand_csr(250, 220, 0.1, 84), 85)                  # canonicalised on a host copy
    M = _canon(Mraw)
    W, S = _want(oracle, A, B)
    old = set_exact(True)
    try:
        C = masked_matrix_multiply(A, B, Mraw)
        assert sp.isspmatrix_csr(C) and C.shape == (250, 220)
        assert np.array_equal(C.indptr, M.indptr) and np.array_equal(C.indices, M.indices)
        _check_values(C.data, M, A, B, W, S, True)
        pa, pb, pm = pin_operand(A), pin_operand(B), pin_operand(M)
        try:
            Cp = masked_matrix_multiply(pa, pb, pm)
            assert np.array_equal(Cp.data.view(np.int64), C.data.view(np.int64))
            with pytest.raises(ValueError, match="canonical"):
                bad = pin_operand(Mraw)
                try:
                    masked_matrix_multiply(pa, pb, bad)
                finally:
                    bad.unpin()
            oldd = set_result_device(True)
            try:
                D = masked_matrix_multiply(A, B, Mraw)
                assert isinstance(D, DeviceCSRResult) and D.shape == (250, 220)
                assert D.indptr.dtype == torch.int64 and D.indices.dtype == torch.int32
                assert np.array_equal(D.indptr.cpu().numpy(), M.indptr) and np.array_equal(D.indices.cpu().numpy(), M.indices)
                assert np.array_equal(D.data.cpu().numpy().view(np.int64), C.data.view(np.int64))
                Dp = masked_matrix_multiply(pa, pb, pm)
                assert np.array_equal(Dp.data.cpu().numpy().view(np.int64), C.data.view(np.int64))
                E = masked_matrix_multiply(A, B, sp.csr_matrix((250, 220)))
                assert isinstance(E, DeviceCSRResult) and E.nnz == 0
                Z = masked_matrix_multiply(sp.csr_matrix((250, 300)), B, M)
                assert np.array_equal(Z.data.cpu().numpy().view(np.int64), np.zeros(M.nnz, dtype=np.int64))
            finally:
                set_result_device(oldd)
        finally:
            pa.unpin(); pb.unpin(); pm.unpin()
        set_exact(False)
        Cd = masked_matrix_multiply(A, B, M)
        _check_values(Cd.data, M, A, B, W, S, False)
        # the empty cases of the contract
        assert masked_matrix_multiply(A, B, sp.csr_matrix((250, 220))).nnz == 0
        for Z in (masked_matrix_multiply(sp.csr_matrix((250, 300)), B, M), masked_matrix_multiply(A, sp.csr_matrix((300, 220)), M)):
            assert np.array_equal(Z.indices, M.indices) and np.array_equal(Z.data.view(np.int64), np.zeros(M.nnz, dtype=np.int64))
    finally:
        set_exact(old)


# ------------------------------------------------------------------------------ BASELINE configs[1] shape
@pytest.mark.parametrize("maskkind", ["diag", "band64"])
def test_config1_shaped_sampled_rows(ctx, oracle, maskkind):
    import torch

    from sparse_matrix_mult_amd.synthetic import gen_csr_device
    dev = torch.device("cuda", 0)
    m = n = 50000
    a_t = gen_csr_device(torch, m, n, 0.01, 1, dev)
    b_t = gen_csr_device(torch, n, n, 0.01, 2, dev)
    a_h = tuple(t.cpu().numpy() for t in a_t)
    b_h = tuple(t.cpu().numpy() for t in b_t)
    A, B = ctx.csr_from_torch(m, n, *a_t), ctx.csr_from_torch(n, n, *b_t)
    w = 0 if maskkind == "diag" else 64
    Mh = _band(m, n, w)
    mk = ctx.csr_from_scipy(Mh)
    try:
        for exact in (False, True):
            for mode in MODES:
                ctx.tune_masked(mode)
                got = ctx.spgemm_masked_host(A, B, mk, exact=exact)
                for r0 in (0, 31337):
                    r1 = r0 + 40
                    cnt, oidx, oval = oracle.sparse_rows(a_h, b_h, n, r0, r1)
                    optr = np.concatenate([[0], np.cumsum(cnt)])
                    for i in range(r0, r1):
                        lo, hi = Mh.indptr[i], Mh.indptr[i + 1]
                        cols, g = Mh.indices[lo:hi], got[lo:hi]
                        ri, rv = oidx[optr[i - r0]:optr[i - r0 + 1]], oval[optr[i - r0]:optr[i - r0 + 1]]
                        want = dict(zip(ri.tolist(), rv.tolist()))
                        wv = np.array([want.get(c, 0.0) for c in cols.tolist()])
                        if exact:
                            assert np.array_equal(g.view(np.int64), wv.view(np.int64)), f"row {i} mode {mode}"
                        else:
                            assert rel_err(g, wv) <= RTOL, f"row {i} mode {mode}"
    finally:
        ctx.tune_masked(0)
        mk.close(); A.close(); B.close()
