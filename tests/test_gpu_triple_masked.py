"""Masked sparse triple product S = H Q H^T on the positions of L with k >= i (smm_triple_product_sparse_masked,
Context.triple_sparse_*(mask=...), sparse_triple_product(..., mask=L)).

Contract checked here: the pattern is triu(L), canonical; SMM_EXACT values are bit-identical to the oracle's dense
triple (full=0) at every position, +0.0 where it holds 0; default values within 1e-10 relative; the full matrix mirrors
the upper part; row ranges and the row-block budget do not change a bit."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import arrays, check_triple_masked as _check, rand_csr, shuffle_rows, signed, upper_mask as _upper

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
RTOL = 1e-10


def _q(k, d, seed):
    S = sp.random(k, k, density=d / 2, format="csr", random_state=np.random.default_rng(seed))
    return (S + S.T).tocsr()


def _masks(n):
    band = sp.diags([np.ones(n)] * 9, list(range(-4, 5)), shape=(n, n), format="csr")
    rnd = rand_csr(n, n, 0.05, 6)
    return {"diag": sp.identity(n, format="csr"), "band": band, "random": rnd,
            "random_unsorted": shuffle_rows(rnd, 7)}


@pytest.mark.parametrize("kind", ["diag", "band", "random", "random_unsorted"])
@pytest.mark.parametrize("exact", [False, True])
def test_masked_triple_matches_oracle(ctx, oracle, kind, exact):
    from sparse_matrix_mult_amd import set_exact, sparse_triple_product
    n, k = 500, 800
    H, Q = signed(rand_csr(n, k, 0.02, 3), 4), signed(_q(k, 0.01, 5), 6)
    want = oracle.triple(arrays(H), arrays(Q), k, 0)
    L = _masks(n)[kind]
    U = _upper(L)
    old = set_exact(exact)
    try:
        S = sparse_triple_product(H, Q, mask=L)
    finally:
        set_exact(old)
    assert sp.isspmatrix_csr(S) and S.shape == (n, n)
    _check((S.indptr, S.indices, S.data), U, want, H, Q, exact)


@pytest.mark.parametrize("exact", [False, True])
def test_masked_triple_long_rows_and_non_canonical_h(ctx, oracle, exact):
    rng = np.random.default_rng(20)
    n, k = 40, 20000
    per_row = np.array([1, 2, 3, 5, 10, 20, 40, 80, 150, 200] * 4)
    rows = [np.sort(rng.choice(k, size=c, replace=False)) for c in per_row]
    ptr = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int32)
    H = sp.csr_matrix((rng.uniform(-1, 1, ptr[-1]), np.concatenate(rows).astype(np.int32), ptr), shape=(n, k))
    H = shuffle_rows(H, 21)
    Q = signed(_q(k, 0.005, 22), 23)
    want = oracle.triple(arrays(H), arrays(Q), k, 0)
    L = rand_csr(n, n, 0.5, 24)
    h, q, mk = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q), ctx.csr_from_scipy(_upper(L))
    try:
        res = ctx.triple_sparse_host(h, q, exact=exact, mask=mk)
    finally:
        h.close(); q.close(); mk.close()
    _check(res, _upper(L), want, H, Q, exact)


def test_full_matrix_is_mirrored(ctx, oracle):
    from sparse_matrix_mult_amd import set_exact, sparse_triple_product
    n, k = 300, 500
    H, Q = signed(rand_csr(n, k, 0.03, 30), 31), signed(_q(k, 0.02, 32), 33)
    L = rand_csr(n, n, 0.1, 34)
    old = set_exact(True)
    try:
        up = sparse_triple_product(H, Q, mask=L)
        F = sparse_triple_product(H, Q, mask=L, compute_full_matrix=True)
    finally:
        set_exact(old)
    for i in range(n):
        assert np.all(np.diff(F.indices[F.indptr[i]:F.indptr[i + 1]]) > 0), f"row {i} not ascending"
    D = F.toarray()
    assert np.array_equal(D.view(np.int64), D.T.view(np.int64)), "not symmetric"
    U = up.toarray()
    assert np.array_equal(np.triu(D).view(np.int64), U.view(np.int64))
    pat = (_upper(L) + _upper(L).T).tocsr()
    pat.sort_indices()
    assert np.array_equal(F.indptr, pat.indptr) and np.array_equal(F.indices, pat.indices)


@pytest.mark.parametrize("exact", [False, True])
def test_row_ranges_and_block_budget(ctx, oracle, exact):
    n, k = 600, 900
    H, Q = signed(rand_csr(n, k, 0.02, 40), 41), signed(_q(k, 0.01, 42), 43)
    L = rand_csr(n, n, 0.05, 44)
    U = _upper(L)
    want = oracle.triple(arrays(H), arrays(Q), k, 0)
    h, q, mk = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q), ctx.csr_from_scipy(U)
    try:
        whole = ctx.triple_sparse_host(h, q, exact=exact, mask=mk)
        _check(whole, U, want, H, Q, exact)
        for r0, r1 in ((0, 1), (17, 333), (333, 600), (600, 600)):
            part = ctx.triple_sparse_host(h, q, exact=exact, mask=mk, row_begin=r0, row_end=r1)
            lo, hi = whole[0][r0], whole[0][r1]
            assert np.array_equal(part[0], whole[0][r0:r1 + 1] - lo)
            assert np.array_equal(part[1], whole[1][lo:hi])
            assert np.array_equal(part[2].view(np.int64), whole[2][lo:hi].view(np.int64))
        ctx.tune_triple_sparse(64)                                   # many row blocks
        try:
            small = ctx.triple_sparse_host(h, q, exact=exact, mask=mk)
        finally:
            ctx.tune_triple_sparse(0)
        for a, b in zip(small, whole):
            assert np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))
    finally:
        h.close(); q.close(); mk.close()


def test_device_result_pinned_and_zero_operands(ctx, oracle):
    import torch

    from sparse_matrix_mult_amd import DeviceCSRResult, pin_operand, set_exact, set_result_device, sparse_triple_product
    n, k = 200, 300
    H, Q = signed(rand_csr(n, k, 0.04, 50), 51), signed(_q(k, 0.03, 52), 53)
    L = rand_csr(n, n, 0.1, 54)
    old = set_exact(True)
    try:
        S = sparse_triple_product(H, Q, mask=L)
        ph, pq, pl = pin_operand(H), pin_operand(Q), pin_operand(_upper(L))
        try:
            Sp = sparse_triple_product(ph, pq, mask=pl)
            assert np.array_equal(Sp.data.view(np.int64), S.data.view(np.int64))
            oldd = set_result_device(True)
            try:
                D = sparse_triple_product(H, Q, mask=L)
                assert isinstance(D, DeviceCSRResult) and D.indptr.dtype == torch.int64
                assert np.array_equal(D.indices.cpu().numpy(), S.indices)
                assert np.array_equal(D.data.cpu().numpy().view(np.int64), S.data.view(np.int64))
            finally:
                set_result_device(oldd)
        finally:
            ph.unpin(); pq.unpin(); pl.unpin()
        Z = sparse_triple_product(sp.csr_matrix((n, k)), Q, mask=L)
        U = _upper(L)
        assert np.array_equal(Z.indptr, U.indptr) and np.array_equal(Z.indices, U.indices)
        assert np.array_equal(Z.data.view(np.int64), np.zeros(U.nnz, np.int64))
    finally:
        set_exact(old)
