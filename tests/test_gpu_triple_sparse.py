"""Sparse-output triple product S = H Q H^T (smm_triple_product_sparse, Context.triple_sparse_*, sparse_triple_product)
and the device CSR transpose (smm_csr_transpose, Context.transpose).

Contract checked here: the pattern is structural -- triu of the 0/1 product Hb @ Qb @ Hb.T --, columns ascend within a
row, SMM_EXACT values are bit-identical to the reference loop (oracle.triple with full=0, and the device's dense triple
product), default values within 1e-10 relative; every upper position left out is 0 in the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import (arrays, check_triple_sparse as _check, rand_csr, shuffle_rows, signed, triple_pattern as _pattern,
                     wide_csr)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
RTOL = 1e-10


def _q(k, d, seed):
    S = sp.random(k, k, density=d / 2, format="csr", random_state=np.random.default_rng(seed))
    return (S + S.T).tocsr()


def _dense(res, rows, n):
    ptr, idx, val = res
    return sp.csr_matrix((val, idx, ptr), shape=(rows, n)).toarray()


def _run(ctx, H, Q, **kw):
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        return ctx.triple_sparse_host(h, q, **kw)
    finally:
        h.close(); q.close()


# ------------------------------------------------------------------------------ transpose
def _csc_arrays(A):
    C = A.tocsc()
    return C.indptr.astype(np.int32), C.indices.astype(np.int32), C.data


def _transpose_arrays(ctx, A):
    a = ctx.csr_from_scipy(A)
    t = ctx.transpose(a)
    try:
        assert (t.rows, t.cols, t.nnz) == (A.shape[1], A.shape[0], A.nnz)
        return t.to_host()
    finally:
        t.close(); a.close()


@pytest.mark.parametrize("case", ["1x1", "empty_rows_cols", "unsorted", "repeated", "wide", "long_column", "zero"])
def test_transpose_equals_tocsc(ctx, case):
    rng = np.random.default_rng(11)
    if case == "1x1":
        A = sp.csr_matrix(np.array([[-2.5]]))
    elif case == "empty_rows_cols":
        A = rand_csr(300, 200, 0.02, 1)
        A = sp.csr_matrix(A.multiply(np.tile(np.arange(200) % 3 != 0, (300, 1))))
        A = sp.vstack([A, sp.csr_matrix((5, 200))]).tocsr()
    elif case == "unsorted":
        A = shuffle_rows(signed(rand_csr(400, 500, 0.03, 2), 3), 4)
    elif case == "repeated":
        ind = rng.integers(0, 50, size=600).astype(np.int32)
        ptr = np.arange(0, 601, 6, dtype=np.int32)
        A = sp.csr_matrix((rng.standard_normal(600), ind, ptr), shape=(100, 50))
    elif case == "wide":
        A = wide_csr(2000, 1_000_000, 20, 5)
    elif case == "long_column":
        B = rand_csr(20000, 300, 0.002, 6).tolil()
        B[:, 7] = rng.standard_normal((20000, 1))             # one column with 20 000 entries (> 8192)
        B[::3, 42] = rng.standard_normal((6667, 1))           # and one in the LDS range
        A = shuffle_rows(B.tocsr(), 7)
    else:
        A = sp.csr_matrix((30, 40))
    wp, wi, wv = _csc_arrays(A)
    gp, gi, gv = _transpose_arrays(ctx, A)
    assert np.array_equal(gp.astype(np.int64), wp.astype(np.int64))
    assert np.array_equal(gi.astype(np.int64), wi.astype(np.int64))
    assert np.array_equal(gv.view(np.int64), np.asarray(wv, dtype=np.float64).view(np.int64))


# ------------------------------------------------------------------------------ sparse triple against the oracle
SHAPES = [(1, 1, 1.0, 1.0), (60, 90, 0.1, 0.1), (500, 500, 0.3, 0.3), (300, 9000, 0.02, 0.004), (257, 5000, 0.05, 0.01),
          (1500, 2500, 0.02, 0.004), (2100, 700, 0.01, 0.01)]


@pytest.mark.parametrize("n,k,dh,dq", SHAPES)
@pytest.mark.parametrize("exact", [False, True])
def test_triple_sparse_matches_oracle(ctx, oracle, n, k, dh, dq, exact):
    H, Q = signed(rand_csr(n, k, dh, 3), 5), signed(_q(k, dq, 4), 6)
    want = oracle.triple(arrays(H), arrays(Q), k, 0)
    res = _run(ctx, H, Q, exact=exact)
    _check(res, H, Q, want, exact)


@pytest.mark.parametrize("n,k,dh,dq", [(500, 500, 0.3, 0.3), (300, 9000, 0.02, 0.004), (1500, 2500, 0.02, 0.004)])
def test_exact_equals_the_device_dense_triple(ctx, n, k, dh, dq):
    H, Q = signed(rand_csr(n, k, dh, 8), 9), signed(_q(k, dq, 10), 11)
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        dense = ctx.triple_host(h, q, exact=True)
        res = ctx.triple_sparse_host(h, q, exact=True)
    finally:
        h.close(); q.close()
    got = _dense(res, n, n)
    assert np.array_equal(got.view(np.int64), dense.view(np.int64))


@pytest.mark.parametrize("exact", [False, True])
def test_unsorted_and_repeated_columns(ctx, oracle, exact):
    rng = np.random.default_rng(12)
    n, k = 400, 600
    H = shuffle_rows(signed(rand_csr(n, k, 0.02, 13), 14), 15)
    # repeated columns: every row of H gets a copy of its first entry behind its own entries; Q likewise, plus its diagonal
    # build row by row (stored order: H's row, then the duplicate)
    data, ind, ptr = [], [], [0]
    for i in range(n):
        s, e = H.indptr[i], H.indptr[i + 1]
        data += list(H.data[s:e]); ind += list(H.indices[s:e])
        if e > s:
            data.append(rng.standard_normal()); ind.append(H.indices[s])
        ptr.append(len(ind))
    H2 = sp.csr_matrix((np.array(data), np.array(ind, dtype=np.int32), np.array(ptr, dtype=np.int32)), shape=(n, k))
    H2.has_sorted_indices = False
    Q = shuffle_rows(signed(_q(k, 0.02, 16), 17), 18)
    data, ind, ptr = [], [], [0]
    for r in range(k):
        s, e = Q.indptr[r], Q.indptr[r + 1]
        data += list(Q.data[s:e]); ind += list(Q.indices[s:e])
        data.append(rng.standard_normal()); ind.append(r)
        if e > s:
            data.append(rng.standard_normal()); ind.append(Q.indices[s])
        ptr.append(len(ind))
    Qd = sp.csr_matrix((np.array(data), np.array(ind, dtype=np.int32), np.array(ptr, dtype=np.int32)), shape=(k, k))
    Qd.has_sorted_indices = False
    want = oracle.triple(arrays(H2), arrays(Qd), k, 0)
    res = _run(ctx, H2, Qd, exact=exact)
    _check(res, H2, Qd, want, exact)


@pytest.mark.parametrize("exact", [False, True])
def test_long_rows_of_t_take_the_workgroup_and_global_paths(ctx, oracle, exact):
    rng = np.random.default_rng(20)
    n, k = 40, 20000
    per_row = np.array([1, 2, 3, 5, 10, 20, 40, 80, 150, 200] * 4)
    rows = [np.sort(rng.choice(k, size=c, replace=False)) for c in per_row]
    ptr = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int32)
    H = sp.csr_matrix((rng.uniform(-1, 1, ptr[-1]), np.concatenate(rows).astype(np.int32), ptr), shape=(n, k))
    Q = signed(_q(k, 0.005, 21), 22)                        # ~100 entries per row: T_i from ~100 to > 4096 entries
    want = oracle.triple(arrays(H), arrays(Q), k, 0)
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        ctx.timing(True); ctx.timing_reset()
        res = ctx.triple_sparse_host(h, q, exact=exact)
        launches = ctx.kernel_time("smm_triple_sparse_s2")[1]
        ctx.timing(False)
    finally:
        h.close(); q.close()
    assert launches == 3, "the wave, workgroup and global classes of stage 2 each ran once"
    _check(res, H, Q, want, exact)


def test_empty_rows_and_zero_operands(ctx, oracle):
    H = signed(rand_csr(300, 400, 0.01, 23), 24)
    H = sp.vstack([H[:100], sp.csr_matrix((50, 400)), H[100:]]).tocsr()      # 50 empty rows of H -> empty rows of S
    Q = signed(_q(400, 0.01, 25), 26)
    want = oracle.triple(arrays(H), arrays(Q), 400, 0)
    res = _run(ctx, H, Q, exact=True)
    _check(res, H, Q, want, True)
    assert np.all(np.diff(res[0])[100:150] == 0)
    for Hz, Qz in ((sp.csr_matrix((30, 40)), _q(40, 0.1, 1)), (rand_csr(30, 40, 0.1, 2), sp.csr_matrix((40, 40)))):
        ptr, idx, val = _run(ctx, Hz, Qz, exact=True)
        assert ptr.shape == (31,) and not ptr.any() and idx.size == 0 and val.size == 0


# ------------------------------------------------------------------------------ full matrix, row ranges, blocking
@pytest.mark.parametrize("exact", [False, True])
def test_full_matrix_is_the_mirrored_upper_triangle(ctx, exact):
    H, Q = signed(rand_csr(700, 900, 0.01, 30), 31), signed(_q(900, 0.01, 32), 33)
    n = H.shape[0]
    up = _run(ctx, H, Q, exact=exact)
    U = sp.csr_matrix((up[2], up[1], up[0]), shape=(n, n))
    fp, fi, fv = _run(ctx, H, Q, exact=exact, full=True)
    for i in range(n):
        assert np.all(np.diff(fi[fp[i]:fp[i + 1]]) > 0)
    want = (U + sp.triu(U, 1).T).tocsr()
    want.sort_indices()
    assert np.array_equal(fp, want.indptr) and np.array_equal(fi, want.indices)
    assert np.array_equal(fv.view(np.int64), want.data.view(np.int64))


def test_row_ranges_concatenate_to_the_whole(ctx):
    H, Q = signed(rand_csr(1200, 1500, 0.01, 34), 35), signed(_q(1500, 0.004, 36), 37)
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        whole = ctx.triple_sparse_host(h, q, exact=True)
        a = ctx.triple_sparse_host(h, q, exact=True, row_begin=0, row_end=517)
        b = ctx.triple_sparse_host(h, q, exact=True, row_begin=517, row_end=1200)
    finally:
        h.close(); q.close()
    assert np.array_equal(whole[0], np.concatenate([a[0], b[0][1:] + a[0][-1]]))
    assert np.array_equal(whole[1], np.concatenate([a[1], b[1]]))
    assert np.array_equal(whole[2].view(np.int64), np.concatenate([a[2], b[2]]).view(np.int64))


def test_tiny_block_budget_is_bit_identical(ctx):
    H, Q = signed(rand_csr(2000, 3000, 0.004, 38), 39), signed(_q(3000, 0.004, 40), 41)
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        ref = ctx.triple_sparse_host(h, q, exact=True)
        full_ref = ctx.triple_sparse_host(h, q, exact=True, full=True)
        ctx.tune_triple_sparse(5000)                       # ~ a hundred row blocks
        try:
            got = ctx.triple_sparse_host(h, q, exact=True)
            full_got = ctx.triple_sparse_host(h, q, exact=True, full=True)
            dev = [t.cpu().numpy() for t in ctx.triple_sparse_torch(h, q, exact=True)]
        finally:
            ctx.tune_triple_sparse(0)
    finally:
        h.close(); q.close()
    for g, w in ((got, ref), (full_got, full_ref), (dev, ref)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
        assert np.array_equal(g[2].view(np.int64), w[2].view(np.int64))


# ------------------------------------------------------------------------------ public API
def test_public_api_modes(oracle):
    import sparse_matrix_mult
    from sparse_matrix_mult_amd import pin_operand, set_exact, set_result_device, sparse_triple_product
    H, Q = signed(rand_csr(600, 800, 0.01, 42), 43), signed(_q(800, 0.01, 44), 45)
    want = oracle.triple(arrays(H), arrays(Q), 800, 0)
    old = set_exact(True)
    try:
        S = sparse_triple_product(H, Q)
        assert sp.isspmatrix_csr(S) and S.shape == (600, 600)
        _check((S.indptr.astype(np.int64), S.indices, S.data), H, Q, want, True)
        S2 = sparse_matrix_mult.sparse_triple_product(H, Q)
        assert np.array_equal(S2.data.view(np.int64), S.data.view(np.int64))
        pinned = pin_operand(H)
        try:
            S3 = sparse_triple_product(pinned, Q)
        finally:
            pinned.unpin()
        assert np.array_equal(S3.indices, S.indices) and np.array_equal(S3.data.view(np.int64), S.data.view(np.int64))
        F = sparse_triple_product(H, Q, compute_full_matrix=True)
        U = S
        assert abs(F - (U + sp.triu(U, 1).T)).max() == 0
        old_dev = set_result_device(True)
        try:
            D = sparse_triple_product(H, Q)
            assert D.shape == (600, 600) and D.nnz == S.nnz
            Ds = D.to_scipy()
            assert np.array_equal(Ds.indices, S.indices) and np.array_equal(Ds.data.view(np.int64), S.data.view(np.int64))
            Z = sparse_triple_product(sp.csr_matrix((600, 800)), Q)
            assert Z.nnz == 0 and Z.shape == (600, 600)
        finally:
            set_result_device(old_dev)
    finally:
        set_exact(old)
    set_exact(False)
    try:
        S = sparse_triple_product(H, Q)
        _check((S.indptr.astype(np.int64), S.indices, S.data), H, Q, want, False)
    finally:
        set_exact(old)
    with pytest.raises(ValueError):
        sparse_triple_product(H, Q[:, :700])


def _local_h(n, K, seed):
    """Each row: 8 distinct columns inside a 16-column window around a random centre."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(8, K - 8, size=n)
    off = np.argsort(rng.random((n, 16)), axis=1)[:, :8]
    cols = np.sort(centre[:, None] - 8 + off, axis=1).astype(np.int32)
    ptr = np.arange(0, 8 * n + 1, 8, dtype=np.int32)
    return sp.csr_matrix((rng.uniform(-1, 1, 8 * n), cols.ravel(), ptr), shape=(n, K))


def _banded_q(K, w, seed):
    rng = np.random.default_rng(seed)
    diags = [rng.uniform(-1, 1, K - abs(d)) for d in range(-w, w + 1)]
    B = sp.diags(diags, list(range(-w, w + 1)), shape=(K, K), format="csr")
    return ((B + B.T) * 0.5).tocsr()


def test_structured_moderate_size(ctx):
    n, K = 20000, 100000
    H, Q = _local_h(n, K, 50), _banded_q(K, 8, 51)
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        ptr, idx, val = ctx.triple_sparse_host(h, q)
    finally:
        h.close(); q.close()
    pp, pi = _pattern(H, Q)
    assert np.array_equal(ptr, pp) and np.array_equal(idx.astype(np.int64), pi.astype(np.int64))
    W = sp.triu((H @ Q @ H.T).tocsr()).tocsr()
    got = sp.csr_matrix((val, idx, ptr), shape=(n, n))
    diff = abs(got - W)
    scale = abs(H) @ abs(Q) @ abs(H).T
    assert (diff - RTOL * sp.triu(scale)).max() <= 0
