"""The cases of tests/empty_products.py are what they claim, shown with the references alone (no GPU): the conditions that
keep tests/test_gpu_empty_products.py honest.  Every operand holds entries; the oracle's product is empty (or the one
planted entry); scipy's structural product agrees; strictly_lower's rows reach every class of the dispatch."""
import numpy as np
import pytest
import scipy.sparse as sp

import empty_products as ep
from empty_products import arrays


def _bits_zero(x):
    return not np.ascontiguousarray(x, dtype=np.float64).view(np.int64).any()


def _structural_nnz(A, B, upper=False):
    """nnz of scipy's structural product, counted before any eliminate_zeros().  (On copies: the comparison canonicalises
    an unsorted operand in place.)"""
    P = ((A.copy() != 0) @ (B.copy() != 0)).tocsr()
    return int(sp.triu(P).nnz if upper else P.nnz)


def _pairs():
    """(id, A, B, symmetric) of every CSR x CSR case whose product is empty."""
    out = []
    for v in ep.MISSED_VARIANTS:
        A, B, _ = ep.missed_rows(v)
        out += [(f"missed_rows-{v}", A, B, False), (f"missed_rows-{v}-sym", A, B, True)]
    A, B = ep.strictly_lower()
    out.append(("strictly_lower-sym", A, B, True))
    for v in ep.VECTOR_VARIANTS:
        A, B = ep.vectors(v)
        out += [(f"vectors-{v}", A, B, False), (f"vectors-{v}-sym", A, B, True)]
    return out


PAIRS = _pairs()


@pytest.mark.parametrize("name,A,B,symmetric", PAIRS, ids=[p[0] for p in PAIRS])
def test_pair_is_structurally_empty_and_no_operand_is(oracle, name, A, B, symmetric):
    assert A.nnz > 0 and B.nnz > 0
    assert not np.any(A.data == 0) and not np.any(B.data == 0)
    n = B.shape[1]
    ptr, idx, val = oracle.sparse(arrays(A), arrays(B), n, symmetric=symmetric)
    assert ptr.dtype == np.int64 and len(ptr) == A.shape[0] + 1 and not ptr.any() and len(idx) == 0 and len(val) == 0
    assert _bits_zero(oracle.dense(arrays(A), arrays(B), n, symmetric=symmetric))
    assert _structural_nnz(A, B, upper=symmetric) == 0


def test_missed_rows_shape_and_row_lengths():
    for v in ep.MISSED_VARIANTS:
        A, B, J = ep.missed_rows(v)
        assert A.shape == (300, 200) and B.shape == (200, 300)
        assert set(A.indices.tolist()) == set(J.tolist())                          # A stores entries only in J, and in all of it
        assert not np.diff(B.indptr)[J].any() and np.all(np.delete(np.diff(B.indptr), J) > 0)
        la = np.diff(A.indptr)
        assert la[0] == 0 and la[1] == 1 and la[2] == len(J) and np.array_equal(A.indices[A.indptr[2]:A.indptr[3]], J)
        assert not ep.row_products(A, B).any()
    B = ep.missed_rows("unsorted")[1]
    cols = [B.indices[B.indptr[r]:B.indptr[r + 1]] for r in range(B.shape[0])]
    assert any(len(c) != len(set(c.tolist())) for c in cols) and any(np.any(np.diff(c) < 0) for c in cols)


def test_thresholds_are_the_sources():
    import inspect
    from sparse_matrix_mult_amd.engine import Context
    tiny, small, medium = ep.thresholds()
    d = inspect.signature(Context.tune_hash).parameters
    assert (small, medium) == (d["small_max"].default, d["medium_max"].default)
    assert 0 < tiny < 2 * tiny < small < medium


def test_strictly_lower_is_lower_and_reaches_every_class(oracle):
    A, B = ep.strictly_lower()
    n = ep.N_LOWER
    assert A.shape == B.shape == (n, n) and abs(n - 400) <= 40
    ra, rb = np.repeat(np.arange(n), np.diff(A.indptr)), np.repeat(np.arange(n), np.diff(B.indptr))
    assert np.all(A.indices < ra) and np.all(B.indices <= rb)
    assert np.all(B.indices[B.indptr[1:] - 1] == np.arange(n))                     # B stores its whole diagonal
    prod = ep.row_products(A, B)
    for name, (lo, hi) in ep.product_classes().items():                            # one count per class
        assert np.any((prod > lo) & (prod <= hi)), f"no row with a product count in ({lo}, {hi}] ({name})"
    tiny = ep.thresholds()[0]
    na = np.diff(A.indptr)
    assert np.any((prod > 0) & (prod <= tiny) & (na <= tiny)) and np.any((prod > tiny) & (prod <= 2 * tiny) & (na <= 2 * tiny))
    for row, count in ep.target_rows().items():                                    # both sides of every threshold, exactly
        assert prod[row] == count, (row, count, prod[row])
        assert n - row > ep.thresholds()[1]         # symmetric: more columns right of the diagonal than the small class takes
    for row in ep.FAR_ROWS:
        assert prod[row] > 2 * ep.thresholds()[2]
    assert not prod[list(ep.EMPTY_ROWS)].any()
    r0, r1 = ep.SHARDS[ep.BEARING_SHARD]
    assert np.all(prod[r0:r1] > 0)                  # a shard of product-bearing rows only
    assert [s[0] for s in ep.SHARDS] + [ep.SHARDS[-1][1]] == [0] + [s[1] for s in ep.SHARDS]
    # the control: without symmetric it is an ordinary product, strictly lower
    ptr, idx, val = oracle.sparse(arrays(A), arrays(B), n, symmetric=False)
    assert len(idx) > 10000 and np.all(idx < np.repeat(np.arange(n), np.diff(ptr))) and np.all(val != 0)
    assert len(idx) == _structural_nnz(A, B)
    assert np.array_equal(np.diff(ptr) > 0, prod > 0)                              # every product-bearing row has output there


@pytest.mark.parametrize("variant", list(ep.PLUS_ONE_VARIANTS))
def test_lower_plus_one_is_exactly_the_one_entry(oracle, variant):
    A, B, r = ep.lower_plus_one(variant)
    n = ep.N_LOWER
    assert A.has_sorted_indices and np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0)
    ptr, idx, val = oracle.sparse(arrays(A), arrays(B), n, symmetric=True)
    want_ptr = (np.arange(n + 1) > r).astype(np.int64)
    brr = B.data[B.indptr[r + 1] - 1]
    assert np.array_equal(ptr, want_ptr) and idx.tolist() == [r] and val.tolist() == [0.75 * brr] and val[0] != 0
    D = oracle.dense(arrays(A), arrays(B), n, symmetric=True)
    assert D[r, r] == val[0] and np.count_nonzero(D) == 1
    assert _structural_nnz(A, B, upper=True) == 1
    if variant == "highest_class":
        assert ep.row_products(A, B)[r] > 2 * ep.thresholds()[2]
    assert {"last_row": n - 1, "row0": 0}.get(variant, r) == r


def test_vectors_shapes():
    A, B = ep.vectors("inner")
    assert A.shape[0] == 1 and B.shape[1] == 1 and A.shape[1] == B.shape[0]
    assert not set(A.indices.tolist()) & set(np.flatnonzero(np.diff(B.indptr)).tolist())
    A, B = ep.vectors("outer")
    assert A.shape[1] == B.shape[0] == 2 and A.shape[0] == B.shape[1]
    assert set(A.indices.tolist()) == {0} and np.diff(B.indptr).tolist()[0] == 0 and 0 in np.diff(A.indptr)


@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_triple_cases_are_empty_where_they_say(oracle, name):
    H, Q = ep.triple_case(name)
    n, K = ep.N_TRIPLE, ep.K_TRIPLE
    assert H.shape == (n, K) and Q.shape == (K, K) and H.nnz > 0 and Q.nnz > 0
    assert abs(Q - Q.T).nnz == 0 and np.array_equal(Q.indptr, Q.T.tocsr().indptr)  # symmetric, pattern and values
    t_nnz = _structural_nnz(H, Q)
    assert (t_nnz == 0) == (name == "triple_t_empty")
    if name == "triple_s_empty":
        assert t_nnz > 500
    assert ((H.copy() != 0) @ (Q.copy() != 0) @ (H.copy() != 0).T).nnz == 0
    for full in (0, 1):
        assert _bits_zero(oracle.triple(arrays(H), arrays(Q), K, full))
    assert _bits_zero(oracle.triple(arrays(H), arrays(Q), K, 0, 37, 150))
    M = ep.triple_mask()
    assert M.has_canonical_format and M.shape == (n, n) and M.nnz > n and np.all(M.diagonal() == 1.0)


def test_solve_systems_end_in_a_few_iterations_with_every_product_zero():
    """The restated CG on the two systems: S's products are all zero, so it is CG on R alone -- three distinct diagonal
    values, a few iterations, every column converged.  The GPU test compares the device CG with exactly this."""
    from cg_restatement import diag_csr, restate_cg
    from spmm_restatement import restate_spmm
    r, D = ep.solve_diagonal(), ep.solve_rhs()
    for name in ep.TRIPLE_CASES:
        H, Q = ep.triple_case(name)
        assert _bits_zero(restate_spmm(H, restate_spmm(Q, restate_spmm(H, D, True))))
        Z, info = restate_cg(H, Q, diag_csr(r), D, tol=1e-8, maxiter=50)
        assert np.all(info.status == 0) and np.all(info.iterations >= 2) and np.all(info.iterations <= 6)
        assert np.allclose(Z, D / r[:, None], rtol=1e-7, atol=0)
        # the quadrature of a +-1 probe on a diagonal matrix of three distinct values is exact after three iterations:
        # the weight of each value is the share of rows that hold it, so every sample is ln det R up to rounding
        from slq_restatement import restate_cg_coef, restate_probes, slq
        info = restate_cg_coef(H, Q, diag_csr(r), restate_probes(ep.N_TRIPLE, 4, 7), tol=1e-8, maxiter=20)[1]
        assert np.all(info.iterations == 3) and np.all(info.status == 0)
        assert np.allclose(slq(info, ep.N_TRIPLE)[0], np.sum(np.log(r)), rtol=1e-9, atol=0)


def test_masked_cases_lie_on_unreached_positions(oracle):
    A, B, M = ep.masked_unreached()
    assert A.nnz > 0 and B.nnz > 0 and M.nnz > 500 and M.has_canonical_format and M.shape == (A.shape[0], B.shape[1])
    reach = ep.structural(A, B)
    assert reach.sum() > 2000                                                      # the product is not empty
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    assert not reach[rows, M.indices].any()
    ptr, idx, val = oracle.sparse(arrays(A), arrays(B), B.shape[1])
    S = np.zeros(reach.shape, bool)
    S[np.repeat(np.arange(A.shape[0]), np.diff(ptr)), idx] = True
    assert np.array_equal(S, reach) and not S[rows, M.indices].any()
    lens = np.diff(M.indptr)
    assert lens[3] == 0 and lens.max() > 16
    M2 = ep.missed_rows_mask()
    assert M2.nnz > 1000 and M2.has_canonical_format and M2.shape == (300, 300)
