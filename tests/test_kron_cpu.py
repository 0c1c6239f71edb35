"""The Kronecker operand on the host: the restatement itself against scipy, and everything the public interface decides
before a device is touched (argument errors, empty factors, KroneckerOperand's own methods, the host CG path).  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from cg_restatement import diag_csr, local_h, rhs
from kron_restatement import canonical_pair, closed_form_indptr, kron_bound, restate_kron_apply, restate_kron_build, tridiag
from spmm_restatement import raw_csr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to get the library's context fails the test."""
    from sparse_matrix_mult_amd import matrix_ops

    def refuse():
        raise AssertionError("a device context was requested")

    monkeypatch.setattr(matrix_ops, "default_context", refuse)


def test_build_restatement_is_scipy_kron_bit_for_bit():
    D, E = canonical_pair()
    ptr, idx, val = restate_kron_build(D, E)
    K = sp.kron(D, E, format="csr")
    assert len(K.data) == D.nnz * E.nnz, "scipy kept the explicit zero as an entry"
    assert np.array_equal(ptr, K.indptr) and np.array_equal(idx, K.indices)
    assert np.array_equal(_bits(val), _bits(K.data))
    assert np.array_equal(ptr, closed_form_indptr(D, E))
    assert all(np.all(np.diff(idx[ptr[i]:ptr[i + 1]]) > 0) for i in range(len(ptr) - 1)), "rows strictly ascending"


def test_closed_form_row_pointer_for_non_canonical_factors():
    rng = np.random.default_rng(5)
    D = raw_csr([0, 3, 3, 5], [2, 0, 2, 1, 1], rng.uniform(-1, 1, 5), (3, 4))
    E = raw_csr([0, 0, 4, 5], [1, 1, 0, 2, 0], rng.uniform(-1, 1, 5), (3, 3))
    ptr, idx, val = restate_kron_build(D, E)
    assert np.array_equal(ptr, closed_form_indptr(D, E)) and ptr[-1] == 25
    # row (0, 1): D's entries (2, 0, 2) outside, E's (1, 1, 0, 2) inside
    assert idx[ptr[1]:ptr[2]].tolist() == [7, 7, 6, 8, 1, 1, 0, 2, 7, 7, 6, 8]
    assert np.array_equal(_bits(val[ptr[1]:ptr[2]]), _bits(np.multiply.outer(D.data[:3], E.data[:4]).ravel()))


def test_build_restatement_special_values():
    D = raw_csr([0, 2], [0, 1], [np.inf, -0.0], (1, 2))
    E = raw_csr([0, 2], [0, 1], [0.0, 2.0], (1, 2))
    _, _, val = restate_kron_build(D, E)
    assert np.isnan(val[0]) and val[1] == np.inf and np.array_equal(_bits(val[2:]), _bits([-0.0, -0.0]))


@pytest.mark.parametrize("k", [1, 3, 16])
def test_apply_restatement_is_within_the_bound_of_kron_times_x(k):
    D, E = canonical_pair()
    X = np.random.default_rng(k).standard_normal((D.shape[1] * E.shape[1], k))
    got = restate_kron_apply(D, E, X)
    want = sp.kron(D, E, format="csr") @ X
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= 1e-10 * kron_bound(D, E, X))
    # and it is scipy's two-step recipe bit for bit
    p, pc, r, rc = *D.shape, *E.shape
    U = np.stack([E @ X[t * rc:(t + 1) * rc] for t in range(pc)])
    two = np.asarray(D @ U.reshape(pc, r * k)).reshape(p * r, k)
    assert np.array_equal(_bits(got), _bits(two))
    x1 = X[:, 0].copy()
    assert np.array_equal(_bits(restate_kron_apply(D, E, x1)), _bits(got[:, 0]))


def test_kronecker_operand_shape_factors_and_to_scipy(no_device):
    from sparse_matrix_mult_amd import KroneckerOperand
    D, E = canonical_pair()
    Q = KroneckerOperand(D, E.toarray())                   # (anything csr_matrix() accepts; the dense form drops the explicit zero)
    assert Q.shape == (7 * 33, 5 * 29) and Q.factors[0] is D and sp.isspmatrix_csr(Q.factors[1])
    assert Q.nnz == D.nnz * (E.nnz - 1)
    S = KroneckerOperand(D, E).to_scipy()
    want = sp.kron(D, E, format="csr")
    assert sp.isspmatrix_csr(S) and S.shape == want.shape and (abs(S - want)).nnz == 0


def test_argument_errors_come_before_any_device_call(no_device):
    import sparse_matrix_mult_amd as smm
    D, E = canonical_pair()
    Q = smm.KroneckerOperand(D, E)
    X = np.zeros((Q.shape[1], 2))
    with pytest.raises(ValueError, match="rows"):
        smm.sparse_dense_multiply(Q, X[:-1])
    with pytest.raises(ValueError, match="1-D or 2-D"):
        smm.sparse_dense_multiply(Q, np.zeros((Q.shape[1], 2, 2)))
    with pytest.raises(ValueError, match=r"D\^T \(x\) E\^T"):
        smm.sparse_dense_multiply(Q, np.zeros((Q.shape[0], 2)), transpose=True)
    # everything else that takes a matrix points to kronecker_product
    for call in (lambda: smm.sparse_matrix_multiply(Q, Q), lambda: smm.sparse_matrix_multiply(D, Q),
                 lambda: smm.sparse_triple_product(Q, D), lambda: smm.sparse_triple_product(D, Q),
                 lambda: smm.masked_matrix_multiply(D, D, Q), lambda: smm.triple_product_apply(Q, D, X),
                 lambda: smm.sampled_dense_product(X, X, Q), lambda: smm.kronecker_product(Q, D),
                 lambda: smm.KroneckerOperand(D, Q), lambda: smm.pin_operand(Q)):
        with pytest.raises(ValueError, match="kronecker_product"):
            call()
    # Q of the triple forms: square factors, p r == K
    H = local_h(20, 7 * 33, 1)
    with pytest.raises(ValueError, match="square"):
        smm.triple_product_apply(H, Q, np.zeros((20, 2)))
    with pytest.raises(ValueError, match="square"):
        smm.innovation_solve(H, Q, None, np.zeros((20, 2)))
    Qs = smm.KroneckerOperand(tridiag(3), tridiag(5))
    with pytest.raises(ValueError, match="incompatible"):
        smm.triple_product_apply(H, Qs, np.zeros((20, 2)))
    with pytest.raises(ValueError, match="incompatible"):
        smm.innovation_solve(H, Qs, None, np.zeros((20, 2)))


def test_overflows_are_value_errors_with_small_arrays(no_device):
    import sparse_matrix_mult_amd as smm
    dense = sp.csr_matrix(np.ones((300, 300)))            # nnz 9e4 each: 8.1e9 entries
    with pytest.raises(ValueError, match="KroneckerOperand"):
        smm.kronecker_product(dense, dense)
    assert smm.KroneckerOperand(dense, dense).nnz == 8100000000      # ... which the factor form holds
    eye = sp.identity(50000, format="csr")                 # 2.5e9 rows
    with pytest.raises(ValueError, match="2\\^31"):
        smm.kronecker_product(eye, eye)
    with pytest.raises(ValueError, match="2\\^31"):
        smm.KroneckerOperand(eye, eye)
    # the largest that fits is not refused here: 46340^2 < 2^31 - 1 rows, one entry
    one = sp.csr_matrix(([1.0], ([0], [0])), shape=(46340, 1))
    assert smm.KroneckerOperand(one, one).shape == (46340 * 46340, 1)


def test_empty_factors_never_touch_a_device(no_device):
    import sparse_matrix_mult_amd as smm
    D, E = canonical_pair()
    Z = sp.csr_matrix((4, 6))
    for a, b in ((Z, E), (D, Z)):
        K = smm.kronecker_product(a, b)
        assert sp.isspmatrix_csr(K) and K.nnz == 0 and K.shape == (a.shape[0] * b.shape[0], a.shape[1] * b.shape[1])
        P = smm.kronecker_product(a, b, pin=True)
        assert isinstance(P, smm.PinnedOperand) and P.nnz == 0 and P.shape == K.shape
        Q = smm.KroneckerOperand(a, b)
        Y = smm.sparse_dense_multiply(Q, np.ones((Q.shape[1], 3)))
        assert Y.shape == (Q.shape[0], 3) and not Y.any()
        assert smm.sparse_dense_multiply(Q, np.ones(Q.shape[1])).shape == (Q.shape[0],)
    Qz = smm.KroneckerOperand(sp.csr_matrix((3, 3)), tridiag(5))
    H = sp.csr_matrix(np.ones((20, 15)))
    assert not smm.triple_product_apply(H, Qz, np.ones((20, 2))).any()
    Qn = smm.KroneckerOperand(tridiag(3), tridiag(5))
    assert smm.sparse_dense_multiply(Qn, np.zeros((15, 0))).shape == (15, 0)
    assert smm.triple_product_apply(H, Qn, np.zeros((20, 0))).shape == (20, 0)


def test_host_cg_path_with_a_q_without_entries(no_device):
    """S = 0: R Z = D is iterated on the host, exactly as with a CSR Q that has no entries."""
    import sparse_matrix_mult_amd as smm
    n, K = 40, 15
    H = sp.csr_matrix(np.random.default_rng(3).standard_normal((n, K)))
    r = np.random.default_rng(4).uniform(0.5, 2.0, n)
    Dm = rhs(n, 3, 5, zero_column=1)
    Qz = smm.KroneckerOperand(sp.csr_matrix((3, 3)), tridiag(5))
    Z, info = smm.innovation_solve(H, Qz, r, Dm, tol=1e-12)
    Zc, infoc = smm.innovation_solve(H, sp.csr_matrix((K, K)), diag_csr(r), Dm, tol=1e-12)
    assert info.converged and info.iterations[1] == 0 and not Z[:, 1].any()
    assert np.array_equal(_bits(Z), _bits(Zc)) and np.array_equal(info.iterations, infoc.iterations)
    assert np.allclose(Z, Dm / r[:, None], rtol=1e-10, atol=0)
    z1, info1 = smm.innovation_solve(H, Qz, None, Dm[:, 0].copy(), tol=1e-8, maxiter=3)      # S + R = 0: breakdown, reported
    assert z1.shape == (n,) and info1.status.tolist() == [2]
