"""Masked products with the factor form Q = D (x) E: the parts that need no GPU -- the entry points are declared and
exported, the public calls exist in both packages, the numpy restatement of the contract equals the CPU oracle on the
explicit operand bit for bit, and argument errors and empty cases are decided before any device context."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import arrays, shuffle_rows, upper_mask
from kron_masked_restatement import (band_mask, bits, factor_cases, h_for, positions, random_mask, restate_aq, restate_masked_aq,
                                     restate_masked_triple, same_bits_nan, special_system, unsorted_dup_system)
from kron_restatement import tridiag

NEW_SYMBOLS = ["smm_triple_product_sparse_masked_kron", "smm_spgemm_masked_kron", "smm_spgemm_masked_kron_host"]


def test_library_exports_and_header_declares_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES
        assert f"{name}(" in text


def test_public_calls_and_engine_methods_exist():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    from sparse_matrix_mult_amd.engine import Context
    for name in ("masked_matrix_multiply", "sparse_triple_product", "KroneckerOperand", "kronecker_product"):
        assert name in sparse_matrix_mult_amd.__all__ and name in sparse_matrix_mult.__all__
        assert getattr(sparse_matrix_mult, name) is getattr(sparse_matrix_mult_amd, name)
    for name in ("spgemm_masked_kron_host", "spgemm_masked_kron_into", "triple_sparse_host", "triple_sparse_torch"):
        assert callable(getattr(Context, name))


# ------------------------------------------------------------------------------ the restatement against the oracle
def _kron(D, E):
    Q = sp.kron(D, E, format="csr")
    assert len(Q.data) == D.nnz * E.nnz                     # explicit zeros stayed entries
    return Q


def _check_triple(oracle, H, D, E, L):
    want = oracle.triple(arrays(H), arrays(_kron(D, E)), H.shape[1])
    U = upper_mask(L)
    rows, cols = positions(U)
    got = restate_masked_triple(H, D, E, U)
    assert same_bits_nan(got, want[rows, cols]), "S differs from the oracle's triple product on kron(D, E)"
    return got


def _check_aq(oracle, A, D, E, M):
    Q = _kron(D, E)
    ptr, idx, val = oracle.sparse(arrays(A), arrays(Q), Q.shape[1])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(ptr))
    T, stored = restate_aq(A, D, E)
    S = np.zeros_like(stored)
    S[rows, idx] = True
    assert np.array_equal(S, stored), "the stored positions are not the SpGEMM pattern"
    assert same_bits_nan(T[rows, idx], val), "A Q differs from the oracle's SpGEMM on kron(D, E)"
    dense = oracle.dense(arrays(A), arrays(Q), Q.shape[1])
    # (the dense oracle sums into calloc's +0.0, so a -0.0 of the first-touch sum is +0.0 there: equal as numbers)
    assert np.array_equal(np.where(stored, T, 0.0), dense, equal_nan=True)
    got = restate_masked_aq(A, D, E, M)
    mr, mc = positions(M)
    assert np.array_equal(bits(got[~stored[mr, mc]]), np.zeros(int((~stored[mr, mc]).sum()), np.int64)), "+0.0 where nothing reaches"
    return got


@pytest.mark.parametrize("name", ["tridiag5_taper33", "d_empty_rows", "explicit_zeros"])
def test_restatement_is_the_oracle_for_canonical_h(oracle, name):
    D, E = factor_cases()[name]
    H = h_for(D, E, lens=[0, 1, 8, 30, 8, 1, 30])
    n, K = H.shape
    _check_triple(oracle, H, D, E, sp.csr_matrix(np.ones((n, n))))
    _check_aq(oracle, H, D, E, random_mask(n, K, 0.3, 5))


def test_restatement_is_the_oracle_for_non_canonical_h(oracle):
    H, D, E = unsorted_dup_system()
    H = H[:40]
    H = sp.csr_matrix((H.data, H.indices, H.indptr), shape=H.shape)
    H.has_sorted_indices = False
    assert not H.has_canonical_format
    _check_triple(oracle, H, D, E, band_mask(40, 6))
    _check_aq(oracle, H, D, E, random_mask(40, 180, 0.2, 6))
    D2, E2 = factor_cases()["tridiag5_taper33"]
    H2 = shuffle_rows(h_for(D2, E2, lens=[8, 30, 1, 8]), 3)
    _check_triple(oracle, H2, D2, E2, sp.csr_matrix(np.ones((4, 4))))


@pytest.mark.parametrize("kind", ["unreached", "reached", "negzero"])
def test_restatement_is_the_oracle_for_special_values(oracle, kind):
    H, D, E = special_system(kind)
    n, K = H.shape
    full = sp.csr_matrix(np.ones((n, n)))
    S = _check_triple(oracle, H, D, E, full)
    C = _check_aq(oracle, H, D, E, sp.csr_matrix(np.ones((n, K))))
    if kind == "unreached":
        assert np.all(np.isfinite(C)), "an inf of H reached A Q through a pair the factors do not store"
        rows, cols = positions(upper_mask(full))
        off = ~np.isin(rows, [3, 6]) & ~np.isin(cols, [3, 6])
        assert np.all(np.isfinite(S[off]))
    elif kind == "reached":
        assert np.isinf(C).any() and np.isnan(C).any()
    else:
        assert np.all(C == 0) and np.signbit(C).any() and not np.signbit(C).all(), "both zeros occur"


# ------------------------------------------------------------------------------ before any device context
@pytest.fixture
def mo(monkeypatch):
    import sparse_matrix_mult_amd.matrix_ops as m

    def boom():
        raise AssertionError("device work started before the arguments were checked")
    monkeypatch.setattr(m, "default_context", boom)
    monkeypatch.setattr(m, "_result_device", False)
    return m


def _system():
    D, E = tridiag(3), tridiag(4)
    H = h_for(D, E, lens=[2, 0, 5, 1, 3])
    return H, D, E


def test_argument_errors_come_before_any_device_work(mo):
    H, D, E = _system()
    Q = mo.KroneckerOperand(D, E)
    L = sp.identity(5, format="csr")
    with pytest.raises(ValueError, match="kronecker_product"):
        mo.sparse_triple_product(H, Q)
    with pytest.raises(ValueError, match="mask="):
        mo.sparse_triple_product(H, Q)
    with pytest.raises(ValueError, match="mask"):
        mo.sparse_triple_product(H, Q, mask=sp.identity(4, format="csr"))
    with pytest.raises(ValueError, match="mask"):
        mo.masked_matrix_multiply(H, Q, sp.identity(5, format="csr"))
    R = mo.KroneckerOperand(sp.csr_matrix(np.ones((3, 2))), sp.csr_matrix(np.ones((4, 6))))          # 12 x 12, factors not square
    with pytest.raises(ValueError, match="square"):
        mo.sparse_triple_product(H, R, mask=L)
    for bad in (mo.KroneckerOperand(tridiag(3), tridiag(5)), mo.KroneckerOperand(tridiag(2), tridiag(4))):
        with pytest.raises(ValueError, match="incompatible"):
            mo.sparse_triple_product(H, bad, mask=L)
        with pytest.raises(ValueError, match="incompatible"):
            mo.masked_matrix_multiply(H, bad, sp.csr_matrix(np.ones((5, bad.shape[1]))))
    # a factor form in any other place is still refused, with the same pointer
    for call in (lambda: mo.sparse_triple_product(Q, D, mask=L), lambda: mo.sparse_triple_product(H, sp.identity(12, format="csr"), mask=Q),
                 lambda: mo.masked_matrix_multiply(Q, D, L), lambda: mo.masked_matrix_multiply(H, D, Q)):
        with pytest.raises(ValueError, match="kronecker_product"):
            call()


def test_empty_mask_gives_an_empty_csr(mo):
    H, D, E = _system()
    Q = mo.KroneckerOperand(D, E)
    S = mo.sparse_triple_product(H, Q, mask=sp.csr_matrix((5, 5)))
    assert sp.isspmatrix_csr(S) and S.shape == (5, 5) and S.nnz == 0
    C = mo.masked_matrix_multiply(H, Q, sp.csr_matrix((5, 12)))
    assert sp.isspmatrix_csr(C) and C.shape == (5, 12) and C.nnz == 0


def test_operand_without_entries_gives_the_pattern_of_positive_zeros(mo):
    H, D, E = _system()
    L = sp.csr_matrix(np.array([[1.0, 0, 1, 0, 0], [1, 1, 0, 0, 0], [0, 1, 0, 0, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 1]]))
    M = sp.csr_matrix((np.array([1.0, 0.0, 2.0, 5.0]), np.array([7, 0, 7, 1]), np.array([0, 3, 3, 4, 4, 4])), shape=(5, 12))
    Z = sp.csr_matrix
    for h, d, e in ((Z((5, 12)), D, E), (H, Z((3, 3)), E), (H, D, Z((4, 4)))):
        Q = mo.KroneckerOperand(d, e)
        S = mo.sparse_triple_product(h, Q, mask=L)
        assert np.array_equal(S.indptr, [0, 2, 3, 4, 4, 5]) and np.array_equal(S.indices, [0, 2, 1, 4, 4])
        assert np.array_equal(bits(S.data), np.zeros(5, np.int64))
        S = mo.sparse_triple_product(h, Q, mask=L, compute_full_matrix=True)
        assert np.array_equal(S.indptr, [0, 2, 3, 5, 5, 7]) and np.array_equal(S.indices, [0, 2, 1, 0, 4, 2, 4])
        assert np.array_equal(bits(S.data), np.zeros(7, np.int64))
        C = mo.masked_matrix_multiply(h, Q, M)
        assert np.array_equal(C.indptr, [0, 2, 2, 3, 3, 3]) and np.array_equal(C.indices, [0, 7, 1])
        assert np.array_equal(bits(C.data), np.zeros(3, np.int64))
    assert M.nnz == 4, "the caller's mask was modified"
