"""Masked products (A*B and H*Q*H^T on a given pattern): the parts that need no GPU -- the library exports the new entry
points, the header declares them, the public functions are exported by both packages, the engine has its methods, and
argument errors come before any device work."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

NEW_SYMBOLS = ["smm_spgemm_masked", "smm_spgemm_masked_host", "smm_ctx_tune_masked", "smm_triple_product_sparse_masked"]


def test_library_exports_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES


def test_header_declares_the_new_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in text


def test_public_functions_in_both_packages():
    import inspect

    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    for name in ("masked_matrix_multiply", "sparse_triple_product"):
        assert name in sparse_matrix_mult_amd.__all__
        assert name in sparse_matrix_mult.__all__
        assert getattr(sparse_matrix_mult, name) is getattr(sparse_matrix_mult_amd, name)
    p = inspect.signature(sparse_matrix_mult_amd.sparse_triple_product).parameters
    assert "mask" in p and p["mask"].default is None


def test_engine_methods_exist():
    import inspect

    from sparse_matrix_mult_amd.engine import Context
    for name in ("spgemm_masked_host", "spgemm_masked_into", "tune_masked"):
        assert callable(getattr(Context, name))
    for name in ("triple_sparse_host", "triple_sparse_torch"):
        assert inspect.signature(getattr(Context, name)).parameters["mask"].default is None


def _no_device(monkeypatch):
    import sparse_matrix_mult_amd.matrix_ops as mo

    def boom():
        raise AssertionError("device work started before the arguments were checked")
    monkeypatch.setattr(mo, "default_context", boom)
    return mo


def _r(m, n, seed):
    return sp.random(m, n, density=0.5, format="csr", random_state=np.random.default_rng(seed))


def test_masked_shape_errors_before_any_device_work(monkeypatch):
    mo = _no_device(monkeypatch)
    A, B = _r(5, 7, 0), _r(7, 6, 1)
    with pytest.raises(ValueError, match="mask"):
        mo.masked_matrix_multiply(A, B, _r(5, 7, 2))
    with pytest.raises(ValueError, match="mask"):
        mo.masked_matrix_multiply(A, B, _r(6, 6, 2))
    with pytest.raises(ValueError, match="incompatible"):
        mo.masked_matrix_multiply(A, _r(6, 6, 3), _r(5, 6, 2))


def test_masked_triple_shape_errors_before_any_device_work(monkeypatch):
    mo = _no_device(monkeypatch)
    H = _r(5, 7, 0)
    Q = (_r(7, 7, 1) + _r(7, 7, 1).T).tocsr()
    with pytest.raises(ValueError, match="mask"):
        mo.sparse_triple_product(H, Q, mask=_r(5, 6, 2))
    with pytest.raises(ValueError, match="mask"):
        mo.sparse_triple_product(H, Q, mask=_r(7, 7, 2))
    with pytest.raises(ValueError, match="square"):
        mo.sparse_triple_product(H, _r(7, 6, 3), mask=_r(5, 5, 2))
    with pytest.raises(ValueError, match="incompatible"):
        mo.sparse_triple_product(H, sp.identity(6, format="csr"), mask=_r(5, 5, 2))


def test_empty_mask_gives_an_empty_csr_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    monkeypatch.setattr(mo, "_result_device", False)
    C = mo.masked_matrix_multiply(_r(4, 6, 0), _r(6, 3, 1), sp.csr_matrix((4, 3)))
    assert sp.isspmatrix_csr(C) and C.shape == (4, 3) and C.nnz == 0
    S = mo.sparse_triple_product(_r(4, 6, 0), sp.identity(6, format="csr"), mask=sp.csr_matrix((4, 4)))
    assert sp.isspmatrix_csr(S) and S.shape == (4, 4) and S.nnz == 0


def test_zero_operand_gives_the_mask_pattern_filled_with_positive_zeros(monkeypatch):
    mo = _no_device(monkeypatch)
    monkeypatch.setattr(mo, "_result_device", False)
    # a non-canonical mask with a duplicate and an explicit zero: canonicalised on a host copy, zeros stay positions
    M = sp.csr_matrix((np.array([1.0, 0.0, 2.0, 5.0]), np.array([2, 0, 2, 1]), np.array([0, 3, 3, 4])), shape=(3, 3))
    for A, B in ((sp.csr_matrix((3, 4)), _r(4, 3, 1)), (_r(3, 4, 0), sp.csr_matrix((4, 3)))):
        C = mo.masked_matrix_multiply(A, B, M)
        assert C.shape == (3, 3)
        assert np.array_equal(C.indptr, [0, 2, 2, 3]) and np.array_equal(C.indices, [0, 2, 1])
        assert np.array_equal(C.data.view(np.int64), np.zeros(3, dtype=np.int64))
    assert M.nnz == 4, "the caller's mask was modified"
    L = sp.csr_matrix(np.array([[1.0, 0, 1], [1, 1, 0], [0, 1, 0]]))
    S = mo.sparse_triple_product(sp.csr_matrix((3, 4)), sp.identity(4, format="csr"), mask=L)
    assert np.array_equal(S.indptr, [0, 2, 3, 3]) and np.array_equal(S.indices, [0, 2, 1])
    S = mo.sparse_triple_product(sp.csr_matrix((3, 4)), sp.identity(4, format="csr"), mask=L, compute_full_matrix=True)
    assert np.array_equal(S.indptr, [0, 2, 3, 4]) and np.array_equal(S.indices, [0, 2, 1, 0])
    assert np.array_equal(S.data.view(np.int64), np.zeros(4, dtype=np.int64))
