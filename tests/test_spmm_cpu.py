"""Sparse x dense products (A X, A^T X, H Q H^T X): the parts that need no GPU -- the library exports the new entry
points, the header declares them, both packages export the public functions, the engine has its methods, argument
errors come before any device work, and the stored-order restatement of the contract equals the installed scipy bit for
bit on the shapes the GPU tests use."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from spmm_restatement import op_rows, operands, restate_spmm, restate_triple

NEW_SYMBOLS = ["smm_spmm", "smm_spmm_host", "smm_triple_apply", "smm_triple_apply_host", "smm_ctx_tune_spmm"]


def test_library_exports_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES


def test_header_declares_the_new_entry_points_and_flag():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in text
    assert "SMM_TRANSPOSE   = 16" in text
    from sparse_matrix_mult_amd._lib import SMM_TRANSPOSE
    assert SMM_TRANSPOSE == 16


def test_public_functions_in_both_packages():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    for name in ("sparse_dense_multiply", "triple_product_apply"):
        assert name in sparse_matrix_mult_amd.__all__
        assert name in sparse_matrix_mult.__all__
        assert getattr(sparse_matrix_mult, name) is getattr(sparse_matrix_mult_amd, name)


def test_engine_methods_exist():
    import inspect

    from sparse_matrix_mult_amd.engine import Context
    for name in ("spmm_host", "spmm_into", "triple_apply_host", "triple_apply_into", "tune_spmm"):
        assert callable(getattr(Context, name))
    p = inspect.signature(Context.spmm_into).parameters
    assert list(p)[1:8] == ["a", "d_x", "ldx", "k", "d_y", "ldy", "transpose"]


def _no_device(monkeypatch):
    import sparse_matrix_mult_amd.matrix_ops as mo

    def boom():
        raise AssertionError("device work started before the arguments were checked")
    monkeypatch.setattr(mo, "default_context", boom)
    monkeypatch.setattr(mo, "_result_device", False)
    return mo


def _r(m, n, seed):
    return sp.random(m, n, density=0.5, format="csr", random_state=np.random.default_rng(seed))


def test_argument_errors_before_any_device_work(monkeypatch):
    mo = _no_device(monkeypatch)
    A = _r(5, 7, 0)
    with pytest.raises(ValueError, match="rows"):
        mo.sparse_dense_multiply(A, np.ones((5, 3)))
    with pytest.raises(ValueError, match="rows"):
        mo.sparse_dense_multiply(A, np.ones(7), transpose=True)
    with pytest.raises(ValueError, match="dimensions"):
        mo.sparse_dense_multiply(A, np.ones((7, 2, 2)))
    with pytest.raises(ValueError, match="dimensions"):
        mo.sparse_dense_multiply(A, np.float64(1.0))
    Q = _r(7, 7, 1)
    with pytest.raises(ValueError, match="square"):
        mo.triple_product_apply(A, _r(7, 6, 2), np.ones(5))
    with pytest.raises(ValueError, match="incompatible"):
        mo.triple_product_apply(A, _r(6, 6, 2), np.ones(5))
    with pytest.raises(ValueError, match="rows"):
        mo.triple_product_apply(A, Q, np.ones((7, 2)))
    with pytest.raises(ValueError, match="dimensions"):
        mo.triple_product_apply(A, Q, np.ones((5, 1, 1)))


def test_empty_operands_and_k0_give_zeros_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    Y = mo.sparse_dense_multiply(sp.csr_matrix((4, 6)), np.ones((6, 3)))
    assert Y.shape == (4, 3) and np.array_equal(Y.view(np.int64), np.zeros((4, 3), dtype=np.int64))
    Y = mo.sparse_dense_multiply(sp.csr_matrix((4, 6)), np.ones(4), transpose=True)
    assert Y.shape == (6,) and not Y.any()
    Y = mo.sparse_dense_multiply(_r(4, 6, 0), np.ones((6, 0)))
    assert Y.shape == (4, 0)
    Y = mo.triple_product_apply(_r(4, 6, 0), sp.csr_matrix((6, 6)), np.ones((4, 2)))
    assert Y.shape == (4, 2) and not Y.any()


@pytest.mark.parametrize("name", list(operands()))
def test_restatement_equals_scipy_bit_for_bit(name):
    """The stored-order loop of the contract (the reference the GPU tests compare against) is scipy's A @ X, A.T @ X
    and H @ (Q @ (H.T @ X)) bit for bit on the operands of the GPU tests, for 1-D and 2-D X."""
    A = operands()[name]
    rng = np.random.default_rng(7)
    for transpose in (False, True):
        kx = op_rows(A, not transpose)
        for k in (1, 3, 8, 65):
            X = rng.standard_normal((kx, k))
            want = (A.T @ X) if transpose else (A @ X)
            got = restate_spmm(A, X, transpose)
            assert np.array_equal(got.view(np.int64), np.asarray(want).view(np.int64)), (name, transpose, k)
        x = rng.standard_normal(kx)
        want = (A.T @ x) if transpose else (A @ x)
        assert np.array_equal(restate_spmm(A, x, transpose).view(np.int64), np.asarray(want).view(np.int64))


def test_triple_restatement_equals_scipy_bit_for_bit():
    ops = operands()
    H = ops["unsorted_dup"]
    K = H.shape[1]
    Q = sp.random(K, K, density=0.05, format="csr", random_state=np.random.default_rng(3))   # not symmetric
    X = np.random.default_rng(4).standard_normal((H.shape[0], 5))
    want = H @ (Q @ (H.T @ X))
    assert np.array_equal(restate_triple(H, Q, X).view(np.int64), want.view(np.int64))


def test_restatement_signed_zeros():
    """+0.0 start: an empty row and a lone -0.0 product both give +0.0 (scipy agrees)."""
    A = sp.csr_matrix((np.array([-1.0]), np.array([0]), np.array([0, 1, 1])), shape=(2, 2))
    X = np.array([[0.0], [5.0]])
    Y = restate_spmm(A, X, False)
    assert np.array_equal(Y.view(np.int64), np.zeros((2, 1), dtype=np.int64))
    assert np.array_equal((A @ X).view(np.int64), Y.view(np.int64))
