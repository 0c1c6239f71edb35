"""Sparse-output triple product and device CSR transpose: the parts that need no GPU -- the library exports the new
entry points, the public function is exported by both packages, and its argument errors come before any device work."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

NEW_SYMBOLS = ["smm_csr_transpose", "smm_csr_download", "smm_triple_product_sparse", "smm_ctx_tune_triple_sparse", "smm_result_nnz",
               "smm_result_rows", "smm_result_download", "smm_result_copy_device", "smm_result_destroy"]


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


def test_public_function_in_both_packages():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    assert "sparse_triple_product" in sparse_matrix_mult_amd.__all__
    assert "sparse_triple_product" in sparse_matrix_mult.__all__
    assert sparse_matrix_mult.sparse_triple_product is sparse_matrix_mult_amd.sparse_triple_product


def test_engine_methods_exist():
    from sparse_matrix_mult_amd.engine import Context
    for name in ("transpose", "triple_sparse_host", "triple_sparse_torch", "tune_triple_sparse"):
        assert callable(getattr(Context, name))


def _no_device(monkeypatch):
    import sparse_matrix_mult_amd.matrix_ops as mo

    def boom():
        raise AssertionError("device work started before the arguments were checked")
    monkeypatch.setattr(mo, "default_context", boom)
    return mo


def test_shape_errors_before_any_device_work(monkeypatch):
    mo = _no_device(monkeypatch)
    H = sp.random(5, 7, density=0.5, format="csr", random_state=np.random.default_rng(0))
    with pytest.raises(ValueError, match="square"):
        mo.sparse_triple_product(H, sp.random(7, 6, density=0.5, format="csr", random_state=np.random.default_rng(1)))
    with pytest.raises(ValueError, match="incompatible"):
        mo.sparse_triple_product(H, sp.identity(6, format="csr"))


def test_zero_operands_give_an_empty_csr_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    monkeypatch.setattr(mo, "_result_device", False)
    H = sp.csr_matrix((4, 6))
    Q = sp.identity(6, format="csr")
    S = mo.sparse_triple_product(H, Q)
    assert sp.isspmatrix_csr(S) and S.shape == (4, 4) and S.nnz == 0
    S = mo.sparse_triple_product(sp.random(3, 6, density=0.5, format="csr", random_state=np.random.default_rng(2)),
                                 sp.csr_matrix((6, 6)), compute_full_matrix=True)
    assert S.shape == (3, 3) and S.nnz == 0
