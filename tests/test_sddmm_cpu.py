"""The sampled dense product (X Y^T on a pattern): the parts that need no GPU -- the library exports the new entry
points, the header declares them, both packages export the public function, the engine has its methods, argument errors
and the degenerate cases come before any device work, and the numpy restatement of the contract (what the GPU tests
compare against) equals a plain Python float loop bit for bit."""
import ctypes
import inspect
import os
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from sddmm_restatement import KS, bound, entries, fma, masks, operands, partials, restate_default, restate_exact

NEW_SYMBOLS = ["smm_sddmm", "smm_sddmm_host", "smm_ctx_tune_sddmm"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_library_exports_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES
    assert len(V2_PROTOTYPES["smm_sddmm"][1]) == 9 and len(V2_PROTOTYPES["smm_sddmm_host"][1]) == 9


def test_header_declares_the_new_entry_points_and_flag():
    text = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in text
    assert "SMM_SCALE_BY_MASK = 32" in text
    from sparse_matrix_mult_amd._lib import SMM_SCALE_BY_MASK
    assert SMM_SCALE_BY_MASK == 32


def test_public_function_in_both_packages():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    assert "sampled_dense_product" in sparse_matrix_mult_amd.__all__
    assert "sampled_dense_product" in sparse_matrix_mult.__all__
    assert sparse_matrix_mult.sampled_dense_product is sparse_matrix_mult_amd.sampled_dense_product
    p = inspect.signature(sparse_matrix_mult_amd.sampled_dense_product).parameters
    assert list(p) == ["x", "y", "mask", "scale_by_mask"] and p["scale_by_mask"].default is False


def test_engine_methods_and_their_parameter_order():
    from sparse_matrix_mult_amd.engine import Context
    p = inspect.signature(Context.sddmm_host).parameters
    assert list(p)[1:] == ["mask", "x", "y", "scale", "exact"]
    assert p["scale"].default is False and p["exact"].default is False
    p = inspect.signature(Context.sddmm_into).parameters
    assert list(p)[1:] == ["mask", "d_x", "ldx", "d_y", "ldy", "k", "d_c", "scale", "exact"]
    p = inspect.signature(Context.tune_sddmm).parameters
    assert list(p)[1:] == ["mode"] and p["mode"].default == 0


def _no_device(monkeypatch):
    import sparse_matrix_mult_amd.matrix_ops as mo

    def boom():
        raise AssertionError("device work started before the arguments were checked")
    monkeypatch.setattr(mo, "default_context", boom)
    monkeypatch.setattr(mo, "_result_device", False)
    return mo


def test_argument_errors_before_any_device_work(monkeypatch):
    mo = _no_device(monkeypatch)
    L = sp.random(5, 7, density=0.5, format="csr", random_state=np.random.default_rng(0))
    X, Y = np.ones((5, 3)), np.ones((7, 3))
    with pytest.raises(ValueError, match="X has 4 rows"):
        mo.sampled_dense_product(np.ones((4, 3)), Y, L)
    with pytest.raises(ValueError, match="Y has 5 rows"):
        mo.sampled_dense_product(X, np.ones((5, 3)), L)
    with pytest.raises(ValueError, match="Y has 5 rows"):
        mo.sampled_dense_product(X, None, L)                       # y = x needs a square mask
    with pytest.raises(ValueError, match="columns"):
        mo.sampled_dense_product(X, np.ones((7, 4)), L)
    with pytest.raises(ValueError, match="dimensions"):
        mo.sampled_dense_product(np.ones(5), Y, L)
    with pytest.raises(ValueError, match="dimensions"):
        mo.sampled_dense_product(X, np.ones((7, 3, 1)), L)
    with pytest.raises(ValueError, match="dimensions"):
        mo.sampled_dense_product(np.float64(1.0), Y, L)
    import torch
    with pytest.raises(ValueError, match="float64 CUDA"):
        mo.sampled_dense_product(torch.ones((5, 3), dtype=torch.float32), Y, L)
    with pytest.raises(ValueError, match="float64 CUDA"):
        mo.sampled_dense_product(X, torch.ones((7, 3), dtype=torch.float64), L)      # a CPU tensor


def test_degenerate_cases_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    C = mo.sampled_dense_product(np.ones((4, 3)), np.ones((6, 3)), sp.csr_matrix((4, 6)))
    assert sp.isspmatrix_csr(C) and C.shape == (4, 6) and C.nnz == 0
    C = mo.sampled_dense_product(np.ones((0, 3)), np.ones((6, 3)), sp.csr_matrix((0, 6)))
    assert C.shape == (0, 6) and C.nnz == 0
    C = mo.sampled_dense_product(np.ones((4, 3)), np.ones((0, 3)), sp.csr_matrix((4, 0)))
    assert C.shape == (4, 0) and C.nnz == 0
    # k = 0: the mask's pattern (canonicalised) holding +0.0, or w * +0.0 when scaled
    L = sp.csr_matrix((np.array([2.0, -3.0, np.inf, 1.0]), np.array([3, 1, 0, 0]), np.array([0, 2, 2, 4])), shape=(3, 4))
    C = mo.sampled_dense_product(np.ones((3, 0)), np.ones((4, 0)), L)
    assert C.shape == (3, 4) and C.indptr.tolist() == [0, 2, 2, 3] and C.indices.tolist() == [1, 3, 0]
    assert np.array_equal(_bits(C.data), np.zeros(3, dtype=np.int64))
    C = mo.sampled_dense_product(np.ones((3, 0)), np.ones((4, 0)), L, scale_by_mask=True)
    assert C.indices.tolist() == [1, 3, 0]
    assert np.array_equal(_bits(C.data[:2]), _bits(np.array([-0.0, 0.0]))) and np.isnan(C.data[2])      # (inf + 1) * 0


def _python_loop(X, Y, rows, cols, weights):
    out = []
    for p in range(len(rows)):
        s = 0.0
        for e in range(X.shape[1]):
            s = s + float(X[rows[p], e]) * float(Y[cols[p], e])
        out.append(s if weights is None else float(weights[p]) * s)
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("name", ["identity", "two_per_row", "arrow", "noncanonical"])
def test_exact_restatement_equals_a_plain_float_loop(name):
    for k in (1, 3, 8, 65):
        M, X, Y = operands(name, k)
        rows, cols, w = entries(M)
        for weights in (None, w):
            got = restate_exact(X, Y, rows, cols, weights)
            assert np.array_equal(_bits(got), _bits(_python_loop(X, Y, rows, cols, weights))), (name, k)


@pytest.mark.parametrize("name", [n for n in masks() if n != "empty"])
def test_exact_restatement_is_close_to_the_matrix_product(name):
    for k in KS:
        M, X, Y = operands(name, k)
        rows, cols, _ = entries(M)
        got = restate_exact(X, Y, rows, cols)
        want = (X @ Y.T)[rows, cols]
        assert np.all(np.abs(got - want) <= 1e-12 * bound(X, Y, rows, cols)), (name, k)


def test_signed_zero_cases():
    rows, cols = np.array([0]), np.array([0])
    z = restate_exact(np.ones((1, 0)), np.ones((1, 0)), rows, cols)
    assert _bits(z)[0] == 0                                                    # k = 0: +0.0
    z = restate_exact(np.ones((1, 0)), np.ones((1, 0)), rows, cols, np.array([-2.0]))
    assert _bits(z)[0] == _bits(np.array([-0.0]))[0]                           # w * +0.0 keeps the weight's sign
    z = restate_exact(np.array([[-1.0]]), np.array([[0.0]]), rows, cols)
    assert _bits(z)[0] == 0                                                    # +0.0 + -0.0 = +0.0
    z = restate_exact(np.array([[np.inf, 1.0]]), np.array([[1.0, 1.0]]), rows, cols, np.array([0.0]))
    assert np.isnan(z[0])                                                      # 0 * inf: the multiply is carried out


def test_partials_depend_on_k_alone():
    assert [partials(k) for k in (0, 1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 1000)] == [8, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128,
                                                                                            128, 128]


def test_fma_emulation_rounds_once():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(400) * 10.0 ** rng.integers(-3, 4, 400)
    b = rng.standard_normal(400) * 10.0 ** rng.integers(-3, 4, 400)
    c = -(a * b) * (1 + rng.integers(-3, 4, 400) * 2.0 ** -52)                  # heavy cancellation: the product's low half decides
    c[::2] = rng.standard_normal(200)
    got = fma(a, b, c)
    want = np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.any(got != a * b + c), "the operands tell one rounding from two"


def test_default_restatement_is_within_the_bound_and_differs_from_exact():
    M, X, Y = operands("random", 257)
    rows, cols, w = entries(M)
    d, x = restate_default(X, Y, rows, cols, w), restate_exact(X, Y, rows, cols, w)
    assert np.all(np.abs(d - x) <= 1e-10 * bound(X, Y, rows, cols, w))
    assert np.any(d != x)
