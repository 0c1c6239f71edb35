"""Parametric covariances on a pattern: the parts that need no GPU -- properties of the numpy restatement of the contract
(what the GPU tests compare against), the exported symbols, argument errors and empty patterns before any device work."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

from cov_restatement import (MODELS, SQRT3, SQRT5, dense_covariance, entries, named_patterns, points, restate, taper_pattern)
from taper_restatement import dense_taper

NEW_SYMBOLS = ["smm_cov_eval", "smm_cov_eval_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------ the restatement
def test_constants_are_the_nearest_doubles():
    assert SQRT3 == float(np.sqrt(np.float64(3.0))) and SQRT5 == float(np.sqrt(np.float64(5.0)))
    from sparse_matrix_mult_amd.engine import COV_MODELS
    assert COV_MODELS == {name: k for k, name in enumerate(MODELS)}


@pytest.mark.parametrize("model", MODELS)
def test_value_at_distance_zero_is_the_variance_and_the_derivative_is_plus_zero(model):
    p = np.array([[0.3, -1.5, 2.0], [0.3, -1.5, 2.0]])
    rows, cols = np.array([0, 0, 1]), np.array([0, 1, 0])
    w = np.array([0.5, 1.25, 0.75])
    for variance in (2.5, 1.0, 0.0, 1e-300):
        for wrt in ("length", 0, 2):
            length = 1.3 if wrt == "length" else [0.9, 1.3, 2.1]
            val, dval = restate(p, None, rows, cols, model, length, variance, wrt)
            assert np.array_equal(_bits(val), _bits(np.full(3, variance)))
            assert np.array_equal(_bits(dval), _bits(np.zeros(3)))
            val, dval = restate(p, None, rows, cols, model, length, variance, wrt, weights=w)
            assert np.array_equal(_bits(val), _bits(variance * w)) and np.array_equal(_bits(dval), _bits(np.zeros(3)))


def test_spherical_is_exactly_zero_at_and_beyond_one():
    a = np.zeros((1, 1))
    b = np.array([1.0, np.nextafter(1.0, 2.0), 1.5, 7.0, 1e150, np.nextafter(1.0, 0.0)]).reshape(-1, 1)
    rows, cols = np.zeros(6, dtype=int), np.arange(6)
    val, dval = restate(a, b, rows, cols, "spherical", 1.0, 2.5, "length")
    assert np.array_equal(_bits(val[:5]), _bits(np.zeros(5))) and np.array_equal(_bits(dval[:5]), _bits(np.zeros(5)))
    assert val[5] > 0.0 and dval[5] > 0.0                          # just inside: the polynomial
    val, dval = restate(a * 2.0, b * 2.0, rows, cols, "spherical", 2.0, 2.5, 0)
    assert np.array_equal(_bits(val[:5]), _bits(np.zeros(5))) and np.array_equal(_bits(dval[:5]), _bits(np.zeros(5)))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_square_case_on_a_symmetric_pattern_is_symmetric_bit_for_bit(dim):
    L = taper_pattern(dim)
    rows, cols, w = entries(L)
    p = points(300, dim)
    length = [0.9, 1.3, 2.1][:dim]
    for model in MODELS:
        for wrt, ell in ((dim - 1, length), ("length", 1.1)):
            for weights in (None, w):
                for part in restate(p, None, rows, cols, model, ell, 2.5, wrt, weights):
                    M = sp.csr_matrix((part, L.indices, L.indptr), shape=L.shape)
                    T = M.T.tocsr()
                    T.sort_indices()
                    assert np.array_equal(T.indices, M.indices) and np.array_equal(_bits(T.data), _bits(M.data)), (model, wrt)


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("model", MODELS)
def test_derivative_against_central_differences(model, dim):
    """dQ against (Q(l + s) - Q(l - s)) / 2 s of the restated value, s = 1e-4, lengths near 1, variance 2.5: within 1e-6
    (2.6e-8 was observed for the four smooth models).  The spherical model has a kink at h = 1: pairs with |h - 1| <= 1e-3
    are left out, and are under 1 % of the pairs."""
    rng = np.random.default_rng(700 + dim)
    n, step, variance = 20000, 1e-4, 2.5
    a, b = rng.random((n, dim)) * 2.0, rng.random((n, dim)) * 2.0
    rows = cols = np.arange(n)
    worst = 0.0
    cases = [("length", 0.9 + 1.2 * rng.random())] + [(t, 0.9 + 1.2 * rng.random(dim)) for t in range(dim)]
    for wrt, length in cases:
        def shifted(s):
            ell = np.array(length, dtype=np.float64, copy=True)
            if wrt == "length":
                return ell + s
            ell[wrt] += s
            return ell
        _, d = restate(a, b, rows, cols, model, length, variance, wrt)
        up, down = (restate(a, b, rows, cols, model, shifted(s), variance)[0] for s in (step, -step))
        err = np.abs(d - (up - down) / (2.0 * step))
        if model == "spherical":
            from cov_restatement import lengths_of, scaled
            h = scaled(a, b, rows, cols, lengths_of(length, dim))[2]
            kink = np.abs(h - 1.0) <= 1e-3
            assert kink.mean() < 0.01
            err = err[~kink]
        worst = max(worst, float(err.max()))
    print(model, dim, "largest difference from central differences", worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_tapered_covariance_of_random_points_is_positive_semidefinite(dim):
    p = np.random.default_rng(20 + dim).random((400, dim))
    for model in MODELS:
        for cutoff, length in ((0.3, 0.2), (1.0, 0.7)):
            low = np.linalg.eigvalsh(dense_taper(p, cutoff) * dense_covariance(p, model, length, 2.5)).min()
            print(dim, model, cutoff, length, "smallest eigenvalue", low)
            assert low > -1e-10


def test_named_patterns_hold_what_their_names_say():
    P = named_patterns()
    lens = np.diff(P["arrow"].indptr)
    assert lens.max() == P["arrow"].shape[1] and (lens == 0).sum() == 37
    assert np.all(np.diff(P["two_per_row"].indptr) == 2) and P["two_per_row"].shape[0] == 5000
    U = P["unsorted_repeated"]
    row = U.indices[U.indptr[1]:U.indptr[2]]
    assert np.any(np.diff(row) < 0) and len(set(row.tolist())) < row.size
    assert P["rectangular"].shape == (37, 300) and P["rectangular"].indptr[-1] == 900
    for dim in (1, 2, 3):
        L = taper_pattern(dim)
        assert L.shape == (300, 300) and L.has_canonical_format and L.nnz > 300
        assert (abs(L - L.T)).nnz == 0


# ------------------------------------------------------------------------------ API and errors
def test_library_exports_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES and len(V2_PROTOTYPES[name][1]) == 16


def test_header_declares_the_new_entry_points_and_models():
    text = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in text
    from sparse_matrix_mult_amd import _lib
    for k, name in enumerate(MODELS):
        assert f"SMM_COV_{name.upper()} = {k}" in text and getattr(_lib, f"SMM_COV_{name.upper()}") == k
    assert "SMM_COV_WRT_NONE = -1" in text and "SMM_COV_WRT_ALL = 3" in text and "SMM_COV_SCALE_BY_PATTERN = 32" in text
    assert (_lib.SMM_COV_WRT_NONE, _lib.SMM_COV_WRT_ALL, _lib.SMM_COV_SCALE_BY_PATTERN) == (-1, 3, 32)


def test_public_names_in_both_packages_and_engine_methods():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    from sparse_matrix_mult_amd.engine import Context
    assert "covariance_on_pattern" in sparse_matrix_mult_amd.__all__ and "covariance_on_pattern" in sparse_matrix_mult.__all__
    assert sparse_matrix_mult.covariance_on_pattern is sparse_matrix_mult_amd.covariance_on_pattern
    p = inspect.signature(sparse_matrix_mult_amd.covariance_on_pattern).parameters
    assert list(p) == ["pattern", "coords", "model", "length", "variance", "coords_b", "scale_by_pattern", "derivative", "pin"]
    assert p["variance"].default == 1.0 and p["coords_b"].default is None and p["scale_by_pattern"].default is False
    assert p["derivative"].default is None and p["pin"].default is False
    assert list(inspect.signature(Context.cov_host).parameters)[1:6] == ["pattern", "a", "b", "model", "length"]
    assert list(inspect.signature(Context.cov_into).parameters)[1:6] == ["pattern", "d_a", "lda", "d_b", "ldb"]


def _no_device(monkeypatch):
    import sparse_matrix_mult_amd.matrix_ops as mo

    def boom():
        raise AssertionError("device work started before the arguments were checked")
    monkeypatch.setattr(mo, "default_context", boom)
    monkeypatch.setattr(mo, "_result_device", False)
    return mo


def test_argument_errors_before_any_device_work(monkeypatch):
    mo = _no_device(monkeypatch)
    P = np.random.default_rng(0).random((6, 2))
    L = sp.identity(6, format="csr")
    call = mo.covariance_on_pattern
    for bad in ("cubic", 1, None):
        with pytest.raises(ValueError, match="unknown model"):
            call(L, P, bad, 1.0)
    with pytest.raises(ValueError, match="4 coordinates"):
        call(L, np.ones((6, 4)), "gaussian", 1.0)
    with pytest.raises(ValueError, match="0 coordinates"):
        call(L, np.ones((6, 0)), "gaussian", 1.0)
    with pytest.raises(ValueError, match="dimensions"):
        call(L, np.ones((6, 2, 1)), "gaussian", 1.0)
    with pytest.raises(ValueError, match="coords_b has 3"):
        call(L, P, "gaussian", 1.0, coords_b=np.ones((6, 3)))
    for bad in (0.0, -1.0, np.inf, np.nan, "wide", None, [1.0, 0.0], [1.0, np.nan]):
        with pytest.raises(ValueError, match="length"):
            call(L, P, "gaussian", bad)
    for bad in ([1.0, 2.0, 3.0], [[1.0, 2.0]], []):
        with pytest.raises(ValueError, match="one number per coordinate"):
            call(L, P, "gaussian", bad)
    for bad in (np.inf, -np.inf, np.nan, "big", None):
        with pytest.raises(ValueError, match="variance"):
            call(L, P, "gaussian", 1.0, variance=bad)
    for bad in (2, -1, 3, "cutoff", 1.0, True):
        with pytest.raises(ValueError, match="derivative"):
            call(L, P, "gaussian", 1.0, derivative=bad)
    with pytest.raises(ValueError, match="common length"):
        call(L, P, "gaussian", [1.0, 1.0], derivative="length")         # (equal lengths, but not given as one)
    # the pattern's rows and columns against the numbers of points
    with pytest.raises(ValueError, match="the pattern is 6 x 6"):
        call(L, P[:5], "gaussian", 1.0)
    with pytest.raises(ValueError, match="the pattern is 6 x 6"):
        call(L, P, "gaussian", 1.0, coords_b=P[:4])
    with pytest.raises(ValueError, match="the pattern is 6 x 4"):
        call(sp.csr_matrix((6, 4)), P, "gaussian", 1.0)
    import torch
    with pytest.raises(ValueError, match="float64 CUDA"):
        call(L, torch.ones((6, 2), dtype=torch.float32), "gaussian", 1.0)
    with pytest.raises(ValueError, match="float64 CUDA"):
        call(L, P, "gaussian", 1.0, coords_b=torch.ones((6, 2), dtype=torch.float64))      # a CPU tensor
    with pytest.raises(ValueError, match="KroneckerOperand"):
        call(mo.KroneckerOperand(np.eye(2), np.eye(3)), P, "gaussian", 1.0)


def test_an_empty_pattern_returns_empty_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    for shape, a, b in (((5, 5), np.ones((5, 2)), None), ((3, 7), np.ones(3), np.ones(7)), ((0, 4), np.ones((0, 3)), np.ones((4, 3)))):
        E = sp.csr_matrix(shape)
        Q = mo.covariance_on_pattern(E, a, "matern32", 1.5, coords_b=b, scale_by_pattern=True)
        assert sp.isspmatrix_csr(Q) and Q.shape == shape and Q.nnz == 0
        pair = mo.covariance_on_pattern(E, a, "matern32", 1.5, coords_b=b, derivative="length")
        assert isinstance(pair, tuple) and len(pair) == 2 and all(sp.isspmatrix_csr(M) and M.shape == shape and M.nnz == 0 for M in pair)
        pinned = mo.covariance_on_pattern(E, a, "matern32", 1.5, coords_b=b, derivative=0, pin=True)
        assert len(pinned) == 2 and pinned[0] is not pinned[1]
        assert all(isinstance(M, mo.PinnedOperand) and M.shape == shape and M.nnz == 0 for M in pinned)
