"""Localisation tapers from coordinates: the parts that need no GPU -- properties of the numpy restatement of the contract
(what the GPU tests compare against), the exported symbols, argument errors and empty inputs before any device work, and
the refusal to pin a device result that does not fit an operand."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

from taper_restatement import (KINDS, NAMED_SETS, d2_matrix, dense_taper, gaspari_cohn_textbook, gc_far, gc_near, named_d2, point_set,
                               restate, restate_csr, weight)

NEW_SYMBOLS = ["smm_taper_build", "smm_taper_build_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------ the restatement
def test_weight_at_distance_zero_is_exactly_one():
    for cutoff in (1e-300, 0.1, 1.0, 4.6, 32.5, 1e300):
        assert weight(np.float64(0.0), cutoff, "gaspari_cohn") == 1.0
        assert weight(np.float64(0.0), cutoff, "boxcar") == 1.0


def test_the_two_branches_agree_at_z_equal_one():
    """Both branches at z = 1, where the function is 5/24: |near - far| = 1.1e-16, half an ulp of 1.0 -- the taper's own
    scale, w(0) = 1 (the far branch's intermediates reach 5, so each of its steps rounds by up to 4.4e-16)."""
    one = np.float64(1.0)
    near, far = gc_near(one), gc_far(one)
    print("near", repr(near), "far", repr(far), "difference", abs(near - far))
    assert abs(near - far) <= np.spacing(1.0)
    assert abs(near - 5.0 / 24.0) <= np.spacing(1.0) and abs(far - 5.0 / 24.0) <= np.spacing(1.0)
    assert weight(np.float64(1.0), 2.0, "gaspari_cohn") == near          # d2 = 1, c = 1: z <= 1 takes the near branch


def test_weights_lie_in_the_unit_interval_and_match_the_textbook_form():
    z = np.linspace(0.0, 2.0, 400001)[:-1]
    d2 = z * z                                                           # half-width 1: cutoff 2
    w = weight(d2, 2.0, "gaspari_cohn")
    assert w.min() >= 0.0 and w.max() <= 1.0
    raw = np.where(z <= 1.0, gc_near(z), gc_far(z))
    print("lowest unclamped value", raw.min(), "largest deviation from the power form", np.abs(raw - gaspari_cohn_textbook(z)).max())
    assert raw.min() < 0.0, "this order does dip below zero just inside z = 2: the clamp is needed"
    assert raw.min() > -1e-14
    assert np.abs(raw - gaspari_cohn_textbook(z)).max() <= 1e-14
    assert np.all(np.signbit(w) == False)                                # noqa: E712  (the clamp writes +0.0)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_square_case_equals_its_transpose_bit_for_bit(dim):
    p = np.random.default_rng(dim).random((300, dim)) * 3.0 - 1.0
    for kind in KINDS:
        L = restate_csr(p, None, 0.7, kind)
        T = L.T.tocsr()
        T.sort_indices()
        assert np.array_equal(L.indptr, T.indptr) and np.array_equal(L.indices, T.indices)
        assert np.array_equal(_bits(L.data), _bits(T.data))
        assert L.has_canonical_format


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_dense_taper_of_random_points_is_positive_semidefinite(dim):
    p = np.random.default_rng(10 + dim).random((400, dim))
    for cutoff in (0.1, 0.3, 1.0):
        low = np.linalg.eigvalsh(dense_taper(p, cutoff)).min()
        print(dim, cutoff, "smallest eigenvalue", low)
        assert low > -1e-10


def test_named_sets_hold_what_their_names_say():
    for dim in (1, 2, 3):
        for name, length in (("rows32", 32), ("rows33", 33), ("long_rows", 8200)):
            a, b, cutoff = point_set(name, dim)
            indptr, _, _ = restate(a, b, cutoff, "boxcar", named_d2(name, dim))
            assert np.all(np.diff(indptr) == length), (name, dim)
        a, _, cutoff = point_set("coincident", dim)
        d2 = named_d2("coincident", dim)
        assert np.all(d2[np.arange(100), 99 - np.arange(100)] == 0.0)    # point i and its copy 99 - i
        assert np.all(weight(d2[np.arange(100), 99 - np.arange(100)], cutoff, "gaspari_cohn") == 1.0)
        a, _, cutoff = point_set("integer_grid", dim)
        d2 = named_d2("integer_grid", dim)
        assert np.any(d2 == cutoff * cutoff), "pairs at exactly the cutoff exist"
        indptr, indices, _ = restate(a, None, cutoff, "boxcar", d2)
        rows = np.repeat(np.arange(len(a)), np.diff(indptr))
        assert np.all(d2[rows, indices] < cutoff * cutoff)
        a, _, cutoff = point_set("cell_boundaries", dim)
        d2 = named_d2("cell_boundaries", dim)
        assert a[:, 0].min() == 0.3
        assert np.any((d2 < cutoff * cutoff) & (d2 > 0.99 * cutoff * cutoff)), "partners just inside the cutoff"
        assert np.any(d2 == cutoff * cutoff) or np.any((d2 >= cutoff * cutoff) & (d2 < 1.01 * cutoff * cutoff))
    assert set(NAMED_SETS) >= {"two_clusters", "anisotropic", "offset_1e6", "negative", "rectangular"}


def test_restatement_follows_the_stated_order_of_the_distance():
    a = np.array([[0.1, 0.2, 0.3]])
    b = np.array([[0.7, -0.4, 1e-3]])
    d2 = 0.0
    for t in range(3):
        df = float(a[0, t]) - float(b[0, t])
        d2 = d2 + df * df
    assert _bits(d2_matrix(a, b))[0, 0] == _bits(np.array([d2]))[0]
    assert _bits(d2_matrix(b, a))[0, 0] == _bits(np.array([d2]))[0]      # the sign of df cannot matter


# ------------------------------------------------------------------------------ API and errors
def test_library_exports_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES and len(V2_PROTOTYPES[name][1]) == 11
    assert hasattr(lib, "smm_csr_copy_device") and len(V2_PROTOTYPES["smm_csr_copy_device"][1]) == 5


def test_header_declares_the_new_entry_points_and_kinds():
    text = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS + ["smm_csr_copy_device"]:
        assert f"{name}(" in text
    assert "SMM_TAPER_BOXCAR = 0" in text and "SMM_TAPER_GASPARI_COHN = 1" in text
    from sparse_matrix_mult_amd._lib import SMM_TAPER_BOXCAR, SMM_TAPER_GASPARI_COHN
    from sparse_matrix_mult_amd.engine import TAPER_KINDS
    assert (SMM_TAPER_BOXCAR, SMM_TAPER_GASPARI_COHN) == (0, 1)
    assert TAPER_KINDS == {"boxcar": 0, "gaspari_cohn": 1}


def test_public_names_in_both_packages_and_engine_methods():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    from sparse_matrix_mult_amd.engine import Context
    for name in ("localization_taper", "pin_operand", "PinnedOperand"):
        assert name in sparse_matrix_mult_amd.__all__ and name in sparse_matrix_mult.__all__
        assert getattr(sparse_matrix_mult, name) is getattr(sparse_matrix_mult_amd, name)
    p = inspect.signature(sparse_matrix_mult_amd.localization_taper).parameters
    assert list(p) == ["coords", "cutoff", "coords_b", "taper", "pin"]
    assert p["coords_b"].default is None and p["taper"].default == "gaspari_cohn" and p["pin"].default is False
    assert list(inspect.signature(Context.taper_host).parameters)[1:] == ["a", "b", "cutoff", "kind"]
    assert list(inspect.signature(Context.taper_into).parameters)[1:5] == ["d_a", "lda", "d_b", "ldb"]
    assert callable(sparse_matrix_mult_amd.PinnedOperand.to_scipy)


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
    for bad in (0.0, -1.0, np.inf, np.nan, "wide", None):
        with pytest.raises(ValueError, match="cutoff"):
            mo.localization_taper(P, bad)
    with pytest.raises(ValueError, match="unknown taper"):
        mo.localization_taper(P, 1.0, taper="gaussian")
    with pytest.raises(ValueError, match="unknown taper"):
        mo.localization_taper(P, 1.0, taper=1)
    with pytest.raises(ValueError, match="4 coordinates"):
        mo.localization_taper(np.ones((6, 4)), 1.0)
    with pytest.raises(ValueError, match="0 coordinates"):
        mo.localization_taper(np.ones((6, 0)), 1.0)
    with pytest.raises(ValueError, match="dimensions"):
        mo.localization_taper(np.ones((6, 2, 1)), 1.0)
    with pytest.raises(ValueError, match="dimensions"):
        mo.localization_taper(np.float64(1.0), 1.0)
    with pytest.raises(ValueError, match="coords_b has 3"):
        mo.localization_taper(P, 1.0, coords_b=np.ones((4, 3)))
    with pytest.raises(ValueError, match="coords_b has 1"):
        mo.localization_taper(P, 1.0, coords_b=np.ones(4))
    import torch
    with pytest.raises(ValueError, match="float64 CUDA"):
        mo.localization_taper(torch.ones((6, 2), dtype=torch.float32), 1.0)
    with pytest.raises(ValueError, match="float64 CUDA"):
        mo.localization_taper(P, 1.0, coords_b=torch.ones((6, 2), dtype=torch.float64))      # a CPU tensor


@pytest.mark.parametrize("shape, strides, dim, want", [
    ((7,), (0,), 1, (True, 1)),              # seven copies of one point (an expanded view): never read as seven doubles
    ((7,), (1,), 1, (False, 1)),
    ((7,), (2,), 1, (False, 2)),             # x[::2] stays where it is
    ((300, 2), (5, 1), 2, (False, 5)),       # a column slice of a wider tensor
    ((300, 2), (1, 300), 2, (True, 2)),      # a transpose
    ((1, 3), (0, 1), 3, (True, 3)),
    ((4, 3), (3, 1), 3, (False, 3)),
])
def test_row_layout_decides_between_in_place_and_a_copy(shape, strides, dim, want):
    """The one rule by which localization_taper and interpolation_operator hand a device view to the kernels, which read
    coordinate t of point i at x + i * ld + t: (copy_needed, ld)."""
    from sparse_matrix_mult_amd.matrix_ops import _row_layout
    assert _row_layout(shape, strides, dim) == want


def test_empty_inputs_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    for a, b, shape in ((np.ones((0, 3)), None, (0, 0)), (np.ones((0, 2)), np.ones((5, 2)), (0, 5)), (np.ones(4), np.ones(0), (4, 0))):
        L = mo.localization_taper(a, 1.0, coords_b=b)
        assert sp.isspmatrix_csr(L) and L.shape == shape and L.nnz == 0 and L.indices.dtype == np.int32
        P = mo.localization_taper(a, 1.0, coords_b=b, pin=True)
        assert isinstance(P, mo.PinnedOperand) and P.shape == shape and P.nnz == 0
        S = P.to_scipy()
        assert sp.isspmatrix_csr(S) and S.shape == shape and S.nnz == 0


class _Sized:
    """Stands in for a device tensor: a size and nothing else."""

    def __init__(self, n):
        self._n = n

    def numel(self):
        return self._n

    def __getattr__(self, name):
        raise AssertionError(f"a tensor of the refused result was touched ({name})")


def test_pinning_a_device_result_that_does_not_fit_is_refused(monkeypatch):
    mo = _no_device(monkeypatch)
    for nnz in (2 ** 31 - 1, 2 ** 31, 2 ** 33):
        res = mo.DeviceCSRResult(_Sized(1001), _Sized(nnz), _Sized(nnz), (1000, 1000))
        with pytest.raises(ValueError, match="does not fit an operand"):
            mo.pin_operand(res)
    res = mo.DeviceCSRResult(_Sized(2 ** 31 + 1), _Sized(10), _Sized(10), (2 ** 31, 5))
    with pytest.raises(ValueError, match="does not fit an operand"):
        mo.pin_operand(res)
