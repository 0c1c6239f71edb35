"""The empirical variogram on a pattern: the parts that need no GPU -- the numpy restatement of the contract (what the GPU
tests compare against bit for bit) against an independent evaluation, the exported symbols and constants, argument errors
and empty patterns before any device work."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from variogram_restatement import (MAX_BINS, RUN, T, bits, bound, edges_of, entries, flat_pattern, independent, points, restate, slots,
                                   taper_pattern, values)

NEW_SYMBOLS = ["smm_variogram", "smm_variogram_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _within(got, want, nnz, what):
    """Counts equal; sums within the derived bound of the correctly rounded sums (all terms are >= 0)."""
    assert np.array_equal(got[0], want[0]), what
    for g, w, part in ((got[1], want[1], "sum_h"), (got[2], want[2], "sum_sq")):
        rel = np.abs(g - w) / np.where(w > 0.0, w, 1.0)
        print(what, part, "largest relative distance from fsum", float(rel.max()), "bound", bound(nnz))
        assert np.all(rel <= bound(nnz)), (what, part, rel.max())
        assert np.array_equal(bits(g[want[0] == 0]), bits(np.zeros(int((want[0] == 0).sum())))), what


# ------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_restatement_on_a_taper_pattern_against_searchsorted_and_fsum(dim):
    L = taper_pattern(dim)
    rows, cols, _ = entries(L)
    p = points(300, dim)
    for k, nb, upper in ((1, 7, True), (3, 32, False), (3, 1, True)):
        e = edges_of(nb)
        _within(restate(p, values(300, k), rows, cols, e, upper), independent(p, values(300, k), rows, cols, e, upper), L.nnz,
                f"taper dim {dim} k {k} nb {nb} upper {upper}")


def test_restatement_on_a_flat_pattern_where_slots_hold_several_entries():
    nnz = 4 * T + 257                                              # 262 401 with the header's constants: four to eight entries per slot
    M = flat_pattern(nnz, 500, 500, 77)
    rows, cols, _ = entries(M)
    per_slot = np.bincount(slots(nnz), minlength=T)
    assert per_slot.min() == 4 and per_slot.max() == 8 and per_slot[64] == 5
    p = points(500, 2)
    e = edges_of(32, 3.6)
    got = restate(p, values(500, 3), rows, cols, e, False)
    _within(got, independent(p, values(500, 3), rows, cols, e, False), nnz, "flat")
    assert got[0].sum() == nnz                                     # every distance of the box is below the last edge


def test_slots_are_the_lane_map_of_runs_taken_round_robin():
    s = slots(2 * (T // 64) * RUN + 70)
    assert s[0] == 0 and s[63] == 63 and s[64] == 0 and s[RUN - 1] == 63 and s[RUN] == 64
    assert s[(T // 64) * RUN - 1] == T - 1 and s[(T // 64) * RUN] == 0 and s[-1] == 5
    assert T % 64 == 0 and RUN % 64 == 0 and T & (T - 1) == 0


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_upper_on_a_symmetric_pattern_counts_what_its_strict_upper_triangle_holds(dim):
    L = taper_pattern(dim)
    U = sp.triu(L, k=1).tocsr()
    p, v, e = points(300, dim), values(300, 3), edges_of(7)
    whole = restate(p, v, *entries(L)[:2], e, True)
    upper = restate(p, v, *entries(U)[:2], e, False)
    everything = restate(p, v, *entries(L)[:2], e, False)
    assert np.array_equal(whole[0], upper[0]) and whole[0].sum() > 0
    assert everything[0].sum() == 2 * whole[0].sum() + np.diff(L.indptr).size          # both triangles and the diagonal (in bin 0)
    assert everything[0][0] == 2 * whole[0][0] + 300


def test_bin_edges_are_met_by_comparison_and_nan_is_in_no_bin():
    x = np.array([0.0, 1.0, 2.0, 3.0, 0.0, np.nan])
    rows, cols = np.zeros(6, dtype=int), np.arange(6)
    count, sum_h, _ = restate(x, x, rows, cols, [0.0, 1.0, 2.0, 3.0], False)
    assert count.tolist() == [2, 1, 1] and sum_h.tolist() == [0.0, 1.0, 2.0]           # h = 3 = edges[nb] is left out
    count, _, _ = restate(x, x, rows, cols, [1.0, 2.0], False)
    assert count.tolist() == [1]


# ------------------------------------------------------------------------------ API and errors
def test_library_exports_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES and len(V2_PROTOTYPES[name][1]) == 14


def test_header_constants_are_the_packages():
    text = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in text
    from sparse_matrix_mult_amd import _lib
    for name in ("SMM_VG_RUN", "SMM_VG_SLOTS", "SMM_VG_MAX_BINS", "SMM_VG_ALL_ENTRIES"):
        found = re.findall(r"\b%s = (\d+)\b" % name, text)
        assert len(found) == 1 and int(found[0]) == getattr(_lib, name), name
    assert (T, RUN, MAX_BINS) == (_lib.SMM_VG_SLOTS, _lib.SMM_VG_RUN, _lib.SMM_VG_MAX_BINS)
    assert _lib.SMM_VG_SLOTS % 64 == 0 and _lib.SMM_VG_RUN % 64 == 0 and _lib.SMM_VG_ALL_ENTRIES not in (1, 2, 4, 8, 16, 32)
    kernel = open(os.path.join(ROOT, "sparse_matrix_mult_amd", "csrc", "smm_variogram.hpp")).read()
    assert "VG_RUN = SMM_VG_RUN" in kernel and "VG_SLOTS = SMM_VG_SLOTS" in kernel and "VG_MAX_BINS = SMM_VG_MAX_BINS" in kernel


def test_public_names_in_both_packages_and_engine_methods():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    from sparse_matrix_mult_amd.engine import Context
    for name in ("empirical_variogram", "VariogramResult"):
        assert name in sparse_matrix_mult_amd.__all__ and name in sparse_matrix_mult.__all__
        assert getattr(sparse_matrix_mult, name) is getattr(sparse_matrix_mult_amd, name)
    p = inspect.signature(sparse_matrix_mult_amd.empirical_variogram).parameters
    assert list(p) == ["pattern", "coords", "values", "bin_edges", "upper"] and p["upper"].default is True
    assert list(inspect.signature(Context.variogram_host).parameters)[1:] == ["pattern", "a", "y", "edges", "upper"]
    assert list(inspect.signature(Context.variogram_device).parameters)[1:] == ["pattern", "d_a", "lda", "dim", "d_y", "ldy", "k", "edges", "upper"]


def _no_device(monkeypatch):
    import sparse_matrix_mult_amd.matrix_ops as mo

    def boom():
        raise AssertionError("device work started before the arguments were checked")
    monkeypatch.setattr(mo, "default_context", boom)
    return mo


def test_argument_errors_before_any_device_work(monkeypatch):
    mo = _no_device(monkeypatch)
    P = np.random.default_rng(0).random((6, 2))
    V = np.arange(6.0)
    L = sp.identity(6, format="csr")
    E = [0.0, 0.5, 1.0]
    call = mo.empirical_variogram
    with pytest.raises(ValueError, match="4 coordinates"):
        call(L, np.ones((6, 4)), V, E)
    with pytest.raises(ValueError, match="0 coordinates"):
        call(L, np.ones((6, 0)), V, E)
    with pytest.raises(ValueError, match="dimensions"):
        call(L, np.ones((6, 2, 1)), V, E)
    with pytest.raises(ValueError, match="dimensions"):
        call(L, P, np.ones((6, 2, 1)), E)
    # the number of bins: 1 .. SMM_VG_MAX_BINS
    for bad in ([], [1.0], np.arange(MAX_BINS + 2.0), [[0.0, 1.0]], 1.0):
        with pytest.raises(ValueError, match="bin_edges must be 1-D"):
            call(L, P, V, bad)
    call_ok = np.arange(MAX_BINS + 1.0)                            # the most bins there are: refused only for want of a device
    with pytest.raises(AssertionError, match="device work started"):
        call(L, P, V, call_ok)
    for bad in ([0.0, np.inf], [0.0, np.nan, 1.0], [-np.inf, 1.0]):
        with pytest.raises(ValueError, match="finite"):
            call(L, P, V, bad)
    with pytest.raises(ValueError, match="sequence of numbers"):
        call(L, P, V, ["near", "far"])
    with pytest.raises(ValueError, match=">= 0"):
        call(L, P, V, [-0.5, 1.0])
    for bad in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [1.0, 0.0]):
        with pytest.raises(ValueError, match="ascend strictly"):
            call(L, P, V, bad)
    # a pattern that is not n x n, and n against the points and the values
    with pytest.raises(ValueError, match="must be square"):
        call(sp.csr_matrix((6, 4)), P, V, E)
    with pytest.raises(ValueError, match="the pattern is 6 x 6"):
        call(L, P[:5], V[:5], E)
    with pytest.raises(ValueError, match="the pattern is 6 x 6"):
        call(L, P, V[:5], E)
    with pytest.raises(ValueError, match="the pattern is 6 x 6"):
        call(L, P, np.ones((5, 3)), E)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="upper"):
            call(L, P, V, E, upper=bad)
    import torch
    with pytest.raises(ValueError, match="float64 CUDA"):
        call(L, torch.ones((6, 2), dtype=torch.float32), V, E)
    with pytest.raises(ValueError, match="float64 CUDA"):
        call(L, P, torch.ones(6, dtype=torch.float64), E)           # a CPU tensor
    with pytest.raises(ValueError, match="KroneckerOperand"):
        call(mo.KroneckerOperand(np.eye(2), np.eye(3)), P, V, E)


def test_an_empty_pattern_returns_zero_counts_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    for n, coords, vals in ((5, np.ones((5, 2)), np.ones(5)), (3, np.ones(3), np.ones((3, 4))), (0, np.ones((0, 3)), np.ones(0))):
        res = mo.empirical_variogram(sp.csr_matrix((n, n)), coords, vals, [0.0, 0.5, 1.0, 4.0])
        assert isinstance(res, mo.VariogramResult)
        assert res.count.dtype == np.int64 and res.count.tolist() == [0, 0, 0]
        assert np.array_equal(bits(res.sum_lag), bits(np.zeros(3))) and np.array_equal(bits(res.sum_sq), bits(np.zeros(3)))
        assert np.all(np.isnan(res.gamma)) and np.all(np.isnan(res.lag)) and res.edges.tolist() == [0.0, 0.5, 1.0, 4.0]


def test_result_divides_where_there_are_pairs():
    from sparse_matrix_mult_amd.matrix_ops import VariogramResult
    r = VariogramResult(np.array([0.0, 1.0, 2.0]), np.array([4, 0], dtype=np.int64), np.array([2.0, 0.0]), np.array([24.0, 0.0]), 3)
    assert r.lag[0] == 0.5 and r.gamma[0] == 1.0 and np.isnan(r.lag[1]) and np.isnan(r.gamma[1])
