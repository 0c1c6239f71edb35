"""The observation operator from coordinates: the parts that need no GPU -- properties of the numpy restatement of the
contract (tests/interp_restatement.py: agreement with scipy's RegularGridInterpolator, the structure of a row, the three
policies for points outside the grid, the tie of NEAREST, the column order of KroneckerOperand), the exported entry
points, and the argument errors of interpolation_operator, which come before any device work."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.interpolate import RegularGridInterpolator

from interp_restatement import (EPS, GRIDS, METHODS, POLICIES, OutsideError, cells, edges, grid, inside, midpoints, nonuniform, on_nodes,
                                outside_count, restate, restate_csr, strides)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["smm_interp_build", "smm_interp_build_host"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _points(axes, seed):
    """Random inside, on nodes, on both ends of every axis and one ulp inside them, one ulp below a node."""
    return np.concatenate([inside(200, axes, seed), on_nodes(50, axes, seed + 1), edges(axes, outside=False)])


# ------------------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
@pytest.mark.parametrize("name", GRIDS)
def test_restatement_agrees_with_scipy_and_the_weights_sum_to_one(name, dim):
    """|H field - RegularGridInterpolator| <= 1e-14 sum_e |w_e| |field_e| per point: about 2^dim + 2 dim roundings on each
    side, under 24 eps at dim = 4 (a prototype gave 6e-16); and |sum_e w_e - 1| <= 8 eps (prototype: 4.5e-16)."""
    axes = grid(name, dim)
    pts = _points(axes, 10 * dim)
    field = np.random.default_rng(dim).standard_normal([a.size for a in axes])
    H = restate_csr(pts, axes)
    got = H @ field.ravel()
    want = RegularGridInterpolator(axes, field)(pts)
    bound = 1e-14 * (abs(H) @ np.abs(field.ravel()))
    err = np.abs(got - want)
    print(f"{name} dim {dim}: worst error / (sum |w| |field|) = {(err / np.maximum(bound, 1e-300)).max() * 1e-14:.2e}")
    assert np.all(err <= bound)
    sums = np.asarray(H.sum(axis=1)).ravel()
    print(f"{name} dim {dim}: worst |sum w - 1| = {np.abs(sums - 1.0).max():.2e}")
    assert np.abs(sums - 1.0).max() <= 8 * EPS


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
@pytest.mark.parametrize("name", GRIDS)
def test_structure_of_the_rows(name, dim):
    axes = grid(name, dim)
    pts = _points(axes, 30 + dim)
    n, E = pts.shape[0], 1 << dim
    K = int(np.prod([a.size for a in axes]))
    c, f, out = cells(pts, axes)
    assert not out.any() and np.all(f >= 0.0) and np.all(f <= 1.0)
    for t, a in enumerate(axes):
        assert np.all(f[pts[:, t] == a[-1], t] == 1.0)                 # exactly 1.0 on the last node
    ptr, idx, val = restate(pts, axes)
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and val.dtype == np.float64
    assert np.array_equal(ptr, np.arange(n + 1) * E)
    rows = idx.reshape(n, E)
    assert np.all(rows[:, 1:] > rows[:, :-1]) and rows.min() >= 0 and rows.max() < K
    assert restate_csr(pts, axes).has_canonical_format
    st = strides(axes)
    assert all(st[t] >= 2 * st[t + 1] for t in range(dim - 1)) and st[-1] == 1
    nptr, nidx, nval = restate(pts, axes, "nearest")
    assert np.array_equal(nptr, np.arange(n + 1)) and np.all(nval == 1.0) and nidx.min() >= 0 and nidx.max() < K
    # the nearest node is the corner with the largest weight (where that corner is unique)
    w = val.reshape(n, E)
    unique = (w == w.max(axis=1, keepdims=True)).sum(axis=1) == 1
    assert unique.sum() > n // 2
    assert np.array_equal(rows[np.arange(n), w.argmax(axis=1)][unique], nidx[unique])


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_a_point_on_a_node_gives_one_weight_of_one(dim):
    axes = grid("mixed", dim)
    rng = np.random.default_rng(dim)
    j = np.stack([rng.integers(0, a.size, 64) for a in axes], axis=1)
    pts = np.stack([a[j[:, t]] for t, a in enumerate(axes)], axis=1)
    ptr, idx, val = restate(pts, axes)
    w, cols = val.reshape(64, -1), idx.reshape(64, -1)
    assert np.all((w == 1.0).sum(axis=1) == 1) and np.all((w == 0.0).sum(axis=1) == (1 << dim) - 1)
    node = sum(j[:, t] * s for t, s in enumerate(strides(axes)))
    assert np.array_equal(cols[np.arange(64), w.argmax(axis=1)], node)
    assert np.array_equal(restate(pts, axes, "nearest")[1], node)


# ------------------------------------------------------------------------------ outside policies and NEAREST
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_policies_one_ulp_outside_either_end(dim):
    axes = grid("uniform", dim)
    base = inside(2 * dim, axes, 3)
    for t, a in enumerate(axes):
        for end, step in ((a[0], -np.inf), (a[-1], np.inf)):
            pts = base.copy()
            pts[0, t] = np.nextafter(end, step)                        # row 0 outside, the others inside
            edge = base.copy()
            edge[0, t] = end
            assert outside_count(pts, axes) == 1 and outside_count(edge, axes) == 0
            with pytest.raises(OutsideError) as e:
                restate(pts, axes, "linear", "error")
            assert e.value.count == 1
            for method in METHODS:
                on_edge = restate(edge, axes, method, "error")
                clamp = restate(pts, axes, method, "clamp")
                zero = restate(pts, axes, method, "zero")
                for got in (clamp, zero):                              # constant extrapolation: the row of the edge point
                    assert np.array_equal(got[0], on_edge[0]) and np.array_equal(got[1], on_edge[1])
                assert np.array_equal(_bits(clamp[2]), _bits(on_edge[2]))
                per_row = on_edge[0][1]
                assert np.array_equal(_bits(zero[2][:per_row]), np.zeros(per_row, dtype=np.int64))      # +0.0, not -0.0
                assert np.array_equal(_bits(zero[2][per_row:]), _bits(on_edge[2][per_row:]))
    far = base.copy()
    far[:, 0] = axes[0][-1] + 5.0
    with pytest.raises(OutsideError) as e:
        restate(far, axes)
    assert e.value.count == 2 * dim


def test_nearest_ties_go_to_the_lower_node():
    for dim in (1, 2, 3, 4):
        axes = [np.array([0.0, 1.0, 3.0, 4.0]) for _ in range(dim)]
        st = strides(axes)
        mid = midpoints(axes)
        assert np.all(cells(mid, axes)[1] == 0.5)
        assert restate(mid, axes, "nearest")[1][0] == 0
        above = np.nextafter(mid, np.inf)
        assert restate(above, axes, "nearest")[1][0] == sum(st)
        tie2 = np.full((1, dim), 2.0)                                  # half-way through the cell [1, 3]
        assert restate(tie2, axes, "nearest")[1][0] == sum(st)
        assert np.all(restate(tie2, axes, "linear")[2] == 0.5 ** dim)


# ------------------------------------------------------------------------------ the column order of KroneckerOperand
@pytest.mark.parametrize("space_dim", [1, 2, 3])
def test_time_as_axis_zero_is_a_kronecker_product_bit_for_bit(space_dim):
    """Points whose time coordinate is a node: H = sum over t of (selection of time t) (x) H_space -- row i of
    scipy.sparse.kron(e_t(i), H_space[i]) -- so column (t, j) of H is t * r + j, KroneckerOperand's."""
    t_axis = nonuniform(5, 50, 0.0, 10.0)
    space = grid("mixed", 4)[1:1 + space_dim]
    n = 40
    rng = np.random.default_rng(51)
    t_idx = rng.integers(0, t_axis.size, n)
    xs = inside(n, space, 52)
    pts = np.column_stack([t_axis[t_idx], xs])
    H = restate_csr(pts, [t_axis] + space)
    Hs = restate_csr(xs, space)
    r = Hs.shape[1]
    assert H.shape == (n, t_axis.size * r)
    for i in range(n):
        row = H[i]
        sel = sp.csr_matrix(([1.0], ([0], [t_idx[i]])), shape=(1, t_axis.size))
        want = sp.kron(sel, Hs[i], format="csr")
        stored = row.data != 0.0                                       # (H also stores the zero weights of the other time node)
        assert np.array_equal(row.indices[stored], want.indices[want.data != 0.0])
        assert np.array_equal(_bits(row.data[stored]), _bits(want.data[want.data != 0.0]))
        assert np.all(row.indices // r >= max(t_idx[i] - 1, 0)) and np.all(row.indices // r <= t_idx[i] + 1)
    # and as one matrix: the selection of time as a CSR of n rows, row-wise Kronecker (Khatri-Rao) product with H_space
    dense = np.zeros((n, t_axis.size * r))
    for i in range(n):
        dense[i, t_idx[i] * r:(t_idx[i] + 1) * r] = Hs[i].toarray().ravel()
    assert np.array_equal(_bits(H.toarray()), _bits(dense))


# ------------------------------------------------------------------------------ API and errors (these fail without the feature)
def test_library_exports_the_new_entry_points():
    from sparse_matrix_mult_amd._lib import LIB_PATH, V2_PROTOTYPES, _share_hip_runtime_with_torch
    assert os.path.exists(LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in V2_PROTOTYPES and len(V2_PROTOTYPES[name][1]) == 10


def test_header_declares_the_new_entry_points_and_constants():
    text = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in text
    assert "SMM_INTERP_LINEAR = 0, SMM_INTERP_NEAREST = 1" in text
    assert "SMM_INTERP_REJECT = 0, SMM_INTERP_CLAMP = 1, SMM_INTERP_ZERO = 2" in text
    from sparse_matrix_mult_amd import _lib
    from sparse_matrix_mult_amd.engine import INTERP_METHODS, INTERP_OUTSIDE
    assert (_lib.SMM_INTERP_LINEAR, _lib.SMM_INTERP_NEAREST) == (0, 1)
    assert (_lib.SMM_INTERP_REJECT, _lib.SMM_INTERP_CLAMP, _lib.SMM_INTERP_ZERO) == (0, 1, 2)
    assert INTERP_METHODS == {"linear": 0, "nearest": 1} and INTERP_OUTSIDE == {"error": 0, "clamp": 1, "zero": 2}
    assert tuple(INTERP_METHODS) == METHODS and tuple(INTERP_OUTSIDE) == POLICIES


def test_public_name_in_both_packages_and_engine_methods():
    import sparse_matrix_mult
    import sparse_matrix_mult_amd
    from sparse_matrix_mult_amd.engine import Context
    assert "interpolation_operator" in sparse_matrix_mult_amd.__all__ and "interpolation_operator" in sparse_matrix_mult.__all__
    assert sparse_matrix_mult.interpolation_operator is sparse_matrix_mult_amd.interpolation_operator
    p = inspect.signature(sparse_matrix_mult_amd.interpolation_operator).parameters
    assert list(p) == ["points", "axes", "method", "outside", "pin"]
    assert p["method"].default == "linear" and p["outside"].default == "error" and p["pin"].default is False
    assert list(inspect.signature(Context.interp_host).parameters)[1:] == ["points", "axes", "method", "outside"]
    assert list(inspect.signature(Context.interp_into).parameters)[1:] == ["d_pts", "ldp", "n", "dim", "axes", "method", "outside"]


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
    good = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    with pytest.raises(ValueError, match="not strictly ascending"):
        mo.interpolation_operator(P, [good[0], good[1][::-1]])                     # a descending axis
    with pytest.raises(ValueError, match="not strictly ascending"):
        mo.interpolation_operator(P, [good[0], np.array([0.0, 0.5, 0.5, 1.0])])    # a repeated node
    with pytest.raises(ValueError, match="at least 2"):
        mo.interpolation_operator(P, [good[0], np.array([0.5])])                   # an axis of length 1
    with pytest.raises(ValueError, match="not finite"):
        mo.interpolation_operator(P, [good[0], np.array([0.0, np.nan, 1.0])])
    with pytest.raises(ValueError, match="not finite"):
        mo.interpolation_operator(P, [good[0], np.array([0.0, 1.0, np.inf])])
    with pytest.raises(ValueError, match="5 axes"):
        mo.interpolation_operator(np.ones((6, 5)), [good[0]] * 5)                  # dim 5
    with pytest.raises(ValueError, match="0 axes"):
        mo.interpolation_operator(P, [])
    with pytest.raises(ValueError, match="unknown method"):
        mo.interpolation_operator(P, good, method="cubic")
    with pytest.raises(ValueError, match="unknown method"):
        mo.interpolation_operator(P, good, method=0)
    with pytest.raises(ValueError, match="unknown policy"):
        mo.interpolation_operator(P, good, outside="wrap")
    with pytest.raises(ValueError, match="3 coordinates per point, the grid has 2"):
        mo.interpolation_operator(np.ones((6, 3)), good)                           # the wrong number of columns
    with pytest.raises(ValueError, match="1 coordinates per point, the grid has 2"):
        mo.interpolation_operator(np.ones(6), good)
    with pytest.raises(ValueError, match="dimensions"):
        mo.interpolation_operator(np.ones((6, 2, 1)), good)
    with pytest.raises(ValueError, match="1-D"):
        mo.interpolation_operator(P, [good[0], np.ones((2, 2))])
    big = [np.arange(2.0 ** 11)] * 3                                               # 2^33 nodes
    with pytest.raises(ValueError, match="below 2\\^31 - 1"):
        mo.interpolation_operator(np.ones((6, 3)), big)
    import torch
    with pytest.raises(ValueError, match="float64 CUDA"):
        mo.interpolation_operator(torch.ones((6, 2), dtype=torch.float32), good)
    with pytest.raises(ValueError, match="float64 CUDA"):
        mo.interpolation_operator(torch.ones((6, 2), dtype=torch.float64), good)   # a CPU tensor


def test_no_points_without_a_device(monkeypatch):
    mo = _no_device(monkeypatch)
    axes = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    for method in METHODS:
        H = mo.interpolation_operator(np.ones((0, 2)), axes, method=method)
        assert sp.isspmatrix_csr(H) and H.shape == (0, 20) and H.nnz == 0
        P = mo.interpolation_operator(np.ones((0, 2)), axes, method=method, pin=True)
        assert isinstance(P, mo.PinnedOperand) and P.shape == (0, 20) and P.nnz == 0
    H = mo.interpolation_operator(np.ones(0), np.linspace(0.0, 1.0, 7))            # one array: a line
    assert H.shape == (0, 7)


def test_valid_arguments_without_a_gpu_fail_loudly_not_through_a_fallback():
    from sparse_matrix_mult_amd._lib import SmmLibrary
    if SmmLibrary().get_lib().smm_device_count() > 0:
        pytest.skip("a GPU is visible here")
    from sparse_matrix_mult_amd import interpolation_operator
    from sparse_matrix_mult_amd.engine import SmmError
    axes = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    for pin in (False, True):
        with pytest.raises(SmmError) as e:
            interpolation_operator(np.random.default_rng(1).random((6, 2)), axes, pin=pin)
        assert e.value.code == -1 and "no CPU path" in str(e.value)
