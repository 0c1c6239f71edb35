"""smm_interp_build on the GPU: row pointer, columns and values compared bit for bit with the numpy restatement of the
contract (tests/interp_restatement.py), for every row count, grid and point placement at which the fill takes another
path, under both methods and the three policies for points outside the grid."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from interp_restatement import (COUNTS, GRIDS, METHODS, edges, grid, inside, midpoints, nonuniform, on_nodes, outside_count, restate,
                                restate_csr)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_same(got, want, what):
    """(indptr, indices, data) against the restatement: the pattern exactly, the values bit for bit."""
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert np.array_equal(got[0], want[0]), f"{what}: row pointer"
    assert np.array_equal(got[1], want[1]), f"{what}: columns"
    same = _bits(got[2]) == _bits(want[2])
    if not same.all():
        print(f"{what}: {int((~same).sum())} of {same.size} values differ, by at most {np.abs(got[2] - want[2]).max():.3e}")
    assert same.all(), f"{what}: values"


def _check(ctx, pts, axes, method, outside, what):
    held = ctx.live_bytes()
    h = ctx.interp_host(pts, axes, method, outside)
    try:
        assert (h.rows, h.cols) == (pts.shape[0], int(np.prod([a.size for a in axes])))
        assert h.is_canonical(), f"{what}: not canonical"
        _assert_same(h.to_host(), restate(pts, axes, method, outside), what)
    finally:
        h.close()
    assert ctx.live_bytes() == held, f"{what}: a temporary of the call is still handed out"


def _mixed_points(n, axes, seed):
    """n points: random inside, every fourth one on a node."""
    p = inside(n, axes, seed)
    p[::4] = on_nodes(n, axes, seed + 1)[::4]
    return p


# ------------------------------------------------------------------------------ row counts
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_row_counts_at_the_pairing_tail_wave_and_block_edges(ctx, dim, method):
    axes = grid("mixed", dim)
    for n in COUNTS:
        _check(ctx, _mixed_points(n, axes, 100 + n), axes, method, "error", f"n {n} dim {dim} {method}")


# ------------------------------------------------------------------------------ grids, placements, policies
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
@pytest.mark.parametrize("name", GRIDS)
def test_grids_and_point_placements_under_every_policy(ctx, name, dim):
    from sparse_matrix_mult_amd.engine import SmmError
    axes = grid(name, dim)
    ins = np.concatenate([inside(101, axes, 5 * dim), on_nodes(40, axes, 6 * dim), edges(axes, outside=False), midpoints(axes)])
    outs = np.concatenate([ins[:50], edges(axes, outside=True)])
    count = outside_count(outs, axes)
    assert count >= 4 * dim and outside_count(ins, axes) == 0
    for method in METHODS:
        for policy in ("error", "clamp", "zero"):
            _check(ctx, ins, axes, method, policy, f"{name} dim {dim} {method} {policy}, inside")
        for policy in ("clamp", "zero"):
            _check(ctx, outs, axes, method, policy, f"{name} dim {dim} {method} {policy}, outside")
        held = ctx.live_bytes()
        with pytest.raises(SmmError) as e:
            ctx.interp_host(outs, axes, method, "error")
        assert e.value.code == -2 and f"{count} points lie outside" in str(e.value)
        assert ctx.live_bytes() == held, "a block of the refused call is still handed out"


@pytest.mark.parametrize("nodes", [4096, 4097])
def test_axes_on_both_sides_of_the_size_that_is_searched_in_lds(ctx, nodes):
    axes = [nonuniform(nodes - 3, 60), nonuniform(3, 61)]
    pts = np.concatenate([_mixed_points(257, axes, 62), edges(axes, outside=True)])
    for method in METHODS:
        _check(ctx, pts, axes, method, "clamp", f"{nodes} nodes {method}")


def test_axes_read_where_they_are_give_the_same_bits(monkeypatch):
    """SMM_INTERP_STAGE=0: the searches read the axes through L2 instead of LDS."""
    from sparse_matrix_mult_amd.engine import Context
    monkeypatch.setenv("SMM_INTERP_STAGE", "0")
    c = Context(0)
    try:
        for dim in (1, 2, 3, 4):
            axes = grid("deep", dim)
            pts = np.concatenate([_mixed_points(257, axes, 70 + dim), edges(axes, outside=True)])
            for method in METHODS:
                _check(c, pts, axes, method, "zero", f"unstaged dim {dim} {method}")
    finally:
        c.close()


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_two_calls_give_the_same_bits(ctx, dim):
    axes = grid("deep", dim)
    pts = _mixed_points(1001, axes, 80 + dim)
    a, b = ctx.interp_host(pts, axes), ctx.interp_host(pts, axes)
    try:
        for x, y in zip(a.to_host(), b.to_host()):
            assert x.tobytes() == y.tobytes()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------ refusals
def test_non_finite_coordinates_are_refused_under_every_policy(ctx):
    from sparse_matrix_mult_amd.engine import SmmError
    axes = grid("uniform", 2)
    good = inside(100, axes, 11)
    held = ctx.live_bytes()
    for bad_value in (np.nan, np.inf, -np.inf):
        for policy in ("error", "clamp", "zero"):
            for method in METHODS:
                p = good.copy()
                p[37, 1] = bad_value
                p[5, 0] = bad_value
                p[5, 1] = bad_value
                with pytest.raises(SmmError) as e:
                    ctx.interp_host(p, axes, method, policy)
                assert e.value.code == -2 and "3 coordinates are not finite" in str(e.value)
                assert ctx.live_bytes() == held
    _check(ctx, good, axes, "linear", "error", "after the refusals")


def test_argument_refusals_leave_nothing_allocated(ctx):
    import torch
    from sparse_matrix_mult_amd.engine import SmmError
    dev = torch.device("cuda", ctx.device)
    axes = grid("uniform", 2)
    good = inside(10, axes, 12)
    d_good = torch.from_numpy(good).to(dev)
    held = ctx.live_bytes()
    host_cases = [
        ("dim 5", lambda: ctx.interp_host(np.ones((4, 5)), [axes[0]] * 5)),
        ("unknown method", lambda: ctx.interp_host(good, axes, 7)),
        ("unknown policy", lambda: ctx.interp_host(good, axes, "linear", 9)),
        ("axis of one node", lambda: ctx.interp_host(good, [axes[0], np.array([0.5])])),
        ("descending axis", lambda: ctx.interp_host(good, [axes[0], axes[1][::-1].copy()])),
        ("repeated node", lambda: ctx.interp_host(good, [axes[0], np.array([0.0, 1.0, 1.0, 2.0])])),
        ("NaN node", lambda: ctx.interp_host(good, [axes[0], np.array([0.0, np.nan, 2.0])])),
        ("infinite node", lambda: ctx.interp_host(good, [np.array([-np.inf, 0.0, 1.0]), axes[1]])),
        ("2^33 nodes", lambda: ctx.interp_host(np.ones((4, 3)), [np.arange(2.0 ** 11)] * 3)),
        ("2^31 nodes", lambda: ctx.interp_host(np.ones((4, 2)), [np.arange(2.0 ** 16), np.arange(2.0 ** 15)])),
        ("ldp < dim", lambda: ctx.interp_into(d_good, 1, 10, 2, axes)),
        ("n < 0", lambda: ctx.interp_into(d_good, 2, -1, 2, axes)),
        ("n = 2^31 - 1", lambda: ctx.interp_into(d_good, 2, 2 ** 31 - 1, 2, axes, "nearest")),
        ("NULL points", lambda: ctx.interp_into(0, 2, 10, 2, axes)),
    ]
    for what, call in host_cases:
        with pytest.raises(SmmError) as e:
            call()
        assert e.value.code == -2, f"{what}: {e.value}"
        assert ctx.live_bytes() == held, what
    for what, n, method in (("2^29 rows of 4", 2 ** 29, "linear"), ("2^31 - 2 rows of 4", 2 ** 31 - 2, "linear")):
        with pytest.raises(SmmError) as e:                           # (refused from the sizes alone: nothing is read)
            ctx.interp_into(d_good, 2, n, 2, axes, method)
        assert e.value.code == -5, f"{what}: {e.value}"
        assert ctx.live_bytes() == held, what
    lens = np.array([a.size for a in axes], dtype=np.int64)
    nodes = np.concatenate(axes)
    out = ctypes.c_void_p()
    lib, i64p, f64p = ctx.lib, lens.ctypes.data, nodes.ctypes.data
    assert lib.smm_interp_build(ctx.handle, 2, i64p, f64p, 0, 0, 10, d_good.data_ptr(), 2, None) == -2
    assert lib.smm_interp_build(ctx.handle, 2, None, f64p, 0, 0, 10, d_good.data_ptr(), 2, ctypes.byref(out)) == -2 and not out.value
    assert lib.smm_interp_build(ctx.handle, 2, i64p, None, 0, 0, 10, d_good.data_ptr(), 2, ctypes.byref(out)) == -2 and not out.value
    assert lib.smm_interp_build_host(ctx.handle, 2, i64p, f64p, 0, 0, 10, None, 2, ctypes.byref(out)) == -2 and not out.value
    assert ctx.live_bytes() == held
    empty = ctx.interp_host(np.ones((0, 2)), axes)
    try:
        assert (empty.rows, empty.cols, empty.nnz) == (0, axes[0].size * axes[1].size, 0) and empty.is_canonical()
        assert np.array_equal(empty.to_host()[0], np.zeros(1, dtype=np.int32))
    finally:
        empty.close()
    _check(ctx, good, axes, "linear", "error", "after the refusals")


def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_interp_build_host made to fail at its 1st, 2nd, ... device allocation (hard) until it succeeds -- the points'
    copy, the axes, the two counts and the operand's three arrays: each failure is SMM_ERR_ALLOC with nothing handed out,
    and the call that succeeds is right."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    axes = grid("mixed", 3)
    pts = np.concatenate([_mixed_points(300, axes, 90), edges(axes, outside=True)])
    want = restate(pts, axes, "linear", "clamp")
    try:
        failures = 0
        for nth in range(1, 33):
            c.release_pool()
            c.inject_alloc_failure(nth, hard=True)
            try:
                h = c.interp_host(pts, axes, "linear", "clamp")
            except SmmError as e:
                assert e.code == -3, f"allocation {nth}: {e}"
                assert c.live_bytes() == 0, f"allocation {nth}: {c.live_bytes()} bytes still handed out"
                failures += 1
                continue
            finally:
                c.inject_alloc_failure(0)
            try:
                _assert_same(h.to_host(), want, f"after {failures} failed allocations")
            finally:
                h.close()
            assert c.live_bytes() == 0
            break
        else:
            pytest.fail("never succeeded")
        assert failures == 6, f"{failures} allocations failed, the call makes 6"
    finally:
        c.close()


# ------------------------------------------------------------------------------ device input
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_column_slice_in_place_against_a_copy_and_numpy(ctx, dim):
    """ldp > dim: a column slice of a wider device tensor, used where it is."""
    import torch
    dev = torch.device("cuda", ctx.device)
    axes = grid("mixed", dim)
    host = np.random.default_rng(40 + dim).random((301, 6))
    host[:, 1:1 + dim] = _mixed_points(301, axes, 41 + dim)
    wide = torch.from_numpy(host).to(dev)
    pts = wide[:, 1:1 + dim]
    want = restate(host[:, 1:1 + dim], axes)
    sliced = ctx.interp_into(pts, 6, 301, dim, axes)
    copy = ctx.interp_into(pts.contiguous().clone(), dim, 301, dim, axes)
    from_host = ctx.interp_host(host[:, 1:1 + dim], axes)
    try:
        for h, what in ((sliced, "slice"), (copy, "contiguous copy"), (from_host, "numpy")):
            _assert_same(h.to_host(), want, what)
    finally:
        for h in (sliced, copy, from_host):
            h.close()
    from sparse_matrix_mult_amd import interpolation_operator
    H = interpolation_operator(pts if dim > 1 else pts[:, 0], axes if dim > 1 else axes[0])
    assert sp.isspmatrix_csr(H) and H.indices.dtype == np.int32 and H.has_canonical_format
    _assert_same((H.indptr, H.indices, H.data), want, "interpolation_operator on a slice")
    if dim == 1:                                                     # a view with stride 0 is copied, not read past its storage
        same = wide[3:4, 1].expand(7)
        H = interpolation_operator(same, axes[0])
        _assert_same((H.indptr, H.indices, H.data), restate(np.full(7, host[3, 1]), axes), "expanded view")


# ------------------------------------------------------------------------------ public path
def test_public_path_results_products_and_device_tensors(ctx):
    import torch
    from scipy.interpolate import RegularGridInterpolator
    import sparse_matrix_mult_amd as smm
    from sparse_matrix_mult_amd.engine import SmmError
    dev = torch.device("cuda", ctx.device)
    axes = grid("mixed", 3)
    pts = np.concatenate([_mixed_points(200, axes, 50), edges(axes, outside=False)])
    n = pts.shape[0]
    field = np.random.default_rng(51).standard_normal([a.size for a in axes])
    want = restate_csr(pts, axes)
    old_exact, old_dev = smm.set_exact(False), smm.set_result_device(False)
    Hp = None
    try:
        for method in METHODS:
            H = smm.interpolation_operator(pts, axes, method=method)
            _assert_same((H.indptr, H.indices, H.data), restate(pts, axes, method), f"scipy result, {method}")
        Hp = smm.interpolation_operator(pts, axes, pin=True)
        assert isinstance(Hp, smm.PinnedOperand) and Hp.shape == want.shape and Hp.nnz == want.nnz
        S = Hp.to_scipy()
        assert S.has_canonical_format
        _assert_same((S.indptr, S.indices, S.data), (want.indptr, want.indices, want.data), "pinned")
        # H field against scipy's interpolator, within the bound of tests/test_interp_cpu.py
        got = smm.sparse_dense_multiply(Hp, field.ravel())
        bound = 1e-14 * (abs(want) @ np.abs(field.ravel()))
        err = np.abs(got - RegularGridInterpolator(axes, field)(pts))
        print(f"worst |H field - RegularGridInterpolator| / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound)
        # H^T d against scipy, default mode: within 1e-10 (|H|^T |d|), the tolerance of tests/test_gpu_spmm.py
        d = np.random.default_rng(52).standard_normal((n, 3))
        got_t = smm.sparse_dense_multiply(Hp, d, transpose=True)
        assert np.all(np.abs(got_t - want.T @ d) <= 1e-10 * (abs(want).T @ np.abs(d)))
        # outside points through the public call
        out_pts = edges(axes, outside=True)
        with pytest.raises(SmmError) as e:
            smm.interpolation_operator(out_pts, axes)
        assert e.value.code == -2 and f"{outside_count(out_pts, axes)} points lie outside" in str(e.value)
        Z = smm.interpolation_operator(out_pts, axes, method="nearest", outside="zero")
        _assert_same((Z.indptr, Z.indices, Z.data), restate(out_pts, axes, "nearest", "zero"), "nearest, zero")
        # results left on the device
        smm.set_result_device(True)
        for source in (pts, torch.from_numpy(pts).to(dev)):
            R = smm.interpolation_operator(source, axes)
            assert isinstance(R, smm.DeviceCSRResult) and R.shape == want.shape and R.indptr.dtype == torch.int64
            assert R.indices.dtype == torch.int32 and R.data.is_cuda
            got_dev = (R.indptr.cpu().numpy().astype(np.int32), R.indices.cpu().numpy(), R.data.cpu().numpy())
            _assert_same(got_dev, (want.indptr, want.indices, want.data), "device result")
    finally:
        smm.set_exact(old_exact)
        smm.set_result_device(old_dev)
        if Hp is not None:
            Hp.unpin()


# ------------------------------------------------------------------------------ end to end
def test_solve_with_h_from_coordinates_and_a_kronecker_prior():
    """3 x 5 x 5 (time, y, x) grid, 40 points, Q = D (x) E: innovation_solve under set_exact(True) with H built on the
    device is bit-identical to the same call on the restatement's scipy H, and its true residual meets the bound
    tests/test_gpu_kron.py applies to its own solves (2 max(tol, the reference solve's residual))."""
    import sparse_matrix_mult_amd as smm
    from cg_restatement import dominant_diagonal, gaussian_band, true_residual
    tol = 1e-10
    axes = [np.array([0.0, 1.0, 2.5]), np.linspace(0.0, 1.0, 5), nonuniform(5, 33, 0.0, 2.0)]
    pts = _mixed_points(40, axes, 34)
    H_ref = restate_csr(pts, axes)
    D, E = gaussian_band(3, 1), gaussian_band(25, 3)
    Q = sp.kron(D, E, format="csr")
    r_diag = dominant_diagonal(H_ref, Q, 35)
    d = np.random.default_rng(36).standard_normal((40, 2))
    old_exact, old_dev = smm.set_exact(True), smm.set_result_device(False)
    Hp = None
    try:
        Z_ref, info_ref = smm.innovation_solve(H_ref, smm.KroneckerOperand(D, E), r_diag, d, tol=tol)
        assert info_ref.converged and np.all(info_ref.iterations > 1)
        Hp = smm.interpolation_operator(pts, axes, pin=True)
        Z, info = smm.innovation_solve(Hp, smm.KroneckerOperand(D, E), r_diag, d, tol=tol)
        assert np.array_equal(_bits(Z), _bits(Z_ref))
        assert np.array_equal(info.iterations, info_ref.iterations) and np.array_equal(info.status, info_ref.status)
        assert np.array_equal(_bits(info.residual_sq), _bits(info_ref.residual_sq))
        assert np.array_equal(_bits(info.rhs_sq), _bits(info_ref.rhs_sq))
        R = sp.diags(r_diag).tocsr()
        res, wres = true_residual(H_ref, Q, R, Z, d), true_residual(H_ref, Q, R, Z_ref, d)
        print("iterations", info.iterations.tolist(), "true residual / tol", (res / tol).tolist())
        assert np.all(res <= 2 * np.maximum(tol, wres))
    finally:
        smm.set_exact(old_exact)
        smm.set_result_device(old_dev)
        if Hp is not None:
            Hp.unpin()
