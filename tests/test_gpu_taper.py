"""smm_taper_build on the GPU: the pattern compared exactly and the values bit for bit against the brute-force numpy
restatement of the contract (tests/taper_restatement.py), for every shape at which the kernels take another path."""
import numpy as np
import pytest
import scipy.sparse as sp

from taper_restatement import (COUNTS, DENSITIES, KINDS, NAMED_SETS, d2_matrix, density_cutoff, named_d2, point_set, restate,
                               restate_csr, uniform, uniform_d2)

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
        worst = np.abs(got[2] - want[2]).max()
        print(f"{what}: {int((~same).sum())} of {same.size} values differ, by at most {worst:.3e}")
    assert same.all(), f"{what}: values"


def _check(ctx, a, b, cutoff, d2, what):
    held = ctx.live_bytes()
    for kind in KINDS:
        h = ctx.taper_host(a, b, cutoff, kind)
        try:
            assert (h.rows, h.cols) == d2.shape
            assert h.is_canonical(), f"{what} {kind}: not canonical"
            _assert_same(h.to_host(), restate(a, b, cutoff, kind, d2), f"{what} {kind}")
        finally:
            h.close()
    assert ctx.live_bytes() == held, f"{what}: a temporary of the call is still handed out"


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("n", COUNTS)
def test_uniform_points_at_three_densities(ctx, n, dim):
    p = uniform(n, dim)
    for density in DENSITIES:
        _check(ctx, p, None, density_cutoff(n, dim, density), uniform_d2(n, dim), f"n {n} dim {dim} {density}")


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", NAMED_SETS)
def test_named_sets(ctx, name, dim):
    a, b, cutoff = point_set(name, dim)
    _check(ctx, a, b, cutoff, named_d2(name, dim), f"{name} dim {dim}")


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_square_result_equals_its_device_transpose_and_repeats(ctx, dim):
    p = uniform(257, dim, 9) * 4.0 - 2.0
    for kind in KINDS:
        h = ctx.taper_host(p, None, 0.9, kind)
        t = ctx.transpose(h)
        again = ctx.taper_host(p, None, 0.9, kind)
        try:
            got = h.to_host()
            assert got[1].size > 257
            for other, what in ((t.to_host(), "transpose"), (again.to_host(), "second call")):
                assert np.array_equal(got[0], other[0]) and np.array_equal(got[1], other[1]), what
                assert np.array_equal(_bits(got[2]), _bits(other[2])), what
        finally:
            for x in (h, t, again):
                x.close()


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_column_slice_in_place_and_own_buffer_against_a_copy(ctx, dim):
    """lda > dim: a column slice of a wider device tensor, used where it is; b as a's own buffer and b as an equal copy
    give the same bits."""
    import torch
    dev = torch.device("cuda", ctx.device)
    wide = torch.from_numpy(np.random.default_rng(40 + dim).random((300, 5)) * 3.0).to(dev)
    pts = wide[:, 1:1 + dim]
    host = wide.cpu().numpy()[:, 1:1 + dim]
    want = restate(host, None, 0.8, "gaspari_cohn")
    own = ctx.taper_into(pts, 5, pts, 5, 300, 300, dim, 0.8)
    copy = ctx.taper_into(pts, 5, pts.contiguous().clone(), dim, 300, 300, dim, 0.8)
    try:
        _assert_same(own.to_host(), want, "own buffer")
        _assert_same(copy.to_host(), want, "equal copy")
    finally:
        own.close()
        copy.close()
    from sparse_matrix_mult_amd import PinnedOperand, localization_taper
    L = localization_taper(pts if dim > 1 else pts[:, 0], 0.8)
    assert sp.isspmatrix_csr(L) and L.indices.dtype == np.int32 and L.has_canonical_format
    _assert_same((L.indptr, L.indices, L.data), want, "localization_taper on a slice")
    P = localization_taper(pts, 0.8, pin=True)
    try:
        assert isinstance(P, PinnedOperand) and P.shape == (300, 300) and P.nnz == want[1].size
        S = P.to_scipy()
        _assert_same((S.indptr, S.indices, S.data), want, "pinned")
    finally:
        P.unpin()
    rect = localization_taper(host[:50], 0.8, coords_b=pts, taper="boxcar")
    _assert_same((rect.indptr, rect.indices, rect.data), restate(host[:50], host, 0.8, "boxcar"), "numpy against a tensor")


def test_an_expanded_view_is_copied_and_a_strided_one_is_used_in_place(ctx):
    """Points on a line as 1-D views of a wider device tensor.  Row stride 0 (seven copies of one point) is copied, never
    read as seven consecutive doubles; row stride 2 of a column (every other row) is read where it is.  Each result is, bit
    for bit, that of the same points as a numpy array (or a contiguous copy) and the restatement's."""
    import torch
    from sparse_matrix_mult_amd import localization_taper
    dev = torch.device("cuda", ctx.device)
    cutoff = 0.8
    wide = torch.from_numpy(np.random.default_rng(45).random((300, 5)) * 3.0).to(dev)
    same = wide[3:4, 1].expand(7)                                    # cut from the middle of the storage
    assert same.stride() == (0,)
    point = wide[3, 1].item()
    copies = np.full(7, point)
    other5 = point + np.array([-1.0, -0.2, 0.0, 0.3, 2.0])            # three inside the cutoff, two outside

    def arrays(L):
        assert sp.isspmatrix_csr(L) and L.has_canonical_format
        return L.indptr, L.indices, L.data

    square = arrays(localization_taper(same, cutoff))
    _assert_same(square, arrays(localization_taper(copies, cutoff)), "expanded view, square: against numpy")
    _assert_same(square, restate(copies, None, cutoff, "gaspari_cohn"), "expanded view, square")
    assert square[1].size == 49 and np.all(square[2] == 1.0)
    rect = arrays(localization_taper(other5, cutoff, coords_b=same))
    _assert_same(rect, arrays(localization_taper(other5, cutoff, coords_b=copies)), "expanded view as coords_b: against numpy")
    _assert_same(rect, restate(other5, copies, cutoff, "gaspari_cohn"), "expanded view as coords_b")
    assert np.array_equal(np.diff(rect[0]), [0, 7, 7, 7, 0])

    strided = wide[::2, 1]
    assert strided.stride() == (10,)
    in_place = arrays(localization_taper(strided, cutoff))
    _assert_same(in_place, arrays(localization_taper(strided.contiguous(), cutoff)), "strided view: against its copy")
    _assert_same(in_place, restate(wide.cpu().numpy()[::2, 1], None, cutoff, "gaspari_cohn"), "strided view")


def test_non_finite_coordinates_are_refused_and_the_context_stays_usable(ctx):
    from sparse_matrix_mult_amd.engine import SmmError
    good = uniform(100, 2, 11)
    held = ctx.live_bytes()
    for bad_value in (np.nan, np.inf, -np.inf):
        for where in ("a", "b", "both"):
            a, b = good.copy(), uniform(80, 2, 12)
            if where in ("a", "both"):
                a[37, 1] = bad_value
            if where in ("b", "both"):
                b[5, 0] = bad_value
            with pytest.raises(SmmError) as e:
                ctx.taper_host(a, None if where == "both" else b, 0.3)
            assert e.value.code == -2 and "not finite" in str(e.value)
            assert ctx.live_bytes() == held
    for args in ((good, None, -1.0), (good, None, np.nan), (np.ones((4, 4)), None, 1.0)):
        with pytest.raises(SmmError) as e:
            ctx.taper_host(*args)
        assert e.value.code == -2
    with pytest.raises(SmmError) as e:
        ctx.taper_host(good, None, 0.3, kind=7)
    assert e.value.code == -2
    _check(ctx, good, None, 0.3, d2_matrix(good, good), "after the refusals")
    empty = ctx.taper_host(np.ones((0, 2)), good, 0.3)
    try:
        assert (empty.rows, empty.cols, empty.nnz) == (0, 100, 0) and empty.is_canonical()
    finally:
        empty.close()
    empty = ctx.taper_host(good, np.ones((0, 2)), 0.3)
    try:
        assert (empty.rows, empty.cols, empty.nnz) == (100, 0, 0)
        assert np.array_equal(empty.to_host()[0], np.zeros(101, dtype=np.int32))
    finally:
        empty.close()


def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_taper_build_host (a and b different: both counting sorts) made to fail at its 1st, 2nd, ... device allocation
    (hard) until it succeeds: each failure is SMM_ERR_ALLOC with nothing handed out, and the call that succeeds is right."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    a, b, cutoff = point_set("rectangular", 3)
    want = restate(a, b, cutoff, "gaspari_cohn", named_d2("rectangular", 3))
    try:
        failures = 0
        for nth in range(1, 65):
            c.release_pool()
            c.inject_alloc_failure(nth, hard=True)
            try:
                h = c.taper_host(a, b, cutoff)
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
        assert failures >= 10, f"only {failures} allocations failed"
    finally:
        c.close()


def test_the_chain_from_coordinates_to_the_solve_stays_on_the_device(monkeypatch):
    """L pinned from coordinates on the device, Q = L o (E E^T) pinned as a result left in HBM, innovation_solve under
    set_exact(True): Z and info bit-identical to the same chain fed with scipy matrices built from the restatement, no
    operand upload for L or Q and no download of an operand's arrays."""
    import torch
    import sparse_matrix_mult_amd as smm
    from sparse_matrix_mult_amd import matrix_ops as mo
    from sparse_matrix_mult_amd.engine import default_context
    rng = np.random.default_rng(300)
    K, n, width, k, cutoff = 300, 120, 8, 3, 0.25
    xy = rng.random((K, 2))
    E = rng.standard_normal((K, width))
    cols = np.stack([rng.choice(K, 3, replace=False) for _ in range(n)])
    H = sp.csr_matrix((rng.uniform(0.5, 1.5, 3 * n), cols.ravel().astype(np.int32), np.arange(0, 3 * n + 1, 3, dtype=np.int32)),
                      shape=(n, K))
    R = sp.diags(rng.uniform(1.0, 2.0, n)).tocsr()
    D = rng.standard_normal((n, k))
    old_exact, old_dev = smm.set_exact(True), smm.set_result_device(False)
    Hp = Rp = L = Q = None
    try:
        L_ref = restate_csr(xy, None, cutoff, "gaspari_cohn")
        Q_ref = smm.sampled_dense_product(E, None, L_ref, scale_by_mask=True)
        Z_ref, info_ref = smm.innovation_solve(H, Q_ref, R, D)
        assert info_ref.converged and np.all(info_ref.iterations > 1)

        dev = torch.device("cuda", default_context().device)
        Hp, Rp = smm.pin_operand(H), smm.pin_operand(R)
        uploads = mo.cache_stats["upload"]
        smm.set_result_device(True)
        from sparse_matrix_mult_amd.engine import DeviceCSR
        downloads = []
        to_host = DeviceCSR.to_host
        monkeypatch.setattr(DeviceCSR, "to_host", lambda self: downloads.append(self) or to_host(self))
        L = smm.localization_taper(torch.from_numpy(xy).to(dev), cutoff, pin=True)
        res = smm.sampled_dense_product(torch.from_numpy(E).to(dev), None, L, scale_by_mask=True)
        assert isinstance(res, smm.DeviceCSRResult)
        Q = smm.pin_operand(res)
        assert isinstance(Q, smm.PinnedOperand) and Q.shape == (K, K) and Q.nnz == L_ref.nnz
        Z, info = smm.innovation_solve(Hp, Q, Rp, torch.from_numpy(D).to(dev))
        assert mo.cache_stats["upload"] == uploads, "L or Q went through an operand upload"
        assert not downloads, "an operand's arrays were copied to the host on the way"
        S = Q.to_scipy()
        assert np.array_equal(S.indptr, Q_ref.indptr) and np.array_equal(S.indices, Q_ref.indices)
        assert np.array_equal(_bits(S.data), _bits(Q_ref.data))
        assert np.array_equal(_bits(Z.cpu().numpy()), _bits(Z_ref))
        assert np.array_equal(info.iterations, info_ref.iterations) and np.array_equal(info.status, info_ref.status)
        assert np.array_equal(_bits(info.residual_sq), _bits(info_ref.residual_sq))
        assert np.array_equal(_bits(info.rhs_sq), _bits(info_ref.rhs_sq))
    finally:
        smm.set_exact(old_exact)
        smm.set_result_device(old_dev)
        for p in (Hp, Rp, L, Q):
            if p is not None:
                p.unpin()
