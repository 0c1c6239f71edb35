"""smm_variogram on the GPU against the numpy restatement of the contract (tests/variogram_restatement.py): count, sum_lag and
sum_sq bit for bit on every shape -- there is one summation order, fixed by the header's SMM_VG_SLOTS and SMM_VG_RUN.  Where a
sum is NaN (a NaN value reached it) the NaN's sign and payload are not compared: IEEE 754 leaves them open."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from sddmm_restatement import raw_csr
from variogram_restatement import RUN, T, bits, edges_of, entries, flat_pattern, per_entry, points, restate, taper_pattern, values

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    """(count, sum_h, sum_sq) against the restatement: the same bits; a NaN sum against a NaN sum."""
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[2].dtype == np.float64, what
    assert np.array_equal(got[0], want[0]), f"{what}: count {got[0].tolist()} != {want[0].tolist()}"
    for g, w, part in ((got[1], want[1], "sum_lag"), (got[2], want[2], "sum_sq")):
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), f"{what}: {part} is NaN in other bins"
        diff = np.flatnonzero(bits(g)[~nan] != bits(w)[~nan])
        assert diff.size == 0, f"{what}: {part} differs in {diff.size} of {g.size} bins, the first got {g[~nan][diff[0]]!r} want {w[~nan][diff[0]]!r}"


@functools.lru_cache(maxsize=None)
def _taper_want(dim, k, nb, upper):
    rows, cols, _ = entries(taper_pattern(dim))
    return restate(points(300, dim), values(300, k), rows, cols, edges_of(nb), upper)


def test_taper_pattern_of_300_points(ctx):
    for dim in (1, 2, 3):
        _taper_case(ctx, dim)


def _taper_case(ctx, dim):
    L = taper_pattern(dim)
    h = ctx.csr_from_scipy(L)
    held = ctx.live_bytes()
    try:
        before, nbytes = h.to_host(), h.device_bytes()
        for k in (1, 3):
            for nb in (1, 7, 32):
                for upper in (True, False):
                    got = ctx.variogram_host(h, points(300, dim), values(300, k), edges_of(nb), upper)
                    _same(got, _taper_want(dim, k, nb, upper), f"taper dim {dim} k {k} nb {nb} upper {upper}")
                    assert got[0].sum() > 0
        after = h.to_host()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and np.array_equal(bits(before[2]), bits(after[2]))
        assert h.device_bytes() == nbytes, "the call cached something for the pattern operand"
        assert ctx.live_bytes() == held, "a temporary of the call is still handed out"
    finally:
        h.close()


def test_flat_split_at_its_small_boundaries(ctx):
    """1, 63, 64, 65 entries (a wave's step), one run +- 1 and the four runs of a 256-lane workgroup +- 1, in 50 x 50 with
    empty rows, unsorted rows and repeated columns; then no entries at all."""
    p, v, e = points(50, 2, 1), values(50, 3, 1), edges_of(7, 3.6)
    for nnz in (1, 63, 64, 65, RUN - 1, RUN, RUN + 1, 4 * RUN - 1, 4 * RUN, 4 * RUN + 1):
        M = flat_pattern(nnz, 50, 50, 910 + nnz)
        rows, cols, _ = entries(M)
        h = ctx.csr_from_scipy(M)
        try:
            for upper in (False, True):
                _same(ctx.variogram_host(h, p, v, e, upper), restate(p, v, rows, cols, e, upper), f"flat {nnz} upper {upper}")
        finally:
            h.close()
    h = ctx.csr_from_scipy(sp.csr_matrix((50, 50)))
    try:
        count, sum_h, sum_sq = ctx.variogram_host(h, p, v, e, False)
        assert count.tolist() == [0] * 7 and np.array_equal(bits(sum_h), bits(np.zeros(7))) and np.array_equal(bits(sum_sq), bits(np.zeros(7)))
    finally:
        h.close()


def test_the_round_robin_comes_round(ctx):
    """4 T - 1, 4 T + 1 and 8 T + 1 entries: every wave of the grid has taken its fourth (eighth) run and the last is one
    entry short, or the first wave comes round for one entry more.  64 entries per row and the columns of test_every_wave_of_the_grid_takes_a_second_run over 4096
    points; the pattern is square, so it has as many rows as 64 per row need (n >= 4096)."""
    for nnz in (4 * T - 1, 4 * T + 1, 8 * T + 1):
        _round_robin_case(ctx, nnz)


def _round_robin_case(ctx, nnz):
    per_row, ncol = 64, 4096
    n = max(nnz // per_row + 1, ncol)
    ptr = np.minimum(np.arange(n + 1, dtype=np.int64) * per_row, nnz)
    cols = (np.arange(nnz, dtype=np.int64) * 2654435761 % ncol).astype(np.int32)
    M = raw_csr(ptr, cols, np.ones(nnz), (n, n))
    rows, cols, _ = entries(M)
    p, v, e = points(n, 2, 5), values(n, 1, 5), edges_of(15, 3.6)
    h = ctx.csr_from_scipy(M)
    try:
        got = ctx.variogram_host(h, p, v, e, False)
    finally:
        h.close()
    assert got[0].sum() == nnz
    _same(got, restate(p, v, rows, cols, e, False), f"{nnz} entries")


def test_bin_edges_met_exactly(ctx):
    """Integer coordinates on a line, every pair stored: h is an exact integer.  h = 1 lands in the bin that starts at 1,
    h = edges[nb] is left out, and coincident points count in bin 0 only where edges[0] = 0 -- once for i < j, and both ways
    beside the diagonal with upper=False."""
    x = np.array([0.0, 1.0, 2.0, 3.0, 1.0, 0.0, 5.0])
    n = x.size
    M = sp.csr_matrix(np.ones((n, n)))
    rows, cols, _ = entries(M)
    hh = np.abs(x[rows] - x[cols]).astype(np.int64)
    h = ctx.csr_from_scipy(M)
    try:
        for e in ([0.0, 1.0, 2.0, 3.0], [1.0, 2.0]):
            for upper in (True, False):
                take = (cols > rows) if upper else np.ones(rows.size, dtype=bool)
                count = [int((take & (hh == int(lo))).sum()) for lo in e[:-1]]        # unit bins: the integers
                got = ctx.variogram_host(h, x, x * x, e, upper)
                assert got[0].tolist() == count, (e, upper)
                assert got[1].tolist() == [c * lo for c, lo in zip(count, e[:-1])]
                _same(got, restate(x, x * x, rows, cols, e, upper), f"edges {e} upper {upper}")
        assert ctx.variogram_host(h, x, x, [0.0, 1.0], True)[0].tolist() == [2]      # the pairs (0, 5) and (1, 4)
        assert ctx.variogram_host(h, x, x, [0.0, 1.0], False)[0].tolist() == [n + 4]
        assert ctx.variogram_host(h, x, x, [0.5, 1.0], False)[0].tolist() == [0]
    finally:
        h.close()


def test_everything_in_one_bin_and_nothing_in_any_bin():
    import sparse_matrix_mult_amd as smm
    L = taper_pattern(2)
    rows, cols, _ = entries(L)
    p, v = points(300, 2), values(300, 3)
    res = smm.empirical_variogram(L, p, v, [0.0, 100.0])
    assert isinstance(res, smm.VariogramResult) and res.count.tolist() == [(L.nnz - 300) // 2]
    _same((res.count, res.sum_lag, res.sum_sq), restate(p, v, rows, cols, [0.0, 100.0], True), "one bin")
    assert res.lag[0] == res.sum_lag[0] / res.count[0] and res.gamma[0] == res.sum_sq[0] / (2.0 * 3 * res.count[0])
    res = smm.empirical_variogram(L, p, v, [50.0, 55.0, 60.0], upper=False)
    assert res.count.tolist() == [0, 0]
    assert np.array_equal(bits(res.sum_lag), bits(np.zeros(2))) and np.array_equal(bits(res.sum_sq), bits(np.zeros(2)))
    assert np.all(np.isnan(res.gamma)) and np.all(np.isnan(res.lag))


def test_special_values_reach_exactly_their_bins(ctx):
    L = taper_pattern(2)
    rows, cols, _ = entries(L)
    p, e, bad = points(300, 2), edges_of(32), 17
    h = ctx.csr_from_scipy(L)
    try:
        clean = ctx.variogram_host(h, p, values(300, 3), e, True)
        v = values(300, 3).copy()
        v[bad, 0], v[bad, 2] = np.nan, np.inf
        got = ctx.variogram_host(h, p, v, e, True)
        _, _, b, take = per_entry(p, v, rows, cols, e, True)
        touched = np.zeros(32, dtype=bool)
        touched[b[take & ((rows == bad) | (cols == bad))]] = True
        assert 0 < touched.sum() < 32
        assert np.array_equal(~np.isfinite(got[2]), touched), "sum_sq is not finite in other bins than those of the point's pairs"
        assert np.array_equal(got[0], clean[0]) and np.array_equal(bits(got[1]), bits(clean[1]))
        assert np.array_equal(bits(got[2][~touched]), bits(clean[2][~touched]))
        _same(got, restate(p, v, rows, cols, e, True), "NaN and inf in the values")
        q = p.copy()
        q[bad, 1] = np.nan                                           # its pairs leave all three outputs
        got = ctx.variogram_host(h, q, values(300, 3), e, True)
        mine = take & ((rows == bad) | (cols == bad))
        assert np.array_equal(got[0], clean[0] - np.bincount(b[mine], minlength=32)) and got[0].sum() < clean[0].sum()
        assert np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2]))
        _same(got, restate(q, values(300, 3), rows, cols, e, True), "a NaN coordinate")
    finally:
        h.close()


def test_column_slices_in_place_numpy_and_a_side_stream(ctx):
    """In dimension 1, 2 and 3.  lda > dim and ldy > k: column slices of wider device tensors, used where they are, through the engine and through the
    public function; numpy inputs; and the public call under a side stream right after the tensors were produced on it (the
    wrapper waits for torch's current stream; this module runs after tests/test_gpu_caller_stream.py, whose races a further
    queue could hide)."""
    for dim in (1, 2, 3):
        _layout_case(ctx, dim)


def _layout_case(ctx, dim):
    import torch
    import sparse_matrix_mult_amd as smm
    dev = torch.device("cuda", ctx.device)
    L = taper_pattern(dim)
    p, v, e = points(300, dim), values(300, 3), edges_of(7)
    want = _taper_want(dim, 3, 7, True)
    host_p, host_v = np.full((300, 5), np.nan), np.full((300, 6), np.nan)
    host_p[:, 1:1 + dim], host_v[:, 2:5] = p, v
    wide_p, wide_v = torch.from_numpy(host_p).to(dev), torch.from_numpy(host_v).to(dev)
    h = ctx.csr_from_scipy(L)
    try:
        _same(ctx.variogram_device(h, wide_p[:, 1:1 + dim], 5, dim, wide_v[:, 2:5], 6, 3, e, True), want, "engine, slices")
        _same(ctx.variogram_device(h, wide_p[:, 1:1 + dim].data_ptr(), 5, dim, wide_v[:, 2:5].data_ptr(), 6, 3, e, True), want, "addresses")
    finally:
        h.close()

    def public(*args):
        r = smm.empirical_variogram(L, *args, e)
        assert all(isinstance(x, np.ndarray) for x in (r.edges, r.count, r.sum_lag, r.sum_sq, r.lag, r.gamma))
        return r.count, r.sum_lag, r.sum_sq

    _same(public(p, v), want, "numpy")
    _same(public(wide_p[:, 1:1 + dim], wide_v[:, 2:5]), want, "public, slices")
    _same(public(wide_p[:, 1:1 + dim], v.copy()), want, "tensor coordinates, numpy values")
    _same(public(p if dim > 1 else p[:, 0], wide_v[:, 2:5]), want, "numpy coordinates, tensor values")
    P = smm.pin_operand(L)
    try:
        r = smm.empirical_variogram(P, wide_p[:, 1:1 + dim], wide_v[:, 2:5], e)
        _same((r.count, r.sum_lag, r.sum_sq), want, "pinned pattern")
    finally:
        P.unpin()
    if dim == 2:
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            tp = torch.from_numpy(host_p).to(dev, non_blocking=True).mul_(1.0)
            tv = torch.from_numpy(host_v).to(dev, non_blocking=True).mul_(1.0)
            got = public(tp[:, 1:1 + dim], tv[:, 2:5])
        side.synchronize()
        _same(got, want, "under a side stream")
    assert np.all(np.isnan(wide_p.cpu().numpy()[:, 0])) and np.all(np.isnan(wide_v.cpu().numpy()[:, :2])), "an input was written"


def test_refusals_leave_the_context_usable(ctx):
    from sparse_matrix_mult_amd.engine import SmmError
    L = taper_pattern(2)
    p, v, e = points(300, 2), values(300, 3), edges_of(7)
    h = ctx.csr_from_scipy(L)
    r = ctx.csr_from_scipy(sp.csr_matrix(np.ones((300, 4))))
    held = ctx.live_bytes()
    try:
        bad = [dict(edges=[0.0]), dict(edges=np.arange(34.0)), dict(edges=[0.0, np.inf]), dict(edges=[0.0, np.nan, 1.0]), dict(edges=[-1.0, 1.0]),
               dict(edges=[0.0, 1.0, 1.0]), dict(edges=[1.0, 0.5]), dict(a=np.ones((300, 4))), dict(pattern=r)]
        for kw in bad:
            args = dict(pattern=h, a=p, y=v, edges=e)
            args.update(kw)
            with pytest.raises(SmmError) as err:
                ctx.variogram_host(**args)
            assert err.value.code == -2, kw
            assert ctx.live_bytes() == held
        import torch
        dev = torch.device("cuda", ctx.device)
        dp, dv = torch.from_numpy(p).to(dev), torch.from_numpy(v.copy()).to(dev)
        for kw in (dict(lda=1), dict(ldy=2), dict(k=-1), dict(dim=0), dict(dim=4), dict(d_a=None), dict(d_y=None)):
            args = dict(pattern=h, d_a=dp, lda=2, dim=2, d_y=dv, ldy=3, k=3, edges=e)
            args.update(kw)
            with pytest.raises(SmmError) as err:
                ctx.variogram_device(**args)
            assert err.value.code == -2, kw
        rc = ctx.lib.smm_variogram_host(ctx.handle, h.handle, 4, 2, p.ctypes.data, 2, 3, v.ctypes.data, 3, 1, np.array([0.0, 1.0]).ctypes.data,
                                        np.zeros(1, dtype=np.int64).ctypes.data, np.zeros(1).ctypes.data, np.zeros(1).ctypes.data)
        assert rc == -2, "SMM_EXACT is no flag of this call"
        _same(ctx.variogram_host(h, p, v, e), _taper_want(2, 3, 7, True), "after the refusals")
        _same(ctx.variogram_device(h, dp, 2, 2, dv, 3, 0, e), restate(p, np.zeros((300, 0)), *entries(L)[:2], e), "k = 0")
    finally:
        h.close()
        r.close()


def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_variogram_host takes four pool blocks (coordinates, values, sums, counts): made to fail at its 1st, 2nd, ... device
    allocation (hard) until it succeeds, each failure is SMM_ERR_ALLOC with nothing handed out, and the call that succeeds is
    right."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    L = taper_pattern(3)
    p, v, e = points(300, 3), values(300, 3), edges_of(7)
    h = c.csr_from_scipy(L)
    try:
        c.variogram_host(h, p, v, e)                               # (the operand is validated: no first-use work is left)
        failures = 0
        for nth in range(1, 9):
            c.release_pool()
            live = c.live_bytes()
            c.inject_alloc_failure(nth, hard=True)
            try:
                got = c.variogram_host(h, p, v, e)
            except SmmError as err:
                assert err.code == -3, f"allocation {nth}: {err}"
                assert c.live_bytes() == live, f"allocation {nth}: {c.live_bytes() - live} bytes still handed out"
                failures += 1
                continue
            finally:
                c.inject_alloc_failure(0)
            _same(got, _taper_want(3, 3, 7, True), "after the failures")
            assert c.live_bytes() == live
            break
        else:
            pytest.fail("never succeeded")
        assert failures == 4, f"{failures} allocations failed, the call takes four pool blocks"
    finally:
        h.close()
        c.close()


def test_two_calls_and_unrelated_tuning_give_the_same_bits(ctx):
    L = taper_pattern(3)
    p, v, e = points(300, 3), values(300, 3), edges_of(32)
    h = ctx.csr_from_scipy(L)
    try:
        first = ctx.variogram_host(h, p, v, e, False)
        _same(ctx.variogram_host(h, p, v, e, False), first, "second call")
        ctx.tune_sddmm(2)
        ctx.tune_spmm(1)
        ctx.tune_masked(2)
        try:
            _same(ctx.variogram_host(h, p, v, e, False), first, "after tuning other features")
        finally:
            ctx.tune_sddmm(0)
            ctx.tune_spmm(0)
            ctx.tune_masked(0)
        _same(first, _taper_want(3, 3, 32, False), "against the restatement")
    finally:
        h.close()
