"""smm_cov_eval on the GPU against the numpy restatement of the contract (tests/cov_restatement.py): the spherical model
bit for bit, the models that call exp within ULPS = 8 ulp of the restated value -- 3 for the device's double exp (the
bound OpenCL sets, which the device library is built to meet), 0.5 for the restatement's own rounding of exp, one for each
of the at most four rounded operations after it.  The largest error seen per model is printed."""
import numpy as np
import pytest
import scipy.sparse as sp

from cov_restatement import (CV_RUN, MODELS, ULPS, entries, flat_pattern, named_patterns, points, restate, taper_pattern, ulps)
from sddmm_restatement import raw_csr

pytestmark = pytest.mark.gpu

WORST = {}                           # model -> the largest error seen, in ulp


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_close(got, want, model, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    err = ulps(got, want)
    worst = float(err.max()) if err.size else 0.0
    WORST[model] = max(WORST.get(model, 0.0), worst)
    bound = 0 if model == "spherical" else ULPS
    assert worst <= bound, f"{what}: {int((err > bound).sum())} of {err.size} values beyond {bound} ulp, the worst by {worst:.2f}"


# what is asked for: (value, wrt) with wrt None, "length" or "axis" (the last coordinate)
ASKS = ((True, None), (False, "axis"), (True, "length"), (True, "axis"))


def _check(ctx, h, M, a, b, model, dim, what, asks=ASKS, variance=2.5):
    """Every way of asking, scaled and unscaled, of one pattern (handle h of the scipy matrix M) against the restatement."""
    rows, cols, w = entries(M)
    for value, ask in asks:
        wrt = dim - 1 if ask == "axis" else ask
        length = 1.1 if ask == "length" else [0.9, 1.3, 2.1][:dim]
        for scale in (False, True):
            val, dval = ctx.cov_host(h, a, b, model, length, variance, wrt=wrt, scale=scale, value=value)
            want = restate(a, b, rows, cols, model, length, variance, wrt, w if scale else None)
            assert (val is None) == (not value) and (dval is None) == (wrt is None)
            for got, ref, part in ((val, want[0], "value"), (dval, want[1], "derivative")):
                if got is not None:
                    _assert_close(got, ref, model, f"{what} {model} wrt={wrt} scale={scale} {part}")


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("model", MODELS)
def test_taper_pattern_of_300_points(ctx, model, dim):
    L = taper_pattern(dim)
    h = ctx.csr_from_scipy(L)
    held = ctx.live_bytes()
    try:
        before, nbytes = h.to_host(), h.device_bytes()
        _check(ctx, h, L, points(300, dim), None, model, dim, f"taper dim {dim}")
        after = h.to_host()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and np.array_equal(_bits(before[2]), _bits(after[2]))
        assert h.device_bytes() == nbytes, "the call cached something for the pattern operand"
        assert ctx.live_bytes() == held, "a temporary of the call is still handed out"
    finally:
        h.close()


@pytest.mark.parametrize("model", MODELS)
def test_flat_split_at_its_small_boundaries(ctx, model):
    """1, 63, 64, 65 entries (a wave's step), one run of a wave +- 1 and the four runs of a workgroup +- 1, in 37 x 50 with
    empty rows, unsorted rows and repeated columns; then no entries at all."""
    a, b = points(37, 2, 1), points(50, 2, 2)
    for nnz in (1, 63, 64, 65, CV_RUN - 1, CV_RUN, CV_RUN + 1, 4 * CV_RUN - 1, 4 * CV_RUN, 4 * CV_RUN + 1):
        M = flat_pattern(nnz, 37, 50, 610 + nnz)
        h = ctx.csr_from_scipy(M)
        try:
            _check(ctx, h, M, a, b, model, 2, f"flat {nnz}", asks=ASKS[2:])
        finally:
            h.close()
    h = ctx.csr_from_scipy(sp.csr_matrix((37, 50)))
    try:
        val, dval = ctx.cov_host(h, a, b, model, 1.0, 2.5, wrt="length")
        assert val.shape == (0,) and dval.shape == (0,)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["arrow", "two_per_row", "unsorted_repeated", "rectangular"])
def test_named_patterns(ctx, name):
    M = named_patterns()[name]
    dim = 3 if name == "rectangular" else 2
    a, b = points(M.shape[0], dim, 3), points(M.shape[1], dim, 4)
    h = ctx.csr_from_scipy(M)
    try:
        for model in MODELS:
            _check(ctx, h, M, a, b, model, dim, name, asks=ASKS[3:])
    finally:
        h.close()


def test_every_wave_of_the_grid_takes_a_second_run(ctx):
    """run * groups +- 1 entries, groups = the waves of the largest grid the library launches (8 workgroups of 4 waves per
    compute unit): the last wave's run ends one short of its end, and the first wave comes round for one more entry."""
    import torch
    groups = torch.cuda.get_device_properties(ctx.device).multi_processor_count * 8 * 4
    full = CV_RUN * groups
    n, per_row = 4096, 64
    m = full // per_row + 1
    a, b = points(m, 2, 5), points(n, 2, 6)
    for nnz in (full - 1, full + 1):
        ptr = np.minimum(np.arange(m + 1, dtype=np.int64) * per_row, nnz)
        cols = (np.arange(nnz, dtype=np.int64) * 2654435761 % n).astype(np.int32)
        M = raw_csr(ptr, cols, np.ones(nnz), (m, n))
        rows, cols, _ = entries(M)
        h = ctx.csr_from_scipy(M)
        try:
            val, dval = ctx.cov_host(h, a, b, "exponential", 1.1, 2.5, wrt="length")
        finally:
            h.close()
        want = restate(a, b, rows, cols, "exponential", 1.1, 2.5, "length")
        _assert_close(val, want[0], "exponential", f"{nnz} entries, value")
        _assert_close(dval, want[1], "exponential", f"{nnz} entries, derivative")


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_column_slice_in_place_own_buffer_against_a_copy_and_two_calls(ctx, dim):
    """lda > dim: a column slice of a wider device tensor, used where it is; b as a's own buffer and b as an equal copy
    give the same bits; so do two calls."""
    import torch
    dev = torch.device("cuda", ctx.device)
    L = taper_pattern(dim)
    rows, cols, w = entries(L)
    host = np.full((300, 5), np.nan)
    host[:, 1:1 + dim] = points(300, dim)
    wide = torch.from_numpy(host).to(dev)
    pts = wide[:, 1:1 + dim]
    length = [0.9, 1.3, 2.1][:dim]
    h = ctx.csr_from_scipy(L)
    try:
        for model in ("spherical", "matern52"):
            want = restate(points(300, dim), None, rows, cols, model, length, 2.5, 0, w)
            out = [torch.full((L.nnz,), float("nan"), dtype=torch.float64, device=dev) for _ in range(6)]
            ctx.cov_into(h, pts, 5, pts, 5, dim, model, length, 2.5, out[0], out[1], wrt=0, scale=True)
            ctx.cov_into(h, pts, 5, pts.contiguous().clone(), dim, dim, model, length, 2.5, out[2], out[3], wrt=0, scale=True)
            ctx.cov_into(h, pts, 5, pts, 5, dim, model, length, 2.5, out[4], out[5], wrt=0, scale=True)
            got = [t.cpu().numpy() for t in out]
            _assert_close(got[0], want[0], model, f"slice {model} value")
            _assert_close(got[1], want[1], model, f"slice {model} derivative")
            for k in (2, 4):
                assert np.array_equal(_bits(got[k]), _bits(got[0])) and np.array_equal(_bits(got[k + 1]), _bits(got[1])), (model, k)
            assert np.all(np.isnan(wide.cpu().numpy()[:, 0])), "the coordinates were written"
    finally:
        h.close()


def test_nan_and_infinite_coordinates_reach_exactly_their_entries(ctx):
    M = named_patterns()["rectangular"]
    rows, cols, _ = entries(M)
    a, b = points(37, 3, 3), points(300, 3, 4)
    a[5, 1], b[17, 0], b[40, 2] = np.nan, np.inf, np.nan
    touched = (rows == 5) | (cols == 17) | (cols == 40)
    h = ctx.csr_from_scipy(M)
    try:
        for model in MODELS:
            val, dval = ctx.cov_host(h, a, b, model, 1.1, 2.5, wrt="length")
            want = restate(a, b, rows, cols, model, 1.1, 2.5, "length")
            assert np.all(np.isnan(val[(rows == 5) | (cols == 40)])), model
            assert np.array_equal(np.isnan(val), np.isnan(want[0])) and np.array_equal(np.isnan(dval), np.isnan(want[1])), model
            _assert_close(val[~touched], want[0][~touched], model, f"{model}: entries no bad point touches")
            _assert_close(dval[~touched], want[1][~touched], model, f"{model}: derivative at entries no bad point touches")
    finally:
        h.close()


def test_refusals_leave_the_context_usable(ctx):
    from sparse_matrix_mult_amd.engine import SmmError
    L = taper_pattern(2)
    p = points(300, 2)
    h = ctx.csr_from_scipy(L)
    held = ctx.live_bytes()
    try:
        bad = [dict(model=9), dict(length=0.0), dict(length=-1.0), dict(length=np.inf), dict(length=[1.0, np.nan]), dict(variance=np.inf),
               dict(variance=np.nan), dict(wrt=2), dict(wrt=-5), dict(length=[1.0, 2.0], wrt="length"), dict(value=False)]
        for kw in bad:
            args = dict(model="gaussian", length=1.0, variance=2.5)
            args.update(kw)
            with pytest.raises(SmmError) as e:
                ctx.cov_host(h, p, None, **args)
            assert e.value.code == -2, kw
            assert ctx.live_bytes() == held
        for a, b in ((p[:299], None), (p, p[:10]), (np.ones((300, 4)), None)):
            with pytest.raises(SmmError) as e:
                ctx.cov_host(h, a, b, "gaussian", 1.0)
            assert e.value.code == -2
        # the device entry: an output without its wrt and the reverse, no output, overlapping outputs, a leading dimension
        # below dim, missing coordinates
        import torch
        dev = torch.device("cuda", ctx.device)
        dp, o1, o2 = torch.from_numpy(p).to(dev), torch.empty(L.nnz + 8, dtype=torch.float64, device=dev), torch.empty(L.nnz, dtype=torch.float64, device=dev)
        for kw in (dict(d_val=o1, d_dval=None, wrt=0), dict(d_val=o1, d_dval=o2, wrt=None), dict(d_val=None, d_dval=None),
                   dict(d_val=o1, d_dval=o1[8:], wrt=0), dict(d_val=o1, lda=1), dict(d_val=o1, ldb=1), dict(d_val=o1, d_a=None),
                   dict(d_val=dp)):
            args = dict(d_a=dp, lda=2, d_b=dp, ldb=2, dim=2, model="gaussian", length=1.0, variance=2.5)
            args.update(kw)
            with pytest.raises(SmmError) as e:
                ctx.cov_into(h, **args)
            assert e.value.code == -2, kw
        ctx.cov_host(h, p, None, "gaussian", 1.0, variance=0.0)         # a variance of 0 is allowed
        _check(ctx, h, L, p, None, "gaussian", 2, "after the refusals", asks=ASKS[2:3])
    finally:
        h.close()


def test_a_failed_allocation_leaves_no_pool_block_handed_out():
    """smm_cov_eval_host (a and b different, both outputs: four pool blocks) made to fail at its 1st, 2nd, ... device
    allocation (hard) until it succeeds: each failure is SMM_ERR_ALLOC with nothing handed out, and the call that succeeds
    is right."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    M = named_patterns()["rectangular"]
    rows, cols, w = entries(M)
    a, b = points(37, 3, 3), points(300, 3, 4)
    want = restate(a, b, rows, cols, "spherical", 1.1, 2.5, 1, w)
    h = c.csr_from_scipy(M)
    try:
        c.cov_host(h, a, b, "spherical", 1.1, 2.5, wrt=1, scale=True)    # (the operand is validated: no first-use work is left)
        failures = 0
        for nth in range(1, 9):
            c.release_pool()
            live = c.live_bytes()
            c.inject_alloc_failure(nth, hard=True)
            try:
                got = c.cov_host(h, a, b, "spherical", 1.1, 2.5, wrt=1, scale=True)
            except SmmError as e:
                assert e.code == -3, f"allocation {nth}: {e}"
                assert c.live_bytes() == live, f"allocation {nth}: {c.live_bytes() - live} bytes still handed out"
                failures += 1
                continue
            finally:
                c.inject_alloc_failure(0)
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
            assert c.live_bytes() == live
            break
        else:
            pytest.fail("never succeeded")
        assert failures == 4, f"{failures} allocations failed, the call takes four pool blocks"
    finally:
        h.close()
        c.close()


def test_on_a_callers_stream():
    """A context that launches on a stream it does not own -- the device's null stream, which is torch's current stream, as
    bench.py runs the library: the coordinates are uploaded by torch on it just before the call and the outputs cloned by
    torch just after, with no wait on the host in between (DESIGN, "Streams": shared stream).  The null stream and not a new
    side stream: tests/test_gpu_caller_stream.py explains why a process of this suite should not open a fifth queue."""
    import torch
    from sparse_matrix_mult_amd.engine import Context
    dev = torch.device("cuda", 0)
    L = taper_pattern(2)
    rows, cols, w = entries(L)
    p = points(300, 2)
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    c = Context(0, 0)
    assert c.stream == 0
    h = c.csr_from_scipy(L)
    try:
        for model in ("spherical", "gaussian"):
            want = restate(p, None, rows, cols, model, 1.1, 2.5, "length", w)
            dp = torch.from_numpy(p).to(dev, non_blocking=True)
            out = [torch.full((L.nnz,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2)]
            c.cov_into(h, dp, 2, dp, 2, 2, model, 1.1, 2.5, out[0], out[1], wrt="length", scale=True)
            clones = [t.clone() for t in out]
            torch.cuda.synchronize()
            for t, ref, part in zip(clones, want, ("value", "derivative")):
                _assert_close(t.cpu().numpy(), ref, model, f"null stream {model} {part}")
            val, dval = c.cov_host(h, p, None, model, 1.1, 2.5, wrt="length", scale=True)
            assert np.array_equal(_bits(val), _bits(out[0].cpu().numpy())) and np.array_equal(_bits(dval), _bits(out[1].cpu().numpy()))
    finally:
        torch.cuda.synchronize()
        h.close()
        c.close()


# ------------------------------------------------------------------------------ the public function
def _arrays(M):
    assert sp.isspmatrix_csr(M) and M.indices.dtype == np.int32 and M.data.dtype == np.float64
    return M.indptr, M.indices, M.data


def test_public_function_delivers_by_the_existing_rules():
    """scipy in and out; a tensor in; a DeviceCSRResult under set_result_device(True); pinned results from a pinned
    pattern -- all the same arrays, and the pattern operand is left as it was."""
    import torch
    import sparse_matrix_mult_amd as smm
    from sparse_matrix_mult_amd.engine import default_context
    dev = torch.device("cuda", default_context().device)
    L = taper_pattern(2)
    rows, cols, w = entries(L)
    p = points(300, 2)
    want = restate(p, None, rows, cols, "matern32", 1.1, 2.5, "length", w)
    kw = dict(variance=2.5, scale_by_pattern=True, derivative="length")

    def same(pair, what):
        for M, ref in zip(pair, want):
            ptr, idx, data = _arrays(M)
            assert np.array_equal(ptr, L.indptr) and np.array_equal(idx, L.indices), what
            _assert_close(data, ref, "matern32", what)

    host = smm.covariance_on_pattern(L, p, "matern32", 1.1, **kw)
    same(host, "scipy in, scipy out")
    Q = smm.covariance_on_pattern(L, p, "matern32", 1.1, variance=2.5, scale_by_pattern=True)
    assert np.array_equal(_bits(_arrays(Q)[2]), _bits(host[0].data)), "the value alone"
    same(smm.covariance_on_pattern(L, torch.from_numpy(p).to(dev), "matern32", 1.1, **kw), "tensor in, scipy out")
    U = named_patterns()["unsorted_repeated"]
    ur, uc, _ = entries(U)
    got = smm.covariance_on_pattern(U, points(4, 2, 3), "spherical", 1.5, coords_b=points(10, 2, 4))
    assert np.array_equal(got.indptr, U.indptr) and np.array_equal(got.indices, U.indices), "the pattern as stored"
    _assert_close(got.data, restate(points(4, 2, 3), points(10, 2, 4), ur, uc, "spherical", 1.5)[0], "spherical", "unsorted, repeated")
    P = smm.pin_operand(L)
    old = smm.set_result_device(True)
    pinned = ()
    try:
        before, nbytes = P._handle.to_host(), P._handle.device_bytes()
        res = smm.covariance_on_pattern(P, p, "matern32", 1.1, **kw)
        assert all(isinstance(r, smm.DeviceCSRResult) and r.indptr.dtype == torch.int64 and r.data.is_cuda for r in res)
        assert res[0].indices.data_ptr() != res[1].indices.data_ptr()
        same([r.to_scipy() for r in res], "pinned pattern, device results")
        pinned = smm.covariance_on_pattern(P, torch.from_numpy(p).to(dev), "matern32", 1.1, pin=True, **kw)
        assert all(isinstance(r, smm.PinnedOperand) and r.shape == (300, 300) and r.nnz == L.nnz for r in pinned)
        same([r.to_scipy() for r in pinned], "pinned pattern, pinned results")
        after = P._handle.to_host()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and P._handle.device_bytes() == nbytes
    finally:
        smm.set_result_device(old)
        for r in (P,) + tuple(pinned):
            r.unpin()


def test_the_chain_from_coordinates_to_the_trace_term_stays_on_the_device(monkeypatch):
    """L pinned from coordinates, (Q, dQ) = L o C and L o dC/dlength pinned from the same coordinates, innovation_solve on Q
    and triple_product_apply on dQ, with no download of an operand's arrays on the way; z^T H dQ H^T z against the same
    expression formed densely in numpy from the downloaded matrices, within the bound tests/test_gpu_spmm.py holds
    triple_apply to in default mode (rtol 1e-9, atol 1e-12)."""
    import torch
    import sparse_matrix_mult_amd as smm
    from sparse_matrix_mult_amd.engine import DeviceCSR, default_context
    rng = np.random.default_rng(800)
    K, n, k, cutoff, ell, s2 = 200, 80, 3, 0.3, 0.15, 2.5
    xy = rng.random((K, 2))
    cols = np.stack([rng.choice(K, 3, replace=False) for _ in range(n)])
    H = sp.csr_matrix((rng.uniform(0.5, 1.5, 3 * n), cols.ravel().astype(np.int32), np.arange(0, 3 * n + 1, 3, dtype=np.int32)), shape=(n, K))
    R = sp.diags(rng.uniform(1.0, 2.0, n)).tocsr()
    D = rng.standard_normal((n, k))
    dev = torch.device("cuda", default_context().device)
    old = smm.set_result_device(True)
    made = []
    try:
        Hp, Rp = smm.pin_operand(H), smm.pin_operand(R)
        made += [Hp, Rp]
        downloads = []
        to_host = DeviceCSR.to_host
        monkeypatch.setattr(DeviceCSR, "to_host", lambda self: downloads.append(self) or to_host(self))
        dxy = torch.from_numpy(xy).to(dev)
        L = smm.localization_taper(dxy, cutoff, pin=True)
        made.append(L)
        Q, dQ = smm.covariance_on_pattern(L, dxy, "exponential", ell, s2, scale_by_pattern=True, derivative="length", pin=True)
        made += [Q, dQ]
        assert isinstance(Q, smm.PinnedOperand) and isinstance(dQ, smm.PinnedOperand) and Q.nnz == dQ.nnz == L.nnz
        Z, info = smm.innovation_solve(Hp, Q, Rp, torch.from_numpy(D).to(dev))
        Y = smm.triple_product_apply(Hp, dQ, Z)
        assert not downloads, "an operand's arrays were copied to the host on the way"
        assert info.converged and torch.is_tensor(Y)
        monkeypatch.undo()
        Z, Y = Z.cpu().numpy(), Y.cpu().numpy()
        Ld, Qd, dQd, Hd = L.to_scipy().toarray(), Q.to_scipy().toarray(), dQ.to_scipy().toarray(), H.toarray()
        got = np.einsum("ij,ij->j", Z, Y)
        want = np.einsum("ij,ij->j", Z, Hd @ (dQd @ (Hd.T @ Z)))
        print("z^T H dQ H^T z", got, "dense", want)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12)
        # and Q, dQ are what the contract says of these coordinates on L's pattern
        S = L.to_scipy()
        rows, cols_, w = entries(S)
        ref = restate(xy, None, rows, cols_, "exponential", ell, s2, "length", w)
        _assert_close(Q.to_scipy().data, ref[0], "exponential", "Q of the chain")
        _assert_close(dQ.to_scipy().data, ref[1], "exponential", "dQ of the chain")
        res = np.linalg.norm((Hd @ Qd @ Hd.T + R.toarray()) @ Z - D, axis=0) / np.linalg.norm(D, axis=0)
        assert np.all(res <= 1e-6) and Ld.shape == (K, K), res
    finally:
        smm.set_result_device(old)
        for p in made:
            p.unpin()


def test_report_the_largest_error_seen():
    """(not a check of the library: prints what DESIGN quotes; it follows the cases it reports)"""
    for model in MODELS:
        if model in WORST:
            print(f"largest error seen, {model}: {WORST[model]:.2f} ulp")
