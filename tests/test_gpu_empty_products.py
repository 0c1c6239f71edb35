"""Products that are structurally empty although both operands hold entries (tests/empty_products.py), through every
path: the CSR product under the seven dispatch configurations, dense, dense triple (chunk and ring), the CSR mirror, the
sparse and the masked triple, the masked product, H (Q (H^T X)), the innovation solve and log-determinant, the public
entry points and the legacy symbols.  tests/test_empty_products_cpu.py shows that the cases are what they claim.

Every expectation is exact: an empty pattern, a row pointer of zeros, +0.0 BY BIT PATTERN (view(int64) == 0, so that -0.0
and a sentinel left in place both fail), the sentinel untouched wherever nothing is to be written.  The one value with a
tolerance is lower_plus_one's single entry in default mode (helpers.RTOL, relative to the magnitude of its one term).

The zero tests that were there before all use an operand with nnz == 0 and return from matrix_ops.py before a plan or a
kernel is involved; here every row walks its products (strictly_lower under symmetric=True: products in every class of
the dispatch, not one output entry) or has none to walk although its entries of A name rows of B (missed_rows)."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import empty_products as ep
import special_values as sv
from empty_products import abs_arrays, arrays
from helpers import RTOL, upper_mask
from test_gpu_api import DArray, SparseMat, _from_sparsemat, _to_sparsemat, legacy  # noqa: F401  (legacy: the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SLACK = 16                                     # sentinel elements behind every buffer the library writes
NAN_BITS = 0x7FF8DEADBEEF0001                  # a quiet NaN with a payload of its own
PTR_SENTINEL = -0x0123456789ABCDEF
IDX_SENTINEL = -0x01234567
ZERO_LINE = "Multiplication resulted in a zero matrix."


@pytest.fixture(params=list(sv.HASH_CONFIGS))
def numeric_paths(request, ctx):
    """The seven dispatch configurations of tests/test_gpu_parity.py (the recipe of tests/test_gpu_special_values.py)."""
    hash_cfg, slab_cfg = {"hash+tiles": ((256, 2048), (0, 0, 4)), "tiles-only": ((0, 0), (0, 0, 4)),
                          "small-hash": ((24, 150), (0, 0, 4)), "slab-all": ((0, 0), (2, 0, 4)),
                          "slab-narrow": ((24, 150), (2, 50, 2)), "idx32": ((24, 150), (0, 0, 4)),
                          "dense-runs": ((0, 0), (0, 0, 4))}[request.param]
    assert hash_cfg == sv.HASH_CONFIGS[request.param]
    ctx.tune_hash(*hash_cfg)
    ctx.tune_slab(*slab_cfg)
    ctx.tune_narrow(request.param != "idx32")
    ctx.tune_dense_runs(2 if request.param == "dense-runs" else 1)
    yield request.param
    ctx.tune_hash(256, 2048)
    ctx.tune_slab(0, 0, 4)
    ctx.tune_narrow(True)
    ctx.tune_dense_runs(1)


@pytest.fixture(params=[False, True], ids=["chunk", "ring"])
def stage2(request, ctx):
    ctx.tune_stage2(request.param)
    yield request.param
    ctx.tune_stage2(False)


@pytest.fixture(params=[0, 1, 2], ids=["masked-auto", "masked-dot", "masked-row"])
def masked_mode(request, ctx):
    ctx.tune_masked(request.param)
    yield request.param
    ctx.tune_masked(0)


@pytest.fixture(params=[0, 8], ids=["block-default", "block-tiny"])
def block_budget(request, ctx):
    ctx.tune_triple_sparse(request.param)
    yield request.param
    ctx.tune_triple_sparse(0)


# ------------------------------------------------------------------------------ sentinels
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _all_plus_zero(x, what):
    b = _bits(x)
    assert not b.any(), f"{what}: {int(np.count_nonzero(b))} of {b.size} elements are not +0.0, first at {int(np.flatnonzero(b.ravel())[0])}"


def _nan_tensor(ctx, n):
    """n float64 on the device, every one the sentinel NaN."""
    import torch
    return torch.full((n,), NAN_BITS, dtype=torch.int64, device=torch.device("cuda", ctx.device)).view(torch.float64)


def _nan_array(shape, dtype=np.float64):
    return np.full(int(np.prod(shape)), NAN_BITS, dtype=np.uint64).view(np.float64).reshape(shape)


def _sentinel_kept(t, start, what):
    """The elements of the float64 tensor t from `start` on still hold the sentinel."""
    import torch
    tail = t.view(torch.int64)[start:].cpu().numpy()
    assert np.all(tail == np.int64(NAN_BITS)), f"{what}: the sentinel behind the output was overwritten at {np.flatnonzero(tail != np.int64(NAN_BITS))[:4]}"


def _settle(ctx):
    """Torch's stream has filled the buffers before the library (on the context's own stream) writes them."""
    import torch
    torch.cuda.synchronize(ctx.device)


# ------------------------------------------------------------------------------ CSR x CSR -> CSR
def _csr_cases():
    """name -> (A, B, symmetric)."""
    out = {}
    for v in ep.MISSED_VARIANTS:
        A, B, _ = ep.missed_rows(v)
        out[f"missed_rows-{v}"] = (A, B, False)
        out[f"missed_rows-{v}-sym"] = (A, B, True)
    A, B = ep.strictly_lower()
    out["strictly_lower-sym"] = (A, B, True)
    out["strictly_lower-control"] = (A, B, False)
    for v in ep.PLUS_ONE_VARIANTS:
        A, B, _ = ep.lower_plus_one(v)
        out[f"lower_plus_one-{v}"] = (A, B, True)
    for v in ep.VECTOR_VARIANTS:
        A, B = ep.vectors(v)
        out[f"vectors-{v}"] = (A, B, False)
        out[f"vectors-{v}-sym"] = (A, B, True)
    return out


CSR_CASES = _csr_cases()
EXPECTED_NNZ = {name: (None if name == "strictly_lower-control" else int(name.startswith("lower_plus_one"))) for name in CSR_CASES}


@functools.lru_cache(maxsize=None)
def _want(name):
    """((indptr, indices, data) of the oracle, the magnitude of every entry's terms): computed once, read only."""
    from oracle import oracle
    A, B, symmetric = CSR_CASES[name]
    want = oracle.sparse(arrays(A), arrays(B), B.shape[1], symmetric=symmetric)
    mag = oracle.sparse(abs_arrays(A), abs_arrays(B), B.shape[1], symmetric=symmetric)[2]
    for x in want + (mag,):
        x.setflags(write=False)
    if EXPECTED_NNZ[name] is not None:
        assert len(want[1]) == EXPECTED_NNZ[name]
    return want, mag


def _check_values(got, want, mag, exact, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    if exact:
        assert np.array_equal(_bits(got), _bits(want)), f"{what}: values differ bitwise"
    else:
        assert np.all(np.abs(got - want) <= RTOL * mag), f"{what}: worst {np.max(np.abs(got - want) - RTOL * mag):.3e} beyond the bound"


def _check_numeric_into(ctx, plan, want, mag, exact, what):
    """The device entry on sentinel-filled buffers with SLACK elements behind each array: the row pointer is written in
    full, the nnz indices and values are the oracle's, and nothing else is touched."""
    import torch
    wp, wi, wv = want
    m, nnz = len(wp) - 1, len(wi)
    dev = torch.device("cuda", ctx.device)
    ptr = torch.full((m + 1 + SLACK,), PTR_SENTINEL, dtype=torch.int64, device=dev)
    idx = torch.full((nnz + SLACK,), IDX_SENTINEL, dtype=torch.int32, device=dev)
    val = _nan_tensor(ctx, nnz + SLACK)
    _settle(ctx)
    plan.numeric_into(ptr.data_ptr(), idx.data_ptr(), val.data_ptr())
    ctx.synchronize()
    p, i = ptr.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(p[:m + 1], wp), f"{what}: indptr"
    assert np.all(p[m + 1:] == PTR_SENTINEL), f"{what}: written behind the row pointer"
    assert np.array_equal(i[:nnz], wi), f"{what}: indices"
    assert np.all(i[nnz:] == IDX_SENTINEL), f"{what}: written behind the {nnz} indices: {i[nnz:]}"
    _sentinel_kept(val, nnz, f"{what}: values")
    _check_values(val[:nnz].cpu().numpy(), wv, mag, exact, what)
    if nnz == 0:                                           # what a caller with empty tensors passes: no arrays at all
        ptr.fill_(PTR_SENTINEL)
        _settle(ctx)
        plan.numeric_into(ptr.data_ptr(), 0, 0)
        ctx.synchronize()
        p = ptr.cpu().numpy()
        assert not p[:m + 1].any() and np.all(p[m + 1:] == PTR_SENTINEL), f"{what}: indptr with NULL index and value arrays"


@pytest.mark.parametrize("name", list(CSR_CASES))
def test_csr_product(ctx, numeric_paths, name):
    A, B, symmetric = CSR_CASES[name]
    want, mag = _want(name)
    wp, wi, wv = want
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        assert a.nnz > 0 and b.nnz > 0
        for exact in (False, True):
            what = f"{name} {numeric_paths} exact={exact}"
            plan = ctx.spgemm_plan(a, b, symmetric=symmetric, exact=exact)
            try:
                assert plan.nnz == len(wi), f"{what}: the plan's nnz"
                assert np.array_equal(plan.indptr_host(), wp), f"{what}: the plan's row pointer"
                gp, gi, gv = plan.numeric_host()
                assert gp.dtype == np.int64 and gp.shape == (A.shape[0] + 1,) and np.array_equal(gp, wp), f"{what}: indptr"
                assert gi.dtype == np.int32 and np.array_equal(gi, wi), f"{what}: indices"
                _check_values(gv, wv, mag, exact, what)
                _check_numeric_into(ctx, plan, want, mag, exact, what)
            finally:
                plan.close()
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("name", ["strictly_lower-sym", "strictly_lower-control", "lower_plus_one-last_row", "lower_plus_one-highest_class"])
def test_row_shards_concatenate_to_the_whole(ctx, numeric_paths, name):
    """The shards of ep.SHARDS, each with its row_offset: the middle one holds product-bearing rows only, which -- with
    symmetric -- store nothing (lower_plus_one-highest_class: but for its first row's diagonal entry)."""
    A, B, symmetric = CSR_CASES[name]
    (wp, wi, wv), mag = _want(name)
    prod = ep.row_products(A, B)
    b = ctx.csr_from_scipy(B)
    try:
        for exact in (False, True):
            ptrs, idxs, vals, base = [np.zeros(1, np.int64)], [], [], 0
            for s, (r0, r1) in enumerate(ep.SHARDS):
                a = ctx.csr_from_scipy(A[r0:r1])
                try:
                    p, i, v = ctx.spgemm_host(a, b, symmetric=symmetric, row_offset=r0, exact=exact)
                finally:
                    a.close()
                if s == ep.BEARING_SHARD:
                    assert np.all(prod[r0:r1] > 0)
                    if name == "strictly_lower-sym":
                        assert not p.any() and len(i) == 0 and len(v) == 0, f"{name} exact={exact}: the shard of output-free rows"
                assert p.dtype == np.int64 and len(p) == r1 - r0 + 1
                ptrs.append(p[1:] + base); base += p[-1]; idxs.append(i); vals.append(v)
            assert np.array_equal(np.concatenate(ptrs), wp) and np.array_equal(np.concatenate(idxs), wi), f"{name} exact={exact}"
            _check_values(np.concatenate(vals), wv, mag, exact, f"{name} shards exact={exact}")
    finally:
        b.close()


# ------------------------------------------------------------------------------ CSR x CSR -> dense
def _dense_cases():
    """name -> (A, B, symmetric, mirror, row0, row1, (r, r) of the one entry or None)."""
    out = {}
    for v in ep.MISSED_VARIANTS:
        A, B, _ = ep.missed_rows(v)
        out[f"missed_rows-{v}"] = (A, B, False, False, 0, 300, None)
        out[f"missed_rows-{v}-sym"] = (A, B, True, False, 0, 300, None)
        out[f"missed_rows-{v}-mirror"] = (A, B, True, True, 0, 300, None)
    A, B, _ = ep.missed_rows()
    out["missed_rows-rows-37-150"] = (A, B, False, False, 37, 150, None)
    A, B = ep.strictly_lower()
    r0, r1 = ep.SHARDS[ep.BEARING_SHARD]
    out["strictly_lower-sym"] = (A, B, True, False, 0, ep.N_LOWER, None)
    out["strictly_lower-mirror"] = (A, B, True, True, 0, ep.N_LOWER, None)
    out["strictly_lower-sym-bearing-shard"] = (A, B, True, False, r0, r1, None)
    for v in ep.PLUS_ONE_VARIANTS:
        A, B, r = ep.lower_plus_one(v)
        out[f"lower_plus_one-{v}-sym"] = (A, B, True, False, 0, ep.N_LOWER, r)
        out[f"lower_plus_one-{v}-mirror"] = (A, B, True, True, 0, ep.N_LOWER, r)
    for v in ep.VECTOR_VARIANTS:
        A, B = ep.vectors(v)
        out[f"vectors-{v}"] = (A, B, False, False, 0, A.shape[0], None)
        out[f"vectors-{v}-mirror"] = (A, B, True, True, 0, A.shape[0], None)
    return out


DENSE_CASES = _dense_cases()


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_product_is_plus_zero_over_a_nan_sentinel(ctx, numeric_paths, name):
    A, B, symmetric, mirror, r0, r1, one = DENSE_CASES[name]
    m, n = r1 - r0, B.shape[1]
    a, b = ctx.csr_from_scipy(A[r0:r1] if (r0, r1) != (0, A.shape[0]) else A), ctx.csr_from_scipy(B)
    try:
        for exact in (False, True):
            what = f"{name} {numeric_paths} exact={exact}"
            out = _nan_tensor(ctx, m * n + SLACK)
            _settle(ctx)
            ctx.dense_into(a, b, out.data_ptr(), symmetric=symmetric, row_offset=r0, exact=exact, mirror=mirror)
            ctx.synchronize()
            _sentinel_kept(out, m * n, what)
            got = out[:m * n].cpu().numpy().reshape(m, n)
            if one is not None:
                want = float(A[one, one]) * float(B[one, one])
                assert want != 0 and abs(got[one - r0, one]) > 0
                _check_values(got[one - r0, one:one + 1], np.array([want]), np.array([abs(want)]), exact, what)
                got[one - r0, one] = 0.0
            _all_plus_zero(got, what)
    finally:
        a.close(); b.close()


def test_dense_host_entry(ctx):
    """The host entry (its own staging buffer) once per kind of case."""
    for name in ("missed_rows-unsorted-mirror", "strictly_lower-sym", "vectors-inner", "vectors-outer-mirror"):
        A, B, symmetric, mirror, _, _, _ = DENSE_CASES[name]
        a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
        try:
            for exact in (False, True):
                got = ctx.dense_host(a, b, symmetric=symmetric, exact=exact, mirror=mirror)
                assert got.shape == (A.shape[0], B.shape[1])
                _all_plus_zero(got, f"{name} exact={exact}")
        finally:
            a.close(); b.close()


# ------------------------------------------------------------------------------ dense triple product
TRIPLE_VARIANTS = {"upper": (False, False, 0, ep.N_TRIPLE), "full": (True, False, 0, ep.N_TRIPLE), "mirror": (False, True, 0, ep.N_TRIPLE),
                   "rows-37-150": (False, False, 37, 150), "rows-199-200": (False, False, 199, 200)}


@pytest.mark.parametrize("variant", list(TRIPLE_VARIANTS))
@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_dense_triple_is_plus_zero_over_a_nan_sentinel(ctx, stage2, name, variant):
    H, Q = ep.triple_case(name)
    full, mirror, r0, r1 = TRIPLE_VARIANTS[variant]
    n = ep.N_TRIPLE
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        assert h.nnz > 0 and q.nnz > 0
        for exact in (False, True):
            what = f"{name} {variant} ring={stage2} exact={exact}"
            out = _nan_tensor(ctx, (r1 - r0) * n + SLACK)
            _settle(ctx)
            ctx.triple_into(h, q, out.data_ptr(), full=full, row_begin=r0, row_end=r1, exact=exact, mirror=mirror)
            ctx.synchronize()
            _sentinel_kept(out, (r1 - r0) * n, what)
            _all_plus_zero(out[:(r1 - r0) * n].cpu().numpy(), what)
        got = ctx.triple_host(h, q, full=full, row_begin=r0, row_end=r1, exact=True, mirror=mirror)
        assert got.shape == (r1 - r0, n)
        _all_plus_zero(got, f"{name} {variant} ring={stage2} host")
    finally:
        h.close(); q.close()


# ------------------------------------------------------------------------------ CSR mirror epilogue
MIRROR_CASES = ["missed_rows-sorted-sym", "strictly_lower-sym"] + [f"lower_plus_one-{v}" for v in ep.PLUS_ONE_VARIANTS]


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name", MIRROR_CASES)
def test_mirrored_csr(ctx, name, where):
    """The full symmetric CSR of an upper triangle without entries is the empty n x n matrix (a row pointer of zeros); the
    mirror of one diagonal entry is that entry.  spgemm_mirrored_torch used to raise SmmError ("NULL CSR array") on the
    empty ones: its torch.empty(0) buffers have no address, and smm_csr_mirror_fill refuses NULL arrays."""
    A, B, symmetric = CSR_CASES[name]
    assert symmetric and A.shape[0] == B.shape[1]
    (wp, wi, wv), mag = _want(name)
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        for exact in (False, True):
            what = f"{name} {where} exact={exact}"
            if where == "host":
                gp, gi, gv = ctx.spgemm_host_mirrored(a, b, exact=exact)
            else:
                import torch
                tp, ti, tv = ctx.spgemm_mirrored_torch(a, b, exact=exact)
                ctx.synchronize()
                _settle(ctx)
                assert tp.is_cuda and tp.dtype == torch.int64 and ti.dtype == torch.int32 and tv.dtype == torch.float64
                gp, gi, gv = tp.cpu().numpy(), ti.cpu().numpy(), tv.cpu().numpy()
            assert gp.dtype == np.int64 and np.array_equal(gp, wp), f"{what}: indptr"
            assert gi.dtype == np.int32 and np.array_equal(gi, wi), f"{what}: indices"
            _check_values(gv, wv, mag, exact, what)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------ sparse triple, masked triple, masked product
ROW_RANGES = [(0, ep.N_TRIPLE), (37, 150), (199, 200), (60, 60)]


@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_sparse_triple_is_empty(ctx, block_budget, name):
    import torch
    H, Q = ep.triple_case(name)
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        for exact in (False, True):
            for full, (r0, r1) in [(True, ROW_RANGES[0])] + [(False, r) for r in ROW_RANGES]:
                what = f"{name} full={full} rows [{r0}, {r1}) exact={exact} budget={block_budget}"
                gp, gi, gv = ctx.triple_sparse_host(h, q, full=full, row_begin=r0, row_end=r1, exact=exact)
                assert gp.dtype == np.int64 and gp.shape == (r1 - r0 + 1,) and not gp.any(), f"{what}: indptr"
                assert gi.dtype == np.int32 and gi.size == 0 and gv.dtype == np.float64 and gv.size == 0, what
                tp, ti, tv = ctx.triple_sparse_torch(h, q, full=full, row_begin=r0, row_end=r1, exact=exact)
                ctx.synchronize()
                assert tp.dtype == torch.int64 and tuple(tp.shape) == (r1 - r0 + 1,) and not bool(tp.any()), f"{what}: indptr (torch)"
                assert ti.numel() == 0 and tv.numel() == 0 and ti.dtype == torch.int32 and tv.dtype == torch.float64, what
    finally:
        h.close(); q.close()


def _mirrored_pattern(U):
    F = (U + U.T).tocsr()
    F.sum_duplicates()
    F.sort_indices()
    return F


@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_masked_triple_is_the_mask_filled_with_plus_zero(ctx, block_budget, masked_mode, name):
    import torch
    H, Q = ep.triple_case(name)
    M = ep.triple_mask()
    h, q, mk = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q), ctx.csr_from_scipy(M)
    try:
        for exact in (False, True):
            for full, (r0, r1) in [(True, ROW_RANGES[0])] + [(False, r) for r in ROW_RANGES]:
                what = f"{name} full={full} rows [{r0}, {r1}) exact={exact} budget={block_budget} mode={masked_mode}"
                U = upper_mask(M, r0, r1)
                P = _mirrored_pattern(U) if full else U
                gp, gi, gv = ctx.triple_sparse_host(h, q, full=full, row_begin=r0, row_end=r1, exact=exact, mask=mk)
                assert np.array_equal(gp, P.indptr.astype(np.int64)) and np.array_equal(gi, P.indices), f"{what}: the pattern is not the mask's"
                assert gv.shape == (P.nnz,)
                _all_plus_zero(gv, what)
                tp, ti, tv = ctx.triple_sparse_torch(h, q, full=full, row_begin=r0, row_end=r1, exact=exact, mask=mk)
                ctx.synchronize()
                assert np.array_equal(tp.cpu().numpy(), P.indptr.astype(np.int64)) and np.array_equal(ti.cpu().numpy(), P.indices), what
                assert tv.dtype == torch.float64
                _all_plus_zero(tv.cpu().numpy(), f"{what} (torch)")
    finally:
        h.close(); q.close(); mk.close()


def _masked_cases():
    A, B, M = ep.masked_unreached()
    out = {"masked_unreached": (A, B, M)}
    for v in ep.MISSED_VARIANTS:
        A, B, _ = ep.missed_rows(v)
        out[f"missed_rows-{v}"] = (A, B, ep.missed_rows_mask())
    return out


MASKED_CASES = _masked_cases()


@pytest.mark.parametrize("name", list(MASKED_CASES))
def test_masked_product_is_plus_zero(ctx, masked_mode, name):
    A, B, M = MASKED_CASES[name]
    a, b, mk = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B), ctx.csr_from_scipy(M)
    try:
        assert mk.is_canonical() and a.nnz > 0 and b.nnz > 0 and mk.nnz > 0
        for exact in (False, True):
            what = f"{name} mode={masked_mode} exact={exact}"
            got = ctx.spgemm_masked_host(a, b, mk, exact=exact)
            assert got.shape == (M.nnz,)
            _all_plus_zero(got, what)
            out = _nan_tensor(ctx, M.nnz + SLACK)
            _settle(ctx)
            ctx.spgemm_masked_into(a, b, mk, out.data_ptr(), exact=exact)
            ctx.synchronize()
            _sentinel_kept(out, M.nnz, what)
            _all_plus_zero(out[:M.nnz].cpu().numpy(), f"{what} (device)")
    finally:
        a.close(); b.close(); mk.close()


# ------------------------------------------------------------------------------ H (Q (H^T X))
@pytest.mark.parametrize("budget", [0, 1], ids=["budget-default", "one-column"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_triple_apply_is_plus_zero_over_a_nan_sentinel(ctx, name, mode, budget):
    """Every stage adds +-0.0 products to a sum that starts at +0.0 (or has no product at all): +0.0, fused or not."""
    from sparse_matrix_mult_amd.engine import SMM_EXACT
    H, Q = ep.triple_case(name)
    n, k, ldy = ep.N_TRIPLE, 5, 8
    X = np.random.default_rng(41).standard_normal((n, k))
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    ctx.tune_spmm(mode, budget)                                # (budget 1 byte: blocks of one column)
    try:
        for exact in (False, True):
            what = f"{name} mode={mode} budget={budget} exact={exact}"
            for x in (X, X[:, 0].copy()):
                got = ctx._host_blocks(ctx.lib.smm_triple_apply_host, (h, q), x, n, n, SMM_EXACT if exact else 0, "X",
                                       f"H has {n}", fill=_nan_array)
                assert got.shape == x.shape
                _all_plus_zero(got, f"{what} host k={x.shape[1] if x.ndim == 2 else 1}")
            import torch
            dx = torch.from_numpy(X).to(torch.device("cuda", ctx.device))
            dy = _nan_tensor(ctx, n * ldy + SLACK)
            ctx.triple_apply_into(h, q, dx, k, k, dy, ldy, exact=exact)
            _sentinel_kept(dy, n * ldy, what)
            Y = dy[:n * ldy].view(torch.int64).cpu().numpy().reshape(n, ldy)
            assert not Y[:, :k].any(), f"{what}: the device block is not +0.0"
            assert np.all(Y[:, k:] == np.int64(NAN_BITS)), f"{what}: the padding between the rows of Y was written"
    finally:
        ctx.tune_spmm(0, 0)
        h.close(); q.close()


# ------------------------------------------------------------------------------ innovation solve and log-determinant
def _same_info(got, want, what, fields=("iterations", "status", "residual_sq", "rhs_sq")):
    for f in fields:
        g, w = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        assert g.shape == w.shape, f"{what}: {f}"
        same = np.array_equal(_bits(g), _bits(w)) if g.dtype == np.float64 else np.array_equal(g, w)
        assert same, f"{what}: {f} differs: got {g.ravel()[:6]}, want {w.ravel()[:6]}"


@functools.lru_cache(maxsize=None)
def _restated_solve(name):
    from cg_restatement import diag_csr, restate_cg
    H, Q = ep.triple_case(name)
    return restate_cg(H, Q, diag_csr(ep.solve_diagonal()), ep.solve_rhs(), tol=1e-8, maxiter=50)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_innovation_solve_with_an_empty_s_runs_the_device_cg(name, device):
    """H and Q hold entries, so the call goes to the device CG (the host branch is for nnz == 0): under set_exact(True) Z
    and info are the bits of the restated CG, whose three products are all +0.0 -- CG on R alone."""
    import sparse_matrix_mult_amd as pkg
    H, Q = ep.triple_case(name)
    r, D = ep.solve_diagonal(), ep.solve_rhs()
    assert H.nnz > 0 and Q.nnz > 0                          # not matrix_ops' host branch
    wz, winfo = _restated_solve(name)
    old = (pkg.set_exact(True), pkg.set_result_device(device))
    try:
        z, info = pkg.innovation_solve(H, Q, r, D, tol=1e-8, maxiter=50)
        z1, info1 = pkg.innovation_solve(H, Q, sp.csr_matrix(sp.diags(r)), D[:, 1], tol=1e-8, maxiter=50)
    finally:
        pkg.set_exact(old[0]); pkg.set_result_device(old[1])
    if device:
        z, z1 = z.cpu().numpy(), z1.cpu().numpy()
    assert np.all(info.status == 0) and info.converged
    assert np.all(info.iterations > 0) and np.array_equal(info.iterations, winfo.iterations)
    _same_info(info, winfo, name)
    assert np.array_equal(_bits(z), _bits(wz)), f"{name}: Z differs from the restated CG"
    assert z1.shape == (ep.N_TRIPLE,) and np.array_equal(_bits(z1), _bits(wz[:, 1])) and info1.iterations[0] == winfo.iterations[1]


@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_innovation_logdet_with_an_empty_s(name):
    import sparse_matrix_mult_amd as pkg
    from cg_restatement import diag_csr
    from slq_restatement import restate_cg_coef, restate_probes, slq
    H, Q = ep.triple_case(name)
    n, probes, seed, maxiter = ep.N_TRIPLE, 4, 7, 20
    r, D = ep.solve_diagonal(), ep.solve_rhs()
    m = D.shape[1]
    batch = np.concatenate([D, restate_probes(n, probes, seed)], axis=1)
    wz, winfo = restate_cg_coef(H, Q, diag_csr(r), batch, tol=1e-8, maxiter=maxiter)
    assert H.nnz > 0 and Q.nnz > 0
    old = pkg.set_exact(True)
    try:
        res = pkg.innovation_logdet(H, Q, r, probes=probes, seed=seed, tol=1e-8, maxiter=maxiter, d=D, return_solutions=True)
    finally:
        pkg.set_exact(old)
    assert res.positive_definite and np.all(res.info.status == 0) and np.all(res.info_d.status == 0)
    assert np.all(res.info.iterations > 0) and np.array_equal(res.info.iterations, winfo.iterations[m:])
    for f in ("iterations", "status", "residual_sq", "rhs_sq"):
        want = np.asarray(getattr(winfo, f))
        _same_info(res.info_d, type("I", (), {f: want[:m]}), f"{name} d", fields=(f,))
        _same_info(res.info, type("I", (), {f: want[m:]}), f"{name} probes", fields=(f,))
    assert np.array_equal(_bits(res.info.alpha), _bits(winfo.alpha[:, m:])) and np.array_equal(_bits(res.info.beta), _bits(winfo.beta[:, m:]))
    assert np.array_equal(_bits(res.Z), _bits(wz[:, :m])) and np.array_equal(_bits(res.solutions), _bits(wz[:, m:]))
    samples, logdet, stderr, lo, hi = slq(res.info, n)     # the quadrature of the recorded coefficients
    assert np.array_equal(res.samples, samples) and res.logdet == logdet and res.stderr == stderr
    assert (res.lambda_min, res.lambda_max) == (lo, hi)


# ------------------------------------------------------------------------------ the public entry points
def _zero_like(M):
    return sp.csr_matrix(M.shape, dtype=np.float64)


def _describe(res):
    """What two results must share: type, shape, dtypes, nnz, row pointer (dense: every element's bits)."""
    import torch
    from sparse_matrix_mult_amd import DeviceCSRResult
    if isinstance(res, DeviceCSRResult):
        assert res.indptr.is_cuda and res.indices.is_cuda and res.data.is_cuda
        return ("DeviceCSRResult", tuple(res.shape), str(res.indptr.dtype), str(res.indices.dtype), str(res.data.dtype), res.nnz,
                res.indptr.cpu().numpy().tolist(), res.indices.cpu().numpy().tolist(), _bits(res.data.cpu().numpy()).tolist())
    if sp.isspmatrix_csr(res):
        return ("csr_matrix", tuple(res.shape), str(res.indptr.dtype), str(res.indices.dtype), str(res.data.dtype), res.nnz,
                res.indptr.tolist(), res.indices.tolist(), _bits(res.data).tolist())
    if isinstance(res, torch.Tensor):
        assert res.is_cuda
        return ("Tensor", tuple(res.shape), str(res.dtype), bool(_bits(res.cpu().numpy()).any()))
    assert isinstance(res, np.ndarray)
    return ("ndarray", tuple(res.shape), str(res.dtype), bool(_bits(res).any()))


def _switches(pkg, device, full_symmetric, exact):
    return pkg.set_result_device(device), pkg.set_full_symmetric(full_symmetric), pkg.set_exact(exact)


def _restore(pkg, old):
    pkg.set_result_device(old[0]); pkg.set_full_symmetric(old[1]); pkg.set_exact(old[2])


def _public_pairs():
    out = {}
    for v in ep.MISSED_VARIANTS:
        out[f"missed_rows-{v}"] = ep.missed_rows(v)[:2] + ((False, True),)
    out["strictly_lower"] = ep.strictly_lower() + ((True,),)
    for v in ep.VECTOR_VARIANTS:
        out[f"vectors-{v}"] = ep.vectors(v) + ((False, True),)
    return out


PUBLIC_PAIRS = _public_pairs()
ALL_SWITCHES = [(d, f, e) for d in (False, True) for f in (False, True) for e in (False, True)]


@pytest.mark.parametrize("name", list(PUBLIC_PAIRS))
def test_sparse_matrix_multiply_equals_the_zero_operand_route(capsys, name):
    """Every combination of output_format, symmetric, set_result_device, set_full_symmetric and set_exact returns what
    the same call returns for an operand with nnz == 0 (matrix_ops' _zero_result), and prints the reference's line once."""
    import sparse_matrix_mult_amd as pkg
    A, B, symmetrics = PUBLIC_PAIRS[name]
    assert A.nnz > 0 and B.nnz > 0
    for device, full_symmetric, exact in ALL_SWITCHES:
        old = _switches(pkg, device, full_symmetric, exact)
        try:
            for fmt in ("sparse", "dense"):
                for symmetric in symmetrics:
                    what = f"{name} {fmt} symmetric={symmetric} device={device} full_symmetric={full_symmetric} exact={exact}"
                    capsys.readouterr()
                    got = pkg.sparse_matrix_multiply(A, B, output_format=fmt, symmetric=symmetric)
                    printed = capsys.readouterr().out
                    assert printed.count(ZERO_LINE) == 1 and printed.strip() == ZERO_LINE, f"{what}: printed {printed!r}"
                    twin = pkg.sparse_matrix_multiply(_zero_like(A), B, output_format=fmt, symmetric=symmetric)
                    assert _describe(got) == _describe(twin), what
                    assert _describe(got)[-1] in ([], False), what                 # no values / every element +0.0
                    if device and fmt == "sparse":
                        _three_ways(pkg, got, B, what)
        finally:
            _restore(pkg, old)
            capsys.readouterr()
    pkg.clear_cache()


def _three_ways(pkg, res, B, what):
    """A device result without entries still serves: as scipy, as torch's CSR, and pinned as the next product's operand."""
    import torch
    S = res.to_scipy()
    assert sp.isspmatrix_csr(S) and S.shape == res.shape and S.nnz == 0 and not S.indptr.any(), what
    T = res.to_torch_sparse_csr()
    y = T @ torch.ones(res.shape[1], 1, dtype=torch.float64, device=res.data.device)
    assert tuple(y.shape) == (res.shape[0], 1) and not bool(y.any()), what
    P = pkg.pin_operand(res)
    try:
        assert P.shape == res.shape and P.nnz == 0
        R = sp.csr_matrix(np.ones((res.shape[1], 3)))
        again = pkg.sparse_matrix_multiply(P, R)
        assert isinstance(again, pkg.DeviceCSRResult) and again.shape == (res.shape[0], 3) and again.nnz == 0, what
        assert not bool(again.indptr.any()), what
    finally:
        P.unpin()


@pytest.mark.parametrize("name", ep.TRIPLE_CASES)
def test_sparse_triple_product_equals_the_zero_operand_route(capsys, name):
    import sparse_matrix_mult_amd as pkg
    H, Q = ep.triple_case(name)
    M = ep.triple_mask()
    for device, _, exact in [s for s in ALL_SWITCHES if not s[1]]:
        old = _switches(pkg, device, False, exact)
        try:
            for mask in (None, M):
                for full in (False, True):
                    what = f"{name} mask={mask is not None} full={full} device={device} exact={exact}"
                    got = pkg.sparse_triple_product(H, Q, compute_full_matrix=full, mask=mask)
                    twin = pkg.sparse_triple_product(_zero_like(H), Q, compute_full_matrix=full, mask=mask)
                    assert _describe(got) == _describe(twin), what
                    d = _describe(got)
                    assert d[1] == (ep.N_TRIPLE, ep.N_TRIPLE) and not any(d[-1]), f"{what}: a value is not +0.0"
                    if mask is None:
                        assert d[5] == 0 and not any(d[6]), what
                    else:
                        U = upper_mask(M)
                        P = _mirrored_pattern(U) if full else U
                        assert d[6] == P.indptr.tolist() and d[7] == P.indices.tolist(), f"{what}: the pattern is not the mask's"
                    if device:
                        S = got.to_scipy()
                        assert S.shape == (ep.N_TRIPLE, ep.N_TRIPLE) and S.nnz == d[5], what
                        got.to_torch_sparse_csr()
            # the dense triple of the reference's entry point: every element +0.0, and its line.  (No twin here: with an
            # operand without entries that call returns the reference's H.rows x Q.cols sparse zero, not the dense n x n.)
            for cfm in (None, 1, "mirror"):
                capsys.readouterr()
                T = pkg.sparse_matrix_multiply(H, Q, use_triple_product=True, compute_full_matrix=cfm)
                assert capsys.readouterr().out.count(ZERO_LINE) == 1
                assert _describe(T) == ("Tensor" if device else "ndarray", (ep.N_TRIPLE, ep.N_TRIPLE),
                                        "torch.float64" if device else "float64", False), f"{name} cfm={cfm} device={device}"
        finally:
            _restore(pkg, old)
            capsys.readouterr()
    pkg.clear_cache()


@pytest.mark.parametrize("name", list(MASKED_CASES))
def test_masked_matrix_multiply_equals_the_zero_operand_route(name):
    import sparse_matrix_mult_amd as pkg
    A, B, M = MASKED_CASES[name]
    for device, _, exact in [s for s in ALL_SWITCHES if not s[1]]:
        old = _switches(pkg, device, False, exact)
        try:
            what = f"{name} device={device} exact={exact}"
            got = pkg.masked_matrix_multiply(A, B, M)
            twin = pkg.masked_matrix_multiply(_zero_like(A), B, M)
            d = _describe(got)
            assert d == _describe(twin), what
            assert d[5] == M.nnz and d[6] == M.indptr.tolist() and d[7] == M.indices.tolist(), f"{what}: the pattern is not the mask's"
            assert not any(d[-1]), f"{what}: a value is not +0.0"
        finally:
            _restore(pkg, old)
    pkg.clear_cache()


# ------------------------------------------------------------------------------ the legacy symbols
def test_legacy_symbols_on_missed_rows(legacy, oracle):  # noqa: F811
    A, B, _ = ep.missed_rows()
    a, b = _to_sparsemat(legacy, A), _to_sparsemat(legacy, B)
    try:
        for symmetric, fn in ((False, legacy.sparse_nosym), (True, legacy.sparse_sym)):
            out = SparseMat()
            fn(ctypes.byref(a), ctypes.byref(b), ctypes.byref(out), 5)
            want = oracle.sparse(arrays(A), arrays(B), 300, symmetric=symmetric)
            assert (out.rows, out.cols, out.nzmax) == (300, 300, 0) and len(want[1]) == 0
            if out.rowPtr:
                assert np.array_equal(np.ctypeslib.as_array(out.rowPtr, shape=(301,)), want[0])
            ptr, idx, val = _from_sparsemat(out)
            assert np.array_equal(ptr, want[0]) and len(idx) == 0 and len(val) == 0
            legacy.destroy_sparsemat(ctypes.byref(out))
        for symmetric, fn in ((False, legacy.dense_nosym), (True, legacy.dense_sym)):
            d = DArray()
            fn(ctypes.byref(a), ctypes.byref(b), ctypes.byref(d))
            assert bool(d.array) and (d.rows, d.cols) == (300, 300)
            got = np.ctypeslib.as_array(d.array, shape=(d.rows, d.cols)).copy()
            legacy.destroy_darray(ctypes.byref(d))
            want = oracle.dense(arrays(A), arrays(B), 300, symmetric=symmetric)
            assert np.array_equal(_bits(got), _bits(want))
            _all_plus_zero(got, f"legacy dense symmetric={symmetric}")
    finally:
        for s in (a, b):
            legacy.destroy_sparsemat(ctypes.byref(s))
