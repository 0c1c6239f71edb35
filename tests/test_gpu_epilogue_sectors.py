"""Index ownership in the CSR epilogue of smm_numeric (SMM_EPI_OWNER; the rule: tests/epilogue_owner_restatement.py).

A store that the ownership predicates drop can hide behind torch.empty: the caching allocator hands back a block that
still holds the previous, correct result.  So every product here is written into buffers that were POISONED first
(negative indices, NaN values, indptr -1), compared with the oracle -- indptr and indices bit for bit, values bit for
bit under exact=True and to 1e-10 otherwise -- and written a second time into the same, re-poisoned buffers after a
different product has gone through the context.  The tile kernel is forced for every row (tune_hash(0, 0)) with
several tiles per row; the table of every case is rebuilt on the CPU from the operands alone to show that the case
holds what its name says (a tail, none, sub-runs shorter than a granule, ...).  The SMM_EXACT walk keeps the stores it had
(ownership loses there, profiles/epi_owner_ab.txt); its cases run all the same: same epilogue code, other template branch."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import epilogue_owner_restatement as own
from helpers import arrays, rand_csr, rel_err

pytestmark = pytest.mark.gpu

SENTINEL = -7
WAVES = {1000: (16, 8), 300: (4, 4), 200: (8, 2), 64: (8, 1)}      # lds_cols -> waves of the default / the exact walk


def _rows_at_least(m, n, lo, hi, seed):
    """Every row holds between lo and hi distinct sorted columns."""
    r = np.random.default_rng(seed)
    cnt = r.integers(lo, hi + 1, size=m)
    idx = np.concatenate([np.sort(r.choice(n, size=int(c), replace=False)) for c in cnt]).astype(np.int32)
    ptr = np.concatenate(([0], np.cumsum(cnt))).astype(np.int32)
    return sp.csr_matrix((r.uniform(0.0, 1.0, size=idx.size), idx, ptr), shape=(m, n))


def _case_mixed():
    # (the issue's case 1 has no tail at these densities: every step appends 50 columns or more.  This one thins half of
    # B's rows to ~8 entries, so that rows of C end in a run of short steps behind long sub-runs)
    A, B = rand_csr(300, 400, 0.05, 101), rand_csr(400, 3000, 0.03, 102).tolil()
    thin = rand_csr(400, 3000, 0.0027, 103).tolil()
    for j in range(200, 400):
        B[j] = thin[j]
    B = B.tocsr(); B.sort_indices()
    return A, B


def _case_lead():
    # B's first 100 rows hold no column below 1000: the first steps of most rows of C are empty in tile 0
    A = rand_csr(300, 400, 0.05, 131)
    top = sp.hstack([sp.csr_matrix((100, 1000)), rand_csr(100, 2000, 0.045, 132)])
    B = sp.vstack([top, rand_csr(300, 3000, 0.03, 133)]).tocsr(); B.sort_indices()
    return A, B


def _case_square():
    A = rand_csr(600, 300, 0.15, 141)
    B = A.T.tocsr(); B.sort_indices()
    return A, B


CASES = {
    "long-subruns": lambda: (rand_csr(300, 400, 0.05, 101), rand_csr(400, 3000, 0.03, 102)),
    "long-subruns-and-tail": _case_mixed,
    "all-tail": lambda: (rand_csr(300, 400, 0.05, 111), rand_csr(400, 3000, 0.005, 112)),
    "no-tail": lambda: (_rows_at_least(300, 400, 1, 2, 121), _rows_at_least(400, 3000, 100, 140, 122)),
    "first-steps-empty-in-tile-0": _case_lead,
    "square": _case_square,
}


@functools.lru_cache(maxsize=None)
def _operands(case):
    A, B = CASES[case]()
    A.sort_indices()
    return A, B


@functools.lru_cache(maxsize=None)
def _want(case, symmetric):
    """The oracle's product, computed once per case and shared (read-only)."""
    from oracle import oracle
    A, B = _operands(case)
    ptr, idx, val = oracle.sparse(arrays(A), arrays(B), B.shape[1], symmetric=symmetric)
    for x in (ptr, idx, val):
        x.setflags(write=False)
    return ptr, idx, val


@functools.lru_cache(maxsize=None)
def _stats(case, lds_cols, exact, symmetric=False):
    A, B = _operands(case)
    if exact:
        nct, wc = own.exact_geometry(B.shape[1], lds_cols, WAVES[lds_cols][1])
    else:
        nct, wc = own.shared_geometry(B.shape[1], lds_cols)
    return own.table_stats(A, B, nct, wc, own.TAIL_MIN_EXACT if exact else own.TAIL_MIN_DEFAULT, symmetric=symmetric)


class _Buffers:
    def __init__(self, torch, rows, nnz):
        dev = torch.device("cuda", 0)
        self.torch = torch
        self.indptr = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        self.indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        self.data = torch.empty(max(nnz, 1), dtype=torch.float64, device=dev)
        self.nnz = nnz

    def run(self, ctx, plan):
        self.indptr.fill_(-1); self.indices.fill_(SENTINEL); self.data.fill_(float("nan"))
        self.torch.cuda.synchronize()
        plan.numeric_into(self.indptr.data_ptr(), self.indices.data_ptr(), self.data.data_ptr())
        ctx.synchronize()
        return (self.indptr.cpu().numpy(), self.indices[:self.nnz].cpu().numpy(), self.data[:self.nnz].cpu().numpy())


def _check(got, want, exact, what):
    gp, gi, gv = got
    wp, wi, wv = want
    assert np.array_equal(gp, np.asarray(wp, dtype=np.int64)), f"{what}: indptr differs"
    lost = np.flatnonzero(gi == SENTINEL)
    assert lost.size == 0, f"{what}: {lost.size} indices were never stored (first at {lost[:8]})"
    assert np.array_equal(gi, wi), f"{what}: indices differ at {np.flatnonzero(gi != wi)[:8]}"
    assert not np.isnan(gv).any(), f"{what}: {int(np.isnan(gv).sum())} values were never stored"
    if exact:
        assert np.array_equal(gv.view(np.int64), wv.view(np.int64)), f"{what}: values differ bitwise"
    else:
        assert rel_err(gv, wv) <= 1e-10, f"{what}: values differ, max rel {rel_err(gv, wv):.3e}"


def _shard(want, r0, r1):
    lo, hi = int(want[0][r0]), int(want[0][r1])
    return want[0][r0:r1 + 1] - lo, want[1][lo:hi], want[2][lo:hi]


def _twice(ctx, A, B, want, other, exact, kernel="smm_numeric", **kw):
    """The product into poisoned buffers, a different product through the same context, the product again."""
    import torch
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    oa, ob = ctx.csr_from_scipy(other[0]), ctx.csr_from_scipy(other[1])
    plan = oplan = None
    try:
        ctx.timing(True); ctx.timing_reset()
        plan = ctx.spgemm_plan(a, b, exact=exact, **kw)
        assert plan.nnz == want[1].size
        buf = _Buffers(torch, A.shape[0], plan.nnz)
        _check(buf.run(ctx, plan), want, exact, "first run")
        assert ctx.kernel_time(kernel)[1] >= 1, f"{kernel} did not run"
        oplan = ctx.spgemm_plan(oa, ob, exact=exact)
        _check(_Buffers(torch, other[0].shape[0], oplan.nnz).run(ctx, oplan), other[2], exact, "the product in between")
        _check(buf.run(ctx, plan), want, exact, "second run")
    finally:
        ctx.timing(False)
        for p in (plan, oplan):
            if p is not None:
                p.close()
        for x in (a, b, oa, ob):
            x.close()


@pytest.fixture
def tiles(ctx):
    """The tile kernel for every row; the geometry is set per test; the defaults come back afterwards."""
    ctx.tune_hash(0, 0)
    try:
        yield ctx
    finally:
        ctx.tune_hash(256, 2048); ctx.tune_shared(20000, 16); ctx.tune(18000, 8)
        ctx.tune_narrow(True); ctx.tune_slab(0, 0, 4)


def _geometry(ctx, lds_cols):
    ctx.tune_shared(lds_cols, WAVES[lds_cols][0])
    ctx.tune(lds_cols, WAVES[lds_cols][1])


def _other(case):
    """The product that goes through the context between the two runs of `case`."""
    name = "all-tail" if case != "all-tail" else "no-tail"
    A, B = _operands(name)
    return A, B, _want(name, False)


# what the CPU model must find in each case (counts over the rows of C)
CLAIMS = {
    "long-subruns": lambda st, lds: (st["long"] > 1000 or lds < 1000) and st["rs_mod16"] == set(range(16)),
    "long-subruns-and-tail": lambda st, lds: st["tail"] > 250 and (st["long"] > 1000 or lds < 1000) and st["rs_mod16"] == set(range(16)),
    "all-tail": lambda st, lds: st["all_tail"] > 250 and st["tail"] == 0 and st["no_tail"] == 0,
    "no-tail": lambda st, lds: st["no_tail"] > 250 and st["tail"] == 0 and st["all_tail"] == 0,
    "first-steps-empty-in-tile-0": lambda st, lds: st["lead_other_tile"] > 100,
}


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("lds_cols", [1000, 300, 64])
@pytest.mark.parametrize("case", ["long-subruns", "long-subruns-and-tail"])
def test_subruns_and_tail(tiles, case, lds_cols, exact):
    """Cases 1, 2 and 9: 3, 10 and 47 tiles.  At 47 tiles the sub-runs hold 1 to 3 entries: most own no index at all and
    one granule holds entries of several sub-runs."""
    st = _stats(case, lds_cols, exact)
    assert CLAIMS[case](st, lds_cols), st
    if lds_cols < 1000:         # 10 tiles: sub-runs of ~9 entries; 47 tiles: of 1 to 3
        assert st["short"] > 10000 and st["shared_granule"] > (1000 if lds_cols == 64 else 300), st
    _geometry(tiles, lds_cols)
    A, B = _operands(case)
    _twice(tiles, A, B, _want(case, False), _other(case), exact)


@pytest.mark.parametrize("case", ["all-tail", "no-tail", "first-steps-empty-in-tile-0"])
def test_rows_of_one_kind(tiles, case):
    """Cases 3, 4 and 5."""
    st = _stats(case, 1000, False)
    assert CLAIMS[case](st, 1000), st
    _geometry(tiles, 1000)
    A, B = _operands(case)
    _twice(tiles, A, B, _want(case, False), _other(case), False)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["full", "symmetric"])
def test_square_symmetric_and_shard(tiles, symmetric, exact):
    """Cases 6 and 9: 600 x 600 in 3 tiles; under symmetric=True the tail's index owner is the tile of the diagonal, and
    a row shard moves the diagonal with row_offset."""
    st = _stats("square", 200, exact, symmetric)
    assert st["tail"] > 100 and st["long"] > 500, st            # rows that mix long sub-runs with a tail
    _geometry(tiles, 200)
    A, B = _operands("square")
    want = _want("square", symmetric)
    _twice(tiles, A, B, want, _other("square"), exact, symmetric=symmetric)
    r0, r1 = 230, 470           # rows whose diagonal lies in tiles 1 and 2
    _twice(tiles, A[r0:r1], B, _shard(want, r0, r1), _other("square"), exact, symmetric=symmetric, row_offset=r0)


@pytest.mark.parametrize("lds_cols", [1000, 64])
def test_int_lists(tiles, lds_cols):
    """Case 7: 32-bit lists (tune_narrow(False))."""
    tiles.tune_narrow(False)
    _geometry(tiles, lds_cols)
    A, B = _operands("long-subruns-and-tail")
    _twice(tiles, A, B, _want("long-subruns-and-tail", False), _other("long-subruns-and-tail"), False)


@pytest.mark.parametrize("case", ["long-subruns-and-tail", "all-tail"])
def test_emit_after_dense_slab(tiles, case):
    """Case 8: tune_slab(2, 0, 4) -- the tile comes from smm_dense_slab's scratch rows, the emission is the same epilogue."""
    tiles.tune_slab(2, 0, 4)
    _geometry(tiles, 1000)
    A, B = _operands(case)
    _twice(tiles, A, B, _want(case, False), _other(case), False, kernel="smm_emit")
