"""Conditions on the inputs of tests/test_gpu_width_boundaries.py, checked without a GPU: the operands of
tests/width_cases.py reach the path each case is named for, touch the first and the last column in every row class, and
the oracle's result for them is the product."""
import numpy as np
import pytest

import width_cases as wc
from width_cases import POPULATIONS, WIDTHS

CASES = [(n, pop) for n in WIDTHS for pop in POPULATIONS]
IDS = [f"{n}-{pop}" for n, pop in CASES]


def _path(n, pop, **kw):
    A, B = wc.operands(n, pop)
    return wc.expected_path(n, A, B, **kw)


def test_width_list_holds_both_sides_of_every_threshold():
    assert list(WIDTHS) == sorted(set(WIDTHS))
    assert [(a, b) for a, b in zip(WIDTHS, WIDTHS[1:]) if b - a == 1] == list(wc.THRESHOLD_PAIRS)
    for i, hs in enumerate(wc.HS):                              # bm_words >= HS[i] from the upper width of the pair on
        lo = hs * 32 - 32
        assert (lo, lo + 1) in wc.THRESHOLD_PAIRS and (lo + 31) // 32 == hs - 1 and (lo + 32) // 32 == hs
    assert (wc.CCS_MAX_WS, wc.CCS_MAX_WS + 1) in wc.THRESHOLD_PAIRS
    # ccs_guard_col: the last guard column of the widest slab is 65503; one more bitmap word and it would be 0xffff, the dummy
    assert ((wc.CCS_MAX_WS + 31) // 32 + 63) * 32 + 31 == 65503 and ((wc.CCS_MAX_WS + 32) // 32 + 63) * 32 + 31 == 0xffff


@pytest.mark.parametrize("n,pop", CASES, ids=IDS)
def test_operands_hold_the_patterns_and_populations(n, pop):
    A, B = wc.operands(n, pop)
    lay = wc.layout(n, pop)
    m = 256 if pop == "light" else wc.heavy_rows(n)
    assert A.shape == (m, wc.K) and B.shape == (wc.K, n)
    for M in (A, B):                                            # canonical, signed values in [-1, 1)
        for i in range(M.shape[0]):
            assert np.all(np.diff(M.indices[M.indptr[i]:M.indptr[i + 1]]) > 0)
        assert M.data.min() >= -1.0 and M.data.max() < 1.0 and (M.data < 0).any() and (M.data > 0).any()
    row = lambda i: B.indices[B.indptr[i]:B.indptr[i + 1]]
    assert np.array_equal(row(lay.dense), np.arange(n))
    for r in range(8):
        assert np.array_equal(row(lay.residue[r]), np.arange(r, n, 8))
    assert np.array_equal(row(lay.edge), np.r_[np.arange(40), np.arange(n - 40, n)])
    spec = wc.special_columns(n)
    for i, s in enumerate(lay.short):
        assert 3 <= len(row(s)) <= 60 and spec[i % 7] in row(s)
    for i, s in enumerate(lay.mid):
        assert len(row(s)) == wc.MID[i] == wc.HS[i] // 2 and row(s)[0] == 0 and row(s)[-1] == n - 1
    na = np.diff(A.indptr)
    assert na.max() <= 6 and (na == 0).sum() >= 3
    # first-touch order in both directions: some row of A meets the dense (or a residue) row before a short one, another after
    long_rows = {lay.dense, *lay.residue}
    before = after = False
    for i in range(m):
        named = list(A.indices[A.indptr[i]:A.indptr[i + 1]])
        longs = [k for k, r in enumerate(named) if r in long_rows]
        shorts = [k for k, r in enumerate(named) if r not in long_rows]
        if longs and shorts:
            before |= min(longs) < max(shorts)
            after |= min(shorts) < max(longs)
    assert before and after
    # populations
    b_len = np.diff(B.indptr)
    prod = np.array([b_len[A.indices[A.indptr[i]:A.indptr[i + 1]]].sum() for i in range(m)])
    names_long = np.array([bool(long_rows & set(A.indices[A.indptr[i]:A.indptr[i + 1]])) for i in range(m)])
    names_dense = np.array([lay.dense in A.indices[A.indptr[i]:A.indptr[i + 1]] for i in range(m)])
    assert prod.sum() <= 2e7
    if pop == "light":
        assert 4 * (prod <= 200).sum() >= 3 * m and 16 * names_long.sum() <= m
    else:
        assert 4 * (prod > 2048).sum() >= 3 * m and names_dense.sum() == 8
    # classes interleaved: no class sits in one contiguous block of rows
    heavy_at = np.flatnonzero(prod > 2048)
    assert heavy_at.max() - heavy_at.min() + 1 > len(heavy_at)


@pytest.mark.parametrize("pop", POPULATIONS)
@pytest.mark.parametrize("exact", [False, True])
def test_path_differs_across_each_pair_in_the_named_field_only(pop, exact):
    pairs = wc.THRESHOLD_PAIRS if pop == "light" else wc.THRESHOLD_PAIRS_HEAVY
    for (lo, hi), want in pairs.items():
        a, b = _path(lo, pop, exact=exact).dispatch(), _path(hi, pop, exact=exact).dispatch()
        assert {k for k in a if a[k] != b[k]} == want, (lo, hi, a, b)


@pytest.mark.parametrize("n,pop", CASES, ids=IDS)
def test_expected_path_of_every_case(n, pop):
    for exact in (False, True):
        p = _path(n, pop, exact=exact)
        bm_words = (n + 31) // 32
        assert p.hash_classes == tuple(bm_words >= hs for hs in wc.HS)
        assert p.lds_bitmap == (n <= 1048544) and p.idle_col_fits16 == (n <= 65504)
        if pop == "light":                                      # never on the slab walk; tiny, hash and rest rows all there
            assert p.walk != "slab"
            assert p.slab_dominant == (n <= 16352)              # (without hash classes `dominant` holds by definition)
            assert p.walk == ("ccs" if n <= 63456 else "bitmap")
            assert p.list16 == (n < 65535)
            assert p.n_tiny > 0 and p.n_rest > 0
        else:
            assert p.slab_dominant
            assert p.walk == ("ccs" if n <= 63456 else "slab") and p.list16 == (n <= 63456 or p.walk == "slab")
            if p.walk == "slab":
                assert p.tps >= 1 and p.ws <= wc.CCS_MAX_WS and p.n_slabs >= 2 and p.n_slabs * p.ws >= n
        assert p.n_tiny + sum(p.n_hash) + p.n_rest == (p.row_class >= 0).sum()
        # every hash class that exists at this width has rows, among them one with the most products the class takes and
        # one with a few more than the class below takes; the rows beyond the last class that exists are bitmap rows
        for i, exists in enumerate(p.hash_classes):
            lo, hi = (wc.HS[i - 1] // 2 if i else 0), wc.HS[i] // 2
            in_range = (p.ub > lo) & (p.ub <= hi) & (p.row_class < 5)
            assert (in_range & (p.ub == hi)).any() and (i == 0 or (in_range & (p.ub <= lo + 5)).any())
            assert np.all(p.row_class[in_range] == (i if exists else 4))
            assert (p.n_hash[i] >= (3 if i else 1)) if exists else (p.n_hash[i] == 0)
        assert ((p.ub > 2048) & (p.ub <= 2053) & (p.row_class == 4)).any()
        assert wc.hash_launches(p) == (sum(p.hash_classes) if p.walk != "slab" else 0)
        # the 63456 | 63457 pair under the default geometry: two tiles of 15 865 columns per slab
        if (n, pop, exact) == (63457, "heavy", False):
            assert (p.tps, p.ws, p.n_slabs) == (2, 31730, 2)
        launches = wc.expected_launches(p)
        assert launches["smm_slab_rowcnt"] == (p.walk == "slab") and launches["smm_ccs_fill"] == (p.walk != "bitmap")


@pytest.mark.parametrize("n,pop", CASES, ids=IDS)
def test_oracle_result_holds_the_boundary_columns_and_is_the_product(oracle, n, pop):
    A, B = wc.operands(n, pop)
    ptr, idx, val = wc.oracle_result(n, pop)
    assert wc.oracle_result(n, pop)[1] is idx                   # cached for the GPU module
    p = wc.expected_path(n, A, B)
    m = A.shape[0]
    cnt = np.diff(ptr)
    assert cnt.max() == n                                       # a full row
    rows = np.repeat(np.arange(m), cnt)
    has_first = np.zeros(m, bool); has_first[rows[idx == 0]] = True
    has_last = np.zeros(m, bool); has_last[rows[idx == n - 1]] = True
    classes = {"tiny": p.row_class >= 5, "hash": (p.row_class >= 0) & (p.row_class <= 3), "rest": p.row_class == 4}
    for name, mask in classes.items():
        if mask.any():
            assert (mask & has_first & has_last).any(), f"no {name} row holds column 0 and column n - 1"
    assert classes["tiny"].any() and classes["rest"].any()
    # against scipy's product, sorted by column
    C = (A @ B).tocsr()
    C.sort_indices()
    assert np.array_equal(C.indptr, ptr)
    order = np.lexsort((idx, rows))
    assert np.array_equal(idx[order], C.indices)
    mag = (abs(A) @ abs(B)).tocsr()
    mag.sort_indices()
    assert np.array_equal(mag.indices, C.indices)
    assert np.all(np.abs(val[order] - C.data) <= 1e-12 * mag.data)
    # first-touch order is not column order wherever a short row of B comes before a long one
    assert not np.array_equal(idx, C.indices)


@pytest.mark.parametrize("n", [63456, 63457, 65504, 65505, 65534, 65535, 65536])
def test_further_cases_reach_their_paths(n):
    A, B = wc.operands(n, "heavy")
    U = wc.unsorted_with_repeat(B, wc.layout(n, "heavy"))
    assert U.nnz == B.nnz + 1 and not U.has_canonical_format
    r = wc.layout(n, "heavy").residue[(n - 1) % 8]
    cols = U.indices[U.indptr[r]:U.indptr[r + 1]]
    assert (cols == n - 1).sum() == 2 and np.any(np.diff(cols) < 0)
    p = wc.expected_path(n, A, U, safe=True)
    assert p.walk == "bitmap" and p.list16 == (n < 65535) and not any(p.hash_classes) and p.n_rest * 4 >= 3 * A.shape[0]
    # symmetric row shards: the last 256 rows are capped by the triangle (no slab walk), a shard across the first slab boundary is not
    ws = wc.slab_geometry(n)[1]
    assert (ws == 31730) == (n == 63457) and ws < n
    for row0, slab in ((n - 256, False), (ws - 128, n > 63456)):
        As, Bs = wc.symmetric_operands(n, row0)
        assert As.shape == (256, n) and Bs.shape == (n, n)
        ps = wc.expected_path(n, As, Bs, symmetric=True, row_offset=row0)
        assert (ps.walk == "slab") == slab and (not slab or ps.ws == ws)
    # 32-bit lists at a width that defaults to 16-bit ones
    assert not wc.expected_path(n, A, B, narrow=False).list16 and wc.expected_path(n, A, B, narrow=False).walk == "bitmap"
