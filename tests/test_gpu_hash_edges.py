"""The LDS hash (LdsHash, smm_rowclass.hpp) under its consumers -- masked SpGEMM (row and dot path), sparse triple product
stage 2, masked triple product -- with adversarial keys and rows on the class boundaries.

Keys: "window" keys all start in the last few slots of the table (tests/hash_keys.py), so a row of them wraps past the end
of the table and forms one probe chain as long as the row, a window key the row does not hold is a near-miss that walks
the whole chain before it reads as absent, and the lanes that insert them collide on one start slot; "random" keys of the
same universe are the easy case.  Lengths: 1, MAX - 1, MAX and MAX + 1 of either class (MAX + 1 is the next class: for
the workgroup class, the global path).  A missed key raises nothing -- a product is dropped --, so every mask position and
every entry of S is compared: bits against the oracle under exact, the files' own tolerances in default mode."""
import numpy as np
import pytest
import scipy.sparse as sp

import hash_keys as hk
from helpers import (RTOL, arrays, check_masked_values, check_triple_masked, check_triple_sparse, masked_want, rel_err,
                     triple_pattern, upper_mask)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1200)]
MODES = [0, 1, 2]          # auto, dot, row
KEYCASES = [("wave", "window"), ("wave", "random"), ("wave_one_slot", "window"), ("wg", "window"), ("wg", "random")]
LENGTHS = ["1", "max-1", "max", "max+1"]


def _keys(name, kind):
    """(class, universe, keys): a row of length L holds keys[:L]; keys[MAX + 1:] are held by no row."""
    c, _, universe, wk = hk.keyset(name)
    return c, universe, (wk if kind == "window" else hk.random_keys(name))


def _length(c, token):
    return {"1": 1, "max-1": c.MAX - 1, "max": c.MAX, "max+1": c.MAX + 1, "0": 0}[token]


def _others(universe, keys, count, seed):
    """count distinct columns of the universe that are no keys, ascending."""
    free = np.setdiff1d(np.arange(universe), keys)
    return np.sort(np.random.default_rng(seed).choice(free, size=count, replace=False))


def _csr(rows_cols, ncols, seed):
    """A CSR with the given columns per row, in the given order, values in [-1, 1)."""
    lens = [len(r) for r in rows_cols]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows_cols] + [np.zeros(0, np.int32)]).astype(np.int32)
    M = sp.csr_matrix((np.random.default_rng(seed).uniform(-1, 1, idx.size), idx, ptr), shape=(len(rows_cols), ncols))
    return M


# ------------------------------------------------------------------------------ operands
def _row_case(c, n, keys, lens, seed=1):
    """Masked row path: mask row i holds keys[:lens[i]].  B has rows of hits and near-misses (every second and every third
    key up to MAX + 1, so some mask positions are reached by no product), of keys no row holds next to the two boundary
    keys, of unrelated columns, and a mixed one; every row of A selects them all."""
    top = c.MAX + 1
    rest = _others(n, keys, 400, seed)
    b_rows = [np.sort(keys[0:top:2]), np.sort(keys[1:top:3]), np.sort(np.concatenate([keys[c.MAX - 1:top], keys[top:top + hk.SPARE - 1]])),
              rest[:300], np.sort(np.concatenate([keys[:3], keys[top + 5:top + 25], rest[300:]]))]
    B = _csr(b_rows, n, seed + 1)
    A = _csr([np.arange(len(b_rows))] * len(lens), len(b_rows), seed + 2)
    M = _csr([np.sort(keys[:L]) for L in lens], n, seed + 3)
    return A, B, M


def _dot_case(c, K, keys, lens, seed=11):
    """Masked dot path: row i of A holds keys[:lens[i]]; rows k of B exist for every key up to MAX + SPARE (inserted or
    near-miss, depending on the row of A) and for unrelated k, two entries each in a B of 12 columns; the mask is full."""
    n = 12
    nk = c.MAX + hk.SPARE
    t = np.arange(nk)
    rest = _others(K, keys, 200, seed)
    r = np.concatenate([keys[:nk], keys[:nk], rest, rest])
    cc = np.concatenate([t % n, (t * 7 + 3) % n, np.arange(200) % n, (np.arange(200) * 5 + 1) % n])
    B = sp.csr_matrix((np.random.default_rng(seed + 1).uniform(-1, 1, r.size), (r, cc)), shape=(K, n))
    B.sum_duplicates()
    B.sort_indices()
    A = _csr([np.sort(keys[:L]) for L in lens], K, seed + 2)
    M = sp.csr_matrix(np.ones((len(lens), n)))
    return A, B, M


def _triple_case(c, K, keys, lens, seed=21, further=10):
    """Row i of H stores one entry at a column of its own, whose row of Q holds keys[:lens[i]]: T_i has exactly those
    keys.  The further rows of H each store some of the keys up to MAX + 1 (hits for the rows long enough, near-misses for
    the others), keys no row holds and unrelated columns, so S[i, k] depends on each kind of lookup."""
    rng = np.random.default_rng(seed)
    m = len(lens)
    rest = _others(K, keys, m + 40, seed)
    cen, rest = rest[:m], rest[m:]
    pr = np.concatenate([np.full(L, cen[i]) for i, L in enumerate(lens)] + [np.zeros(0, np.int64)]).astype(np.int64)
    pc = np.concatenate([keys[:L] for L in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    P = sp.csr_matrix((rng.uniform(-1, 1, pr.size), (pr, pc)), shape=(K, K))
    Q = (P + P.T).tocsr()
    Q.sort_indices()
    top = c.MAX + 1
    rows = [[cen[i]] for i in range(m)]
    for f in range(further):
        held = np.concatenate([[0] if f % 2 == 0 else [1], [c.MAX - 2, c.MAX - 1, c.MAX][f % 3:], rng.choice(top, size=6, replace=False)])
        never = top + rng.choice(hk.SPARE - 1, size=12, replace=False)
        rows.append(np.unique(np.concatenate([keys[np.unique(held)], keys[never], rng.choice(rest, size=4, replace=False)])))
    H = _csr(rows, K, seed + 1)
    return H, Q


# ------------------------------------------------------------------------------ runs
def _masked_all_modes(ctx, oracle, A, B, M, what):
    W, S = masked_want(oracle, A, B)
    a, b, mk = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B), ctx.csr_from_scipy(M)
    try:
        for exact in (False, True):
            for mode in MODES:
                ctx.tune_masked(mode)
                got = ctx.spgemm_masked_host(a, b, mk, exact=exact)
                try:
                    check_masked_values(got, M, A, B, W, S, exact)
                except AssertionError as e:
                    raise AssertionError(f"{what} mode={mode} exact={exact}: {e}") from None
    finally:
        ctx.tune_masked(0)
        a.close(); b.close(); mk.close()
    return S


def _triple_both(ctx, oracle, H, Q, what):
    n, K = H.shape
    want = oracle.triple(arrays(H), arrays(Q), K, 0)
    U = upper_mask(sp.csr_matrix(np.ones((n, n))))
    h, q, mk = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q), ctx.csr_from_scipy(U)
    try:
        for exact in (False, True):
            try:
                check_triple_sparse(ctx.triple_sparse_host(h, q, exact=exact), H, Q, want, exact)
                check_triple_masked(ctx.triple_sparse_host(h, q, exact=exact, mask=mk), U, want, H, Q, exact)
            except AssertionError as e:
                raise AssertionError(f"{what} exact={exact}: {e}") from None
    finally:
        h.close(); q.close(); mk.close()
    return want


# ------------------------------------------------------------------------------ one row on a class boundary
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("name,kind", KEYCASES)
def test_masked_row_path(ctx, oracle, name, kind, length):
    c, n, keys = _keys(name, kind)
    L = _length(c, length)
    A, B, M = _row_case(c, n, keys, [L])
    S = _masked_all_modes(ctx, oracle, A, B, M, f"{name} {kind} len={L}")
    stored = S[0, M.indices]
    assert stored.any() and (L < 8 or not stored.all()), "the case lost its reached or its unreached mask positions"


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("name,kind", KEYCASES)
def test_masked_dot_path(ctx, oracle, name, kind, length):
    c, K, keys = _keys(name, kind)
    L = _length(c, length)
    A, B, M = _dot_case(c, K, keys, [L])
    S = _masked_all_modes(ctx, oracle, A, B, M, f"{name} {kind} len={L}")
    assert S.any() and (L > 1 or not S.all())


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("name,kind", KEYCASES)
def test_triple_and_masked_triple(ctx, oracle, name, kind, length):
    c, K, keys = _keys(name, kind)
    L = _length(c, length)
    H, Q = _triple_case(c, K, keys, [L])
    assert np.diff(Q.indptr)[H.indices[0]] == L, "T_0 does not have the wanted length"
    want = _triple_both(ctx, oracle, H, Q, f"{name} {kind} len={L}")
    assert np.count_nonzero(want[0]) >= 5


# ------------------------------------------------------------------------------ neighbours in one workgroup
NEIGHBOURS = ["max", "1", "max-1", "0", "max", "max-1", "1"]


@pytest.mark.parametrize("name", ["wave", "wave_one_slot"])
def test_neighbouring_tables_of_one_workgroup(ctx, oracle, name):
    """WaveHash serves four rows per workgroup from adjacent LDS tables: rows of MAX, 1, MAX - 1 and 0 keys side by side
    (fewer than 64 rows, so the class list keeps their order), and a row count that is no multiple of four, so the last
    workgroup has lanes without a row.  (An empty mask row, and a row of S without entries, is in no class list: there
    the count is six.)"""
    c, universe, keys = _keys(name, "window")
    lens = [_length(c, t) for t in NEIGHBOURS]
    assert len(lens) % c.RPB and (len(lens) - 1) % c.RPB
    _masked_all_modes(ctx, oracle, *_row_case(c, universe, keys, lens), f"{name} row layout")
    _masked_all_modes(ctx, oracle, *_dot_case(c, universe, keys, lens), f"{name} dot layout")
    _triple_both(ctx, oracle, *_triple_case(c, universe, keys, lens), f"{name} triple")


# ------------------------------------------------------------------------------ table reuse
class _Lookup:
    """A sparse m x n matrix read like a dense one at [rows, cols]: `fill` where nothing is stored."""

    def __init__(self, n, rows, cols, vals, fill):
        key = rows.astype(np.int64) * n + cols
        o = np.argsort(key, kind="stable")
        self.n, self.key, self.vals, self.fill = n, key[o], np.asarray(vals)[o], fill

    def __getitem__(self, rc):
        key = np.asarray(rc[0], dtype=np.int64) * self.n + np.asarray(rc[1])
        p = np.minimum(np.searchsorted(self.key, key), max(len(self.key) - 1, 0))
        hit = self.key[p] == key
        return np.where(hit, self.vals[p], self.fill)


def _reuse_rows(ctx):
    """More rows than one pass of a WaveHash grid covers: most LDS tables serve a second row."""
    import torch
    n_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    return hk.wave_rows_per_pass(n_cu) + 1026


def _reuse_sets(c, keys, m):
    """Row r holds keys[s : s + L]: L = MAX for even r and 3 for odd r, s = (r // 64) % 61.  The rows that share an LDS
    table have the same r % 64 and (but for one pair in 61) another s, so the earlier row's keys -- all of them looked up by
    the later row -- must read as absent."""
    assert hk.SPARE >= 61
    r = np.arange(m)
    return (r // 64) % 61, np.where(r % 2 == 0, c.MAX, 3)


def test_reused_table_masked_row_path(ctx, oracle):
    c, n, keys = _keys("wave", "window")
    m = _reuse_rows(ctx)
    s, L = _reuse_sets(c, keys, m)
    nk = c.MAX + hk.SPARE
    M = _csr([keys[a:a + b] for a, b in zip(s.tolist(), L.tolist())], n, 31)
    t = np.arange(nk)
    B = _csr([keys[:nk][t % 5 != 4], _others(n, keys, 50, 32)], n, 33)      # row 0: four in five of the keys any row holds
    A = _csr([[0, 1]] * m, 2, 34)
    ptr, idx, val = oracle.sparse(arrays(A), arrays(B), n)
    rows = np.repeat(np.arange(m), np.diff(ptr))
    W, S = _Lookup(n, rows, idx, val, 0.0), _Lookup(n, rows, idx, np.ones(idx.size, dtype=bool), False)
    a, b, mk = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B), ctx.csr_from_scipy(M)
    try:
        ctx.tune_masked(2)
        for exact in (False, True):
            check_masked_values(ctx.spgemm_masked_host(a, b, mk, exact=exact), M, A, B, W, S, exact)
    finally:
        ctx.tune_masked(0)
        a.close(); b.close(); mk.close()


def test_reused_table_masked_dot_path(ctx, oracle):
    c, K, keys = _keys("wave", "window")
    m = _reuse_rows(ctx)
    s, L = _reuse_sets(c, keys, m)
    _, B, _ = _dot_case(c, K, keys, [1])
    A = _csr([keys[a:a + b] for a, b in zip(s.tolist(), L.tolist())], K, 41)
    M = sp.csr_matrix(np.ones((m, B.shape[1])))
    W, S = masked_want(oracle, A, B)
    a, b, mk = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B), ctx.csr_from_scipy(M)
    try:
        ctx.tune_masked(1)
        for exact in (False, True):
            check_masked_values(ctx.spgemm_masked_host(a, b, mk, exact=exact), M, A, B, W, S, exact)
    finally:
        ctx.tune_masked(0)
        a.close(); b.close(); mk.close()


def test_reused_table_triple(ctx, oracle):
    """Row r of H stores one entry whose row of Q holds the keys of _reuse_sets; three further rows of H hold every key
    between them.  The dense checks of check_triple_sparse would cost seconds at this n: the pattern is compared as it is
    there, the values at every stored position, and the oracle's nonzeros are counted instead of scanned."""
    c, K, keys = _keys("wave", "window")
    m = _reuse_rows(ctx)
    s, L = _reuse_sets(c, keys, m)
    rng = np.random.default_rng(51)
    nk = c.MAX + hk.SPARE
    rest = _others(K, keys, m + 20, 52)
    cen, rest = rest[:m], rest[m:]
    pr = np.repeat(cen, L)
    pc = np.concatenate([keys[a:a + b] for a, b in zip(s.tolist(), L.tolist())])
    P = sp.csr_matrix((rng.uniform(-1, 1, pr.size), (pr, pc)), shape=(K, K))
    Q = (P + P.T).tocsr()
    Q.sort_indices()
    further = [np.sort(np.concatenate([keys[0:nk:2], rest[:5]])), np.sort(np.concatenate([keys[1:nk:2], rest[5:10]])),
               np.sort(np.concatenate([keys[0:nk:7], rest[10:]]))]
    H = _csr([[x] for x in cen] + further, K, 53)
    n = H.shape[0]
    want = oracle.triple(arrays(H), arrays(Q), K, 0)
    pp, pi = triple_pattern(H, Q)
    rows = np.repeat(np.arange(n), np.diff(pp))
    w = want[rows, pi]
    assert np.count_nonzero(want) == np.count_nonzero(w), "a nonzero of the oracle is missing from the pattern"
    mag = np.asarray((abs(H) @ abs(Q) @ abs(H).T).tocsr()[rows, pi]).ravel()
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    try:
        for exact in (False, True):
            ptr, idx, val = ctx.triple_sparse_host(h, q, exact=exact)
            assert np.array_equal(ptr, pp) and np.array_equal(idx.astype(np.int64), pi.astype(np.int64)), "pattern"
            if exact:
                assert np.array_equal(val.view(np.int64), w.view(np.int64)), f"values differ bitwise (max rel {rel_err(val, w):.3e})"
            else:
                assert np.all(np.abs(val - w) <= RTOL * mag), f"values: max rel {rel_err(val, w):.3e}"
    finally:
        h.close(); q.close()
