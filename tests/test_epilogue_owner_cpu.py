"""The ownership rule of the CSR epilogue (tests/epilogue_owner_restatement.py) over random and hand-made run tables:
the owned index ranges partition the row, stay within S-1 entries of their value ranges and never leave the row."""
import numpy as np
import pytest
import scipy.sparse as sp

import epilogue_owner_restatement as own


def _random_table(r, rowlen, nsub, tail0, lead_empty):
    """nsub consecutive sub-runs covering [0, tail0), many of them empty, lead_empty empty ones in front."""
    cuts = np.sort(r.integers(0, tail0 + 1, size=max(nsub - 1, 0))) if nsub else np.zeros(0, np.int64)
    edges = np.concatenate(([0] * (lead_empty + 1), cuts, [tail0])).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("S", own.GRANULES)
def test_up_and_f(S):
    for rs in range(0, 3 * S):
        for x in range(0, 5 * S):
            y = own.up(x, rs, S)
            assert x <= y < x + S and (rs + y) % S == 0
            assert all((rs + z) % S for z in range(x, y))
            for rowlen in (x, x + 1, x + S - 1, x + 3 * S):
                fx = own.f(x, rs, rowlen, S)
                assert fx == (0 if x == 0 else min(y, rowlen))
                assert fx <= rowlen
        # monotone
        for rowlen in (1, S - 1, S, 4 * S + 3):
            fs = [own.f(x, rs, rowlen, S) for x in range(rowlen + 1)]
            assert fs[0] == 0 and fs[-1] == rowlen and all(a <= b for a, b in zip(fs, fs[1:]))


@pytest.mark.parametrize("S", own.GRANULES)
def test_random_tables_partition_the_row(S):
    r = np.random.default_rng(20260 + S)
    n_short = n_all_tail = n_no_tail = n_lead = 0
    for it in range(4000):
        rowlen = int(r.choice([int(r.integers(1, S)), int(r.integers(S, 6 * S)), int(r.integers(6 * S, 400))]))
        tail0 = int(r.choice([0, rowlen, int(r.integers(0, rowlen + 1))]))
        nsub = 0 if tail0 == 0 and r.random() < 0.5 else int(r.integers(1, 40))
        lead = int(r.integers(0, 4)) if nsub else 0
        sub = _random_table(r, rowlen, nsub, tail0, lead)
        rs = int(r.integers(0, 1 << 20)) if it % 3 else int(r.integers(0, 2 * S))
        kept = own.check_row(sub, tail0, rowlen, rs, S)
        assert kept[0][0] == 0 and kept[-1][1] == rowlen
        n_short += rowlen < S
        n_all_tail += tail0 == 0
        n_no_tail += tail0 == rowlen
        n_lead += lead > 0 and tail0 > 0
    assert min(n_short, n_all_tail, n_no_tail, n_lead) > 100          # (the generator reaches every kind)


@pytest.mark.parametrize("S", own.GRANULES)
def test_hand_made_rows(S):
    # sub-runs shorter than a granule own nothing until one crosses a granule boundary
    sub = [(i, i + 1) for i in range(3 * S)]
    for rs in range(S):
        kept = own.check_row(sub, 3 * S, 3 * S + 5, rs, S)
        assert len(kept) <= 5
    # empty sub-runs at position 0: the first non-empty one owns position 0
    ranges = own.owned_ranges([(0, 0), (0, 0), (0, 5), (5, 5), (5, 40)], 40, 50, 3, S)
    assert ranges[0][1] == (0, 0) and ranges[1][1] == (0, 0) and ranges[2][1][0] == 0
    # a row shorter than a granule: one owner for all of it
    for tail0 in (0, 3):
        kept = own.check_row([(0, tail0)] if tail0 else [], tail0, 3, 5, S)
        assert kept == [(0, 3)]


def test_owner_tile():
    assert own.owner_tile(0, 100, False) == 0 and own.owner_tile(250, 100, False) == 0
    assert own.owner_tile(250, 100, True) == 2 and own.owner_tile(99, 100, True) == 0 and own.owner_tile(100, 100, True) == 1


def test_run_table_of_a_small_product():
    """The table builder against the product itself: sub-runs and tail reproduce the first-touch list."""
    r = np.random.default_rng(5)
    A = sp.random(30, 40, density=0.2, format="csr", random_state=r)
    B = sp.random(40, 300, density=0.1, format="csr", random_state=r)
    A.sort_indices(); B.sort_indices()
    nct, wc = own.shared_geometry(300, 64)
    assert (nct, wc) == (5, 60)
    for i in range(30):
        steps = own.row_steps(A, B, i)
        sub, tail0, rowlen = own.run_table(steps, wc, nct, 8)
        flat = [c for s in steps for c in s]
        assert rowlen == len(flat) == len(set(flat)) == (A[i] @ B).nnz
        for r0, r1, t in sub:
            assert all(c // wc == t for c in flat[r0:r1])
        assert all(len(s) < 8 for s in steps[len(sub) // nct:])
        for S in own.GRANULES:
            own.check_row([(a, b) for a, b, _ in sub], tail0, rowlen, 7 * i, S)
