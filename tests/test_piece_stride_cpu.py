"""The strided pack12 layout and its rule (tests/piece_stride_restatement.py) on small operands, and the operands of
tests/test_gpu_piece_stride.py (tests/piece_stride_cases.py) shown to be what that module takes them for."""
import numpy as np
import pytest

import piece_stride_cases as cases
import piece_stride_restatement as ps
from pack12_restatement import ALIGN, decode, slots_of, units12


def small_operand(longest, rows=12, nct=3, wc=700, seed=0, short=(130, 200)):
    """pieces[t][k] and values[t][k]: `short` entries per piece, piece (1, 3) empty, piece (2, 5) of `longest` entries."""
    rng = np.random.default_rng(seed)
    P = [[np.sort(rng.choice(wc, int(rng.integers(*short)), replace=False)).tolist() for _ in range(rows)] for _ in range(nct)]
    P[1][3] = []
    P[2][5] = np.sort(rng.choice(wc, longest, replace=False)).tolist()
    V = [[(1.0 + np.arange(len(c)) / 64.0 + t).tolist() for c in tile] for t, tile in enumerate(P)]
    return P, V


@pytest.mark.parametrize("longest", [201, 255, 256])
def test_layout(longest):
    wc = 700
    P, V = small_operand(longest)
    nct, rows = len(P), len(P[0])
    ns = ps.piece_ns(P)
    pay, len16, stride = ps.build(P, V, wc)
    assert ns.max() == longest and stride == units12(longest) and stride % ALIGN == 0
    assert 8 * stride >= 8 * longest + 6 * ((longest + 3) // 4) > 8 * (stride - ALIGN)      # the longest piece, rounded up to 128 bytes
    assert len16.dtype == np.uint16 and len(len16) == nct * rows and len16[1 * rows + 3] == 0 and len16[2 * rows + 5] == longest
    assert len(pay) == 8 * (stride * nct * rows + ps.SLACK)
    for t in range(nct):
        for k in range(rows):
            n = int(len16[t * rows + k])
            at = 8 * ps.first_unit(t, k, rows, stride)
            assert at % 128 == 0 and n == len(slots_of(P[t][k]))
            g = (n + 3) // 4
            v = pay[at:at + 8 * n].view(np.float64)
            D = pay[at + 8 * n:at + 8 * n + 4 * g].view(np.uint32)
            H = pay[at + 8 * n + 4 * g:at + 8 * n + 6 * g].view(np.uint16)
            assert decode(D, H, wc)[:n] == P[t][k] and v.tolist() == V[t][k]        # (these pieces have no pads: slot = entry)
            used = 8 * n + 6 * g
            assert np.all(pay[at + used:at + 8 * stride] == 0xA5)                   # nothing behind the piece is written
            # ... and what the walk loads stays inside the piece's own stride (the last piece: inside the slack)
            assert ps.walk_extent(n) <= max(8 * stride, 32) and at + ps.walk_extent(n) <= len(pay)


def test_the_slack_covers_a_clamped_length():
    """The walk clamps a length to 256 slots whatever the table holds; from the last piece's start that reaches 2432 bytes."""
    assert max(ps.walk_extent(n) for n in range(0, 257)) == ps.walk_extent(256) == 8 * ps.SLACK == 2432
    assert units12(256) == ps.SLACK                         # a piece of 256 slots fills exactly that


def test_rule():
    P, _ = small_operand(256, short=(170, 250))
    ns, L = ps.piece_ns(P), cases.lengths(P)
    total, compact = ps.stride_of(ns) * ns.size, ps.compact_units(ns)
    assert compact < total <= 1.5 * compact
    assert ps.strided_rule(ns, L, 1) and ps.strided_rule(ns, L, 2) and not ps.strided_rule(ns, L, 0)
    assert not ps.strided_rule(ns, L, 2, pack12_mode=0)
    # one very long row among short ones: pack12 still applies, the stride would multiply the payload
    P, _ = small_operand(250, short=(40, 60))
    ns, L = ps.piece_ns(P), cases.lengths(P)
    assert ps.pack12_rule(ns, L) and 2 * ps.stride_of(ns) * ns.size > 3 * ps.compact_units(ns)
    assert not ps.strided_rule(ns, L, 1) and ps.strided_rule(ns, L, 2)
    # no piece above 128 slots, or one above 256: no pack12, so no stride under any mode
    for longest in (100, 257):
        P, _ = small_operand(longest, short=(40, 60))
        ns, L = ps.piece_ns(P), cases.lengths(P)
        assert not any(ps.strided_rule(ns, L, m, pack12_mode=2) for m in (0, 1, 2))
    # the payload must stay below 2^31 units: 304 units x 7.1e6 pieces does not
    ns = np.full((3, 2_400_000), 256, np.int64)
    assert ps.stride_of(ns) * ns.size + ps.SLACK >= ps.INT32_MAX and not ps.strided_rule(ns, ns, 2, pack12_mode=2)
    ns = np.full((3, 2_000_000), 256, np.int64)
    assert ps.strided_rule(ns, ns, 1, pack12_mode=2)


@pytest.mark.parametrize("ncols,wc", [(3070, 1024), (12286, 4096)])
def test_gpu_operands(ncols, wc):
    P = cases.pieces(ncols, wc)
    ns, L = ps.piece_ns(P), cases.lengths(P)
    nct = len(P)
    # three tiles, the last one narrower: the library balances the tiles, wc = ceil(ncols / ceil(ncols / lds_cols))
    assert nct == 3 == -(-ncols // wc) and -(-ncols // nct) == wc and 0 < ncols - 2 * wc < wc
    assert ns.max() == 256 and ns[min(1, nct - 1), 20] == 256 and L.max() == 256
    assert np.all(ns[:, 5] == 0) and np.all(ns[:, 17] == 0) and ns[1, 9] == 0 and ns[0, 11] == 1 and ns[2, 12] == 1
    assert P[2][12] == [ncols - 2 * wc - 1] and P[2][cases.ROWS_B - 1][-1] == ncols - 2 * wc - 1
    body = ns[:2][(ns[:2] > 1)]
    assert body.min() >= 129 and body.max() <= 256
    if wc >= 4096:
        assert ns[0, 30] == 152 and L[0, 30] == 150                                 # two mid-piece pads
    else:
        assert np.array_equal(ns, L)
    assert ps.pack12_rule(ns, L) and ps.strided_rule(ns, L, 1)
    ratio = ps.stride_of(ns) * ns.size / ps.compact_units(ns)
    assert 1.0 < ratio <= 1.5, ratio
    B, A = cases.operand_b(ncols, wc), cases.operand_a()
    assert B.shape == (cases.ROWS_B, ncols) and B.has_canonical_format and B.nnz == L.sum() and A.shape == (cases.ROWS_A, cases.ROWS_B)
    assert B[cases.ROWS_B - 1, ncols - 1] != 0.0 and A[:, cases.ROWS_B - 1].nnz >= 6
    for k in (5, 9, 11, 12, 17, 20, 30):
        assert A[:, k].nnz >= 6


def test_gpu_skewed_operand():
    P = cases.pieces(3070, 1024, "skewed")
    ns, L = ps.piece_ns(P), cases.lengths(P)
    assert ns.max() == 250 and ps.pack12_rule(ns, L)
    assert not ps.strided_rule(ns, L, 1) and ps.strided_rule(ns, L, 2)
    assert ps.stride_of(ns) * ns.size > 4 * ps.compact_units(ns)
