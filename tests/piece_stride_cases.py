"""Operands of tests/test_gpu_piece_stride.py and tests/test_piece_stride_cpu.py: B given piece by piece for a tile width,
so that the GPU test knows what every piece is, and the CPU test shows it without a GPU."""
import functools

import numpy as np
import scipy.sparse as sp

from pack12_restatement import MAXGAP, slots_of

ROWS_B, ROWS_A = 300, 64


def _cols(rng, count, width):
    return np.sort(rng.choice(width, count, replace=False)).tolist()


def _padded_piece(rng, width):
    """150 entries, the entry that would take slot 2 of the tenth group comes 2100 columns behind its predecessor: two
    mid-piece pads, n = 152."""
    head = np.cumsum(rng.integers(1, 9, 38)).tolist()                  # 38 entries: slots 0..37, the next would be slot 2 of group 9
    tail = (head[-1] + MAXGAP + 54 + np.cumsum(rng.integers(1, 9, 112))).tolist()
    cols = head + tail
    assert len(cols) == 150 and cols[-1] < width
    s = slots_of(cols)
    assert len(s) == 152 and s[38] is None and s[39] is None and s[40] == cols[38]
    return cols


@functools.lru_cache(maxsize=None)
def pieces(ncols, wc, kind="main"):
    """pieces[t][k]: sorted tile-local columns of (tile t, row k) of B (ROWS_B x ncols, tiles of wc columns).
    main:   130..250 entries per piece (as many as a narrow last tile holds), and by hand: rows 5 and 17 empty, an empty piece
            in the middle tile, one-entry pieces (one of them the last column of B), a piece of exactly 256 entries, the last
            row's last piece ending on the last column; with tiles of 4096 columns and more, a piece with two mid-piece pads.
    skewed: 40..60 entries per piece and one piece of 250: the stride of the longest would be five times the payload."""
    rng = np.random.default_rng(ncols * 7 + wc + len(kind))
    nct = -(-ncols // wc)
    out = []
    for t in range(nct):
        w = min(wc, ncols - t * wc)
        lo, hi = (130, 251) if kind == "main" else (40, 61)
        out.append([_cols(rng, int(rng.integers(min(lo, w // 2), min(hi, w // 2 + 1))), w) for _ in range(ROWS_B)])
    last_w = ncols - (nct - 1) * wc
    if kind == "skewed":
        out[0][7] = _cols(rng, 250, wc)
        return out
    for t in range(nct):
        out[t][5], out[t][17] = [], []
    out[nct // 2][9] = []
    out[0][11] = [int(rng.integers(0, wc))]
    out[nct - 1][12] = [last_w - 1]
    out[min(1, nct - 1)][20] = _cols(rng, 256, wc if nct > 1 else last_w)
    if out[nct - 1][ROWS_B - 1][-1] != last_w - 1:
        out[nct - 1][ROWS_B - 1] = out[nct - 1][ROWS_B - 1][:-1] + [last_w - 1]
    if wc >= 4096:
        out[0][30] = _padded_piece(rng, wc)
    return out


@functools.lru_cache(maxsize=None)
def operand_b(ncols, wc, kind="main", seed=1):
    """B as a canonical scipy CSR, values in [-1, 1) without zeros."""
    P = pieces(ncols, wc, kind)
    rows = [[t * wc + c for t in range(len(P)) for c in P[t][k]] for k in range(ROWS_B)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows])
    val = np.random.default_rng(seed).uniform(-1.0, 1.0, len(idx))
    val[val == 0.0] = 0.5
    B = sp.csr_matrix((val, idx, ptr), shape=(ROWS_B, ncols))
    B.has_sorted_indices = True
    return B


@functools.lru_cache(maxsize=None)
def operand_a(seed=2):
    """A: ROWS_A x ROWS_B, about 40 entries per row; the hand-made rows of B and its last row are used by several rows of A."""
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.0, 1.0, (ROWS_A, ROWS_B)) < 0.13
    for k in (5, 9, 11, 12, 17, 20, 30, 7, ROWS_B - 1):
        D[rng.choice(ROWS_A, 6, replace=False), k] = True
    D[np.arange(ROWS_A), np.arange(ROWS_A) * (ROWS_B // ROWS_A)] = True
    A = sp.csr_matrix(np.where(D, rng.uniform(0.1, 1.0, D.shape), 0.0))
    A.sort_indices()
    return A


def lengths(P):
    return np.array([[len(c) for c in tile] for tile in P], np.int64)
