"""The pack12 layout (tests/pack12_restatement.py) against a brute-force list of (slot -> column or sink, value)."""
import numpy as np
import pytest

from pack12_restatement import ALIGN, MAXGAP, PAD, SINK, decode, eligible, encode, fill_by_windows, slots_of, units12, units16

GAPS = [1, 2046, 2047, 2048, 4093]


def brute(cols, vals):
    """Slot by slot, by the rule's words: [(column or SINK, value or None for a trailing pad)]."""
    out = []
    for c, v in zip(cols, vals):
        in_group = len(out) % 4
        if in_group:
            last_real = [x for x in out[len(out) - in_group:] if x[0] != SINK][-1][0]
            if c - last_real > 2046:
                out += [(SINK, 0.0)] * (4 - in_group)
        out.append((int(c), float(v)))
    n = len(out)
    out += [(SINK, None)] * (-n % 4)
    return out, n


def check(cols, wc):
    cols = np.asarray(cols, np.int64)
    assert np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < wc
    vals = 1.0 + np.arange(len(cols)) / 1024.0
    want, n = brute(cols, vals)
    v, D, H = encode(cols, vals, wc)
    g = (n + 3) // 4
    assert len(v) == n == len(slots_of(cols)) and len(D) == len(H) == g and D.dtype == np.uint32 and H.dtype == np.uint16
    got = decode(D, H, wc)
    assert got == [w[0] for w in want]
    for s in range(n):
        assert v[s] == want[s][1] and (want[s][0] != SINK or not np.signbit(v[s]))
    assert all(w[1] is None for w in want[n:])
    assert units12(n) % ALIGN == 0 and units12(n) * 8 >= 8 * n + 6 * g
    assert units12(n) * 8 - (8 * n + 6 * g) < 8 * ALIGN + 8
    return n, want


@pytest.mark.parametrize("length", [1, 3, 4, 5, 127, 128, 129, 255, 256])
def test_piece_lengths(length):
    rng = np.random.default_rng(length)
    cols = np.sort(rng.choice(16667, length, replace=False))
    # (a random piece of a 16 667-column tile: mean gap >= 65, a gap above 2046 is possible only for the short ones)
    n, want = check(cols, 16667)
    assert n >= length and (n == length) == all(w[0] != SINK for w in want[:n])
    assert eligible(n) == (128 < n <= 256)


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("slot", [0, 1, 2, 3])
def test_gaps_in_every_slot(gap, slot):
    """The gap sits in front of the entry that would take `slot` of the third group (entries 2 apart otherwise)."""
    before = 8 + slot
    cols = list(range(0, 2 * before, 2))
    cols += [cols[-1] + gap + 2 * k for k in range(12)]
    n, want = check(cols, 16667)
    if slot == 0 or gap <= MAXGAP:
        assert n == len(cols) and all(w[0] != SINK for w in want[:n])          # a group's slot 0 is absolute: no pad
    else:
        assert n == len(cols) + (4 - slot)
        assert [w[0] for w in want[before:before + 4 - slot]] == [SINK] * (4 - slot)
        assert want[before + 4 - slot][0] == cols[before]


@pytest.mark.parametrize("wc", [16667, 32767])
def test_first_and_last_column(wc):
    for cols in ([0], [wc - 1], [0, wc - 1], [0, 1, 2, 3, wc - 1], list(range(0, 300, 2)) + [wc - 1],
                 [0] + list(range(wc - 140, wc))):
        check(cols, wc)
    v, D, H = encode([wc - 1], [2.5], wc)
    assert int(D[0]) & 0x7fff == wc - 1 and decode(D, H, wc) == [wc - 1, SINK, SINK, SINK]
    assert (int(D[0]) >> 15) & 0x7ff == PAD and int(H[0]) >> 5 == PAD


def test_pads_push_a_piece_past_256_slots():
    """254 entries; gaps of 2047 in front of the entries that would take slot 1 of two groups: 2 x 3 pads, n = 260."""
    cols, c = [], 0
    for k in range(254):
        c += 2047 if k in (9, 102) else 3
        cols.append(c)
    n, want = check(cols, 32767)
    assert len(cols) == 254 and n == 260 and not eligible(n)
    assert eligible(len(slots_of(range(0, 508, 2))))                # the same length without pads is


def test_byte_model_of_the_workload():
    """Piece lengths of a 50 000-column operand at density 0.01 in three tiles: Binomial(16 667, 0.01).  Pads: 0.99^2046
    per in-group gap, about 0.02 in the whole operand, so n = length here.  Bytes per piece step by 128, their spread
    is about 100 B: two million draws put the mean within 0.1 B."""
    L = np.random.default_rng(12).binomial(16667, 0.01, 2_000_000).astype(np.int64)
    b16, b12 = 8.0 * np.mean(units16(L)), 8.0 * np.mean(units12(L))
    assert abs(b16 - 1729.6) <= 0.5 and abs(b12 - 1646.7) <= 0.5, (b16, b12)


@pytest.mark.parametrize("seed", range(40))
def test_the_fill_by_windows_builds_the_same_piece(seed):
    """The device fill works a piece in windows of 64 entries (a wave).  Pieces of 1 .. 256 entries with long gaps at random
    places, so that groups start in every lane of a window, the last three included, and windows end inside padded groups."""
    rng = np.random.default_rng(1000 + seed)
    length = int(rng.integers(1, 257)) if seed % 4 else (60, 61, 64, 65, 67, 128, 129, 253, 256, 1)[seed // 4]
    gaps = rng.integers(1, 4, length)
    gaps[rng.choice(length, min(length, (0, 3, 14)[seed % 3]), replace=False)] = MAXGAP + 1      # 14 x 2047 + 256 x 3 < 32 767
    cols = np.cumsum(gaps) - gaps[0]
    vals = 1.0 + np.arange(length) / 1024.0
    wc = int(cols[-1]) + 1
    assert wc <= 32767
    want = encode(cols, vals, wc)
    got = fill_by_windows(cols, vals, wc)
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and np.array_equal(w, g)
