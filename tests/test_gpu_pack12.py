"""B's packed payload with 1.5-byte columns ("pack12", tests/pack12_restatement.py) in the CSR product's piece walk.

Every case runs with tune_pack(0) (16-bit columns) and tune_pack(2) (pack12 wherever the four-entries-per-lane walk
applies): each run against the oracle the way tests/test_gpu_parity.py does (indptr and indices bit-exact, values to 1e-10
relative), the two runs against each other (indptr and indices equal), and once more on values that are multiples of 2^-8,
where no sum rounds and the two runs must agree bit for bit.  smm_pack12_fill must have run in the second run.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import special_values as sv
from helpers import arrays, assert_csr_equal, rand_csr
from pack12_restatement import MAXGAP, eligible, slots_of

pytestmark = pytest.mark.gpu

WC = 20000                                                  # the default tile width: one tile for 20 000 columns


@pytest.fixture(autouse=True)
def tiles_only(ctx):
    """Every row of C through the dense LDS tiles (the piece walk), whatever its length."""
    ctx.tune_hash(0, 0)
    ctx.timing(True)
    yield
    ctx.timing(False)
    ctx.tune_hash(256, 2048)
    ctx.tune_shared(20000, 16)
    ctx.tune_pack(1)


def product(ctx, A, B, mode, symmetric=False):
    """(result, launches of smm_pack12_fill) of A*B with tune_pack(mode) on fresh operands."""
    ctx.tune_pack(mode)
    ctx.timing_reset()
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        got = ctx.spgemm_host(a, b, symmetric=symmetric)
    finally:
        a.close(); b.close()
    return got, ctx.kernel_time("smm_pack12_fill")[1]


def both_formats(ctx, oracle, A, B, symmetric=False, pack12=True):
    n = B.shape[1]
    want = oracle.sparse(arrays(A), arrays(B), n, symmetric=symmetric)
    g16, f16 = product(ctx, A, B, 0, symmetric)
    g12, f12 = product(ctx, A, B, 2, symmetric)
    assert f16 == 0 and (f12 > 0) == pack12
    assert_csr_equal(g16, want, values="tol", rtol=1e-10)
    assert_csr_equal(g12, want, values="tol", rtol=1e-10)
    assert np.array_equal(g16[0], g12[0]) and np.array_equal(g16[1], g12[1])
    Aq, Bq = sv.quantised(A), sv.quantised(B)               # multiples of 2^-8: every sum exact in any order
    q16, _ = product(ctx, Aq, Bq, 0, symmetric)
    q12, f12 = product(ctx, Aq, Bq, 2, symmetric)
    assert (f12 > 0) == pack12
    assert_csr_equal(q12, q16, values="bits")
    assert_csr_equal(q12, oracle.sparse(arrays(Aq), arrays(Bq), n, symmetric=symmetric), values="bits")


# ------------------------------------------------------------------------------ hand-written rows of B
def row_with(length, specials, first0, last, seed):
    """Sorted columns of one piece: `length` entries 1..40 apart; specials = [(slot in group, gap)]: the entry that would
    take that slot of some group comes `gap` columns behind its predecessor; first0: the first column is 0; last: the
    last column is WC - 1."""
    rng = np.random.default_rng(seed)
    cols = [0 if first0 else int(rng.integers(1, 30))]
    todo = list(specials)
    while len(cols) < length - (1 if last else 0):
        slot = len(slots_of(cols)) % 4
        if todo and slot == todo[0][0] and len(cols) > 8:
            cols.append(cols[-1] + todo.pop(0)[1])
        else:
            cols.append(cols[-1] + int(rng.integers(1, 41)))
    assert not todo and cols[-1] < WC - 1
    if last:
        cols.append(WC - 1)
    return cols


def csr_of(rows, ncols, seed):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows if len(r)] or [np.zeros(0, np.int32)])
    val = np.random.default_rng(seed).uniform(0.0, 1.0, len(idx))
    M = sp.csr_matrix((val, idx, ptr), shape=(len(rows), ncols))
    M.has_sorted_indices = True
    return M


def handwritten_b():
    """24 rows x 20 000 columns, 130-250 entries per piece; gaps of 2046, 2047 and 2048 in slots 1, 2, 3 and at a group
    start; first column 0, last column WC - 1; row 7 is empty."""
    combos = [(s, g) for g in (MAXGAP, MAXGAP + 1, MAXGAP + 2) for s in (1, 2, 3, 0)]
    rows = []
    for r in range(24):
        if r == 7:
            rows.append([])
            continue
        specials = [combos[r % 12]] if r < 12 else [combos[(r + k) % 12] for k in (0, 5, 7)]
        rows.append(row_with(130 + (r * 37) % 115, specials, first0=r % 2 == 0, last=r % 3 == 0, seed=100 + r))
    ns = [len(slots_of(r)) for r in rows]
    assert all(eligible(n) for n in ns if n) and any(n > len(r) for n, r in zip(ns, rows))      # pieces of 129..256 slots, some with pads
    assert min(len(r) for r in rows if r) >= 130 and max(len(r) for r in rows) <= 250
    return csr_of(rows, WC, 5)


def test_a_pieces_without_pads(ctx, oracle):
    """Two tiles of 2048 columns, pieces of about 184 entries."""
    ctx.tune_shared(2048, 16)
    A, B = rand_csr(32, 48, 0.5, 11), rand_csr(48, 4096, 0.09, 12)
    both_formats(ctx, oracle, A, B)


def test_b_handwritten_gaps_at_the_default_tile_width(ctx, oracle):
    both_formats(ctx, oracle, rand_csr(16, 24, 0.6, 21), handwritten_b())


def test_c_pads_past_256_slots_fall_back(ctx, oracle):
    """254 entries whose pads make n = 260: the operand keeps the 16-bit payload, whatever tune_pack says."""
    cols, c = [], 0
    for k in range(254):
        c += MAXGAP + 1 if k in (9, 102) else 3
        cols.append(c)
    assert len(slots_of(cols)) == 260
    rows = [cols] + [row_with(150 + 9 * r, [], r % 2 == 0, False, 200 + r) for r in range(7)]
    both_formats(ctx, oracle, rand_csr(12, 8, 0.7, 31), csr_of(rows, WC, 6), pack12=False)


def test_d_symmetric(ctx, oracle):
    """The upper triangle: `c >= thresh ? c : sink` behind the decode.  Two tiles of 1024 columns."""
    ctx.tune_shared(1024, 16)
    A, B = rand_csr(2048, 48, 0.06, 41), rand_csr(48, 2048, 0.18, 42)
    both_formats(ctx, oracle, A, B, symmetric=True)


@pytest.mark.parametrize("mode", [0, 2])
def test_e_update_values_and_replay(ctx, oracle, mode):
    """New values of B under a cached plan: the replay equals a fresh product (exact sums: bit for bit)."""
    A, B = sv.quantised(rand_csr(16, 24, 0.6, 51)), sv.quantised(handwritten_b())
    B2 = B.copy()
    B2.data = np.maximum(np.round(np.random.default_rng(52).uniform(0.0, 1.0, B.nnz) * 256.0), 1.0) / 256.0
    ctx.tune_pack(mode)
    ctx.timing_reset()
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        plan = ctx.spgemm_plan(a, b)
        first = plan.numeric_host()
        b.update_values(np.ascontiguousarray(B2.data))
        replay = plan.numeric_host()
        plan.close()
    finally:
        a.close(); b.close()
    assert ctx.kernel_time("smm_pack12_fill")[1] == (2 if mode else 0)          # built once, re-filled once
    assert_csr_equal(first, oracle.sparse(arrays(A), arrays(B), WC), values="bits")
    fresh, _ = product(ctx, A, B2, mode)
    assert_csr_equal(replay, fresh, values="bits")
    assert_csr_equal(replay, oracle.sparse(arrays(A), arrays(B2), WC), values="bits")


def padded_b():
    """16 rows whose last entry, column WC - 1, comes more than 2046 columns behind its predecessor in the same group:
    the slot in front of it is a mid-piece pad.  The plants of special_values.plant sit on a row's last column."""
    rows = []
    for r in range(16):
        cols = row_with(140 + 6 * r, [], r % 2 == 0, False, 300 + r)
        while len(cols) % 4 == 0:
            cols.append(cols[-1] + 3)
        cols.append(WC - 1)
        assert slots_of(cols)[-2] is None and eligible(len(slots_of(cols)))
        rows.append(cols)
    return csr_of(rows, WC, 7)


@pytest.mark.parametrize("name", ["inf_reached_by_some", "inf_minus_inf", "stored_zero_times_inf", "unstored_zero_times_inf",
                                  "nan_in_left", "inf_in_left"])
def test_f_special_values_next_to_a_pad(ctx, name):
    """inf, NaN and a stored zero in the entry behind a mid-piece pad, and inf / NaN in the entry of A that multiplies the
    pad's +0.0: that product is a NaN and must reach the sink accumulator only.  Exact sums, so the plain loop over the
    stored entries gives the bits (any NaN for a NaN)."""
    A, B = sv.bounded(rand_csr(12, 16, 0.5, 61), 62), sv.bounded(padded_b(), 63)
    if name == "inf_in_left":
        i, r1, _ = sv._pick_pair(A, B)
        A = sv.with_entries(A, [(i, r1, np.inf)])
    else:
        A, B, _ = sv.plant(A, B, name)
    A, B = sv.quantised(A), sv.quantised(B)
    want = sv.plain_sparse(A, B)
    if name != "unstored_zero_times_inf":
        assert not np.all(np.isfinite(want[2]))
    for mode in (0, 2):
        got, fills = product(ctx, A, B, mode)
        assert (fills > 0) == (mode == 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert sv.same_bits_nan(got[2], want[2]), f"tune_pack({mode})"
