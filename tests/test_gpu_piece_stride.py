"""B's pack12 pieces at a fixed stride, addressed by (tile, row) behind a 2-byte length table (tune_pack_stride,
tests/piece_stride_restatement.py) in the CSR product's piece walk.

B (tests/piece_stride_cases.py) has 300 rows in three tiles, the last one narrower (the library balances the tiles: by two columns), pieces of 130..256 slots and by hand:
empty rows, an empty piece, one-entry pieces, a piece of 256 slots, the last row's last piece ending on the last column and
(with tiles of 4096 columns) a piece with two mid-piece pads.  Every result against the CPU oracle: indptr and indices bit for
bit, values within 1e-12 of the sum of the magnitudes of the terms (the bound of tests/test_gpu_width_boundaries.py; about
40 products meet per entry, so the rounding bound is 40 * 2^-53 = 4.4e-15 of that sum).  Every context of the suite checks
every plan (SMM_CHECK=1), the strided payload's length table included.  Which payload was built is read from the launch
counts (smm_pack12_len16 builds the length table, smm_pack12_desc the descriptors) and from the operand's device bytes.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import piece_stride_cases as cases
import piece_stride_restatement as ps
from helpers import arrays

pytestmark = pytest.mark.gpu

GEOMS = [(3070, 1024), (12286, 4096)]
KERNELS = ("smm_pack12_fill", "smm_pack12_len16", "smm_pack12_desc", "smm_pack_fill")


@pytest.fixture(autouse=True)
def tiles_only(ctx):
    """Every row of C through the dense LDS tiles (the piece walk), whatever its length."""
    ctx.tune_hash(0, 0)
    ctx.timing(True)
    yield
    ctx.timing(False)
    ctx.tune_hash(256, 2048)
    ctx.tune_shared(20000, 16)
    ctx.tune_pack_stride(1)


def abs_arrays(M):
    p, i, v = arrays(M)
    return p, i, np.abs(v)


def zero_padded(A, row0):
    """A as rows row0 .. of a taller matrix whose other rows are empty (the oracle has no row offset)."""
    return sp.vstack([sp.csr_matrix((row0, A.shape[1])), A]).tocsr()


@functools.lru_cache(maxsize=None)
def reference(ncols, wc, kind="main", seed=1, symmetric=False, row0=0):
    """(A, B, oracle's product, sum of the magnitudes of every entry's terms), computed once per case."""
    from oracle import oracle
    A, B = cases.operand_a(), cases.operand_b(ncols, wc, kind, seed)
    Ap = zero_padded(A, row0)
    want = oracle.sparse(arrays(Ap), arrays(B), ncols, symmetric=symmetric)
    mag = oracle.sparse(abs_arrays(Ap), abs_arrays(B), ncols, symmetric=symmetric)[2]
    lo, hi = int(want[0][row0]), int(want[0][row0 + A.shape[0]])
    return A, B, (want[0][row0:] - lo, want[1][lo:hi], want[2][lo:hi]), mag[lo:hi]


def check(got, want, mag):
    assert np.array_equal(np.asarray(got[0], np.int64), np.asarray(want[0], np.int64)), "indptr differs"
    assert np.array_equal(got[1], want[1]), "indices differ (first-touch order)"
    err = np.abs(got[2] - want[2])
    worst = float(np.max(err / np.maximum(mag, 1e-300))) if len(err) else 0.0
    print(f"largest error {worst:.3e} of the terms' magnitudes")
    assert np.all(err <= 1e-12 * mag), f"values: {worst:.3e} of the terms' magnitudes"


def counts(ctx):
    return {k: ctx.kernel_time(k)[1] for k in KERNELS}


def product(ctx, A, B, wc, mode, symmetric=False, row_offset=0):
    """(result, launch counts, device bytes of B) of A*B on fresh operands with tune_pack_stride(mode)."""
    ctx.tune_shared(wc, 16)
    ctx.tune_pack_stride(mode)
    ctx.timing_reset()
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        bare = b.device_bytes()
        got = ctx.spgemm_host(a, b, symmetric=symmetric, row_offset=row_offset)
        held = b.device_bytes() - bare
    finally:
        a.close(); b.close()
    return got, counts(ctx), held


def assert_payload(ran, strided):
    assert ran["smm_pack12_fill"] == 1 and ran["smm_pack_fill"] == 0
    assert ran["smm_pack12_len16"] == (1 if strided else 0) and ran["smm_pack12_desc"] == (0 if strided else 1)


@pytest.mark.parametrize("ncols,wc", GEOMS)
def test_knob_0_1_2(ctx, ncols, wc):
    """Empty pieces, one-entry pieces, a piece of 256 slots, the last row and the last tile (and, at 4096 columns per tile,
    mid-piece pads) under every mode: one pattern, values within the bound, the strided payload under 1 and 2."""
    A, B, want, mag = reference(ncols, wc)
    ns = ps.piece_ns(cases.pieces(ncols, wc))
    assert want[1].max() == ncols - 1
    got, held = {}, {}
    for mode in (0, 1, 2):
        got[mode], ran, held[mode] = product(ctx, A, B, wc, mode)
        assert_payload(ran, strided=mode > 0)
        check(got[mode], want, mag)
    for mode in (1, 2):
        assert np.array_equal(got[mode][0], got[0][0]) and np.array_equal(got[mode][1], got[0][1])
    # what B holds on top of its CSR arrays differs by the two payloads alone (the tile index and the column stream are shared)
    assert held[1] == held[2] and held[1] - held[0] == ps.device_bytes(ns, True) - ps.device_bytes(ns, False)


def test_symmetric_with_a_row_offset(ctx):
    """Rows 1000..1063 of a symmetric product: the diagonal crosses from tile 0 into tile 1 (1024 columns per tile)."""
    ncols, wc, row0 = 3070, 1024, 1000
    A, B, want, mag = reference(ncols, wc, symmetric=True, row0=row0)
    assert want[1].min() >= row0 and want[1].max() == ncols - 1
    for mode in (0, 1):
        got, ran, _ = product(ctx, A, B, wc, mode, symmetric=True, row_offset=row0)
        assert_payload(ran, strided=mode > 0)
        check(got, want, mag)


def test_replay_after_update_values(ctx):
    """New values of B under a cached plan: the strided payload is re-filled in place, pattern and layout stay."""
    ncols, wc = 12286, 4096
    A, B, want, mag = reference(ncols, wc)
    _, B2, want2, mag2 = reference(ncols, wc, seed=3)
    assert np.array_equal(B.indices, B2.indices) and not np.array_equal(B.data, B2.data)
    ctx.tune_shared(wc, 16)
    ctx.tune_pack_stride(1)
    ctx.timing_reset()
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        plan = ctx.spgemm_plan(a, b)
        first = plan.numeric_host()
        held = b.device_bytes()
        b.update_values(np.ascontiguousarray(B2.data))
        replay = plan.numeric_host()
        plan.check()
        plan.close()
        assert b.device_bytes() == held
    finally:
        a.close(); b.close()
    ran = counts(ctx)
    assert ran["smm_pack12_fill"] == 2 and ran["smm_pack12_len16"] == 1 and ran["smm_pack12_desc"] == 0      # built once, re-filled once
    check(first, want, mag)
    check(replay, want2, mag2)


def test_dense_product_afterwards(ctx, oracle):
    """The dense product keeps the 16-bit payload and its descriptors: both payloads of one operand side by side."""
    ncols, wc = 3070, 1024
    A, B, want, mag = reference(ncols, wc)
    ctx.tune_shared(wc, 16)
    ctx.tune_pack_stride(1)
    ctx.timing_reset()
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        first = ctx.spgemm_host(a, b)
        held = b.device_bytes()
        D = ctx.dense_host(a, b)
        assert b.device_bytes() > held
        again = ctx.spgemm_host(a, b)
    finally:
        a.close(); b.close()
    ran = counts(ctx)
    assert ran["smm_pack12_fill"] == 1 and ran["smm_pack12_len16"] == 1 and ran["smm_pack12_desc"] == 0 and ran["smm_pack_fill"] == 1
    check(first, want, mag)
    check(again, want, mag)
    wantD = oracle.dense(arrays(A), arrays(B), ncols)
    magD = oracle.dense(abs_arrays(A), abs_arrays(B), ncols)
    assert np.all(np.abs(D - wantD) <= 1e-12 * magD)


def test_knob_changed_on_a_live_operand(ctx):
    """The mode changes between two products of the same operand handles: the other payload is built beside the first, a
    plan made before keeps reading its own."""
    ncols, wc = 3070, 1024
    A, B, want, mag = reference(ncols, wc)
    ctx.tune_shared(wc, 16)
    ctx.tune_pack_stride(0)
    ctx.timing_reset()
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    try:
        plan0 = ctx.spgemm_plan(a, b)
        ctx.tune_pack_stride(1)
        plan1 = ctx.spgemm_plan(a, b)
        got1 = plan1.numeric_host()
        got0 = plan0.numeric_host()
        plan0.close(); plan1.close()
    finally:
        a.close(); b.close()
    ran = counts(ctx)
    assert ran["smm_pack12_fill"] == 2 and ran["smm_pack12_len16"] == 1 and ran["smm_pack12_desc"] == 1
    check(got0, want, mag)
    check(got1, want, mag)


def test_skewed_operand_falls_back_under_auto(ctx):
    """One piece of 250 entries among pieces of 40..60: the stride would be five times the payload.  Mode 1 keeps the compact
    payload and its descriptors, mode 2 builds the strided one; the same result either way."""
    ncols, wc = 3070, 1024
    A, B, want, mag = reference(ncols, wc, kind="skewed")
    ns = ps.piece_ns(cases.pieces(ncols, wc, "skewed"))
    held = {}
    for mode in (1, 2):
        got, ran, held[mode] = product(ctx, A, B, wc, mode)
        assert_payload(ran, strided=mode == 2)
        check(got, want, mag)
    assert held[2] - held[1] == ps.device_bytes(ns, True) - ps.device_bytes(ns, False)
