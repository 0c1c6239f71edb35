"""The sparse product on both sides of every column width at which its symbolic phase switches kernels, list widths or
marker structure (tests/width_cases.py lists them and restates the dispatch): default tuning, operands that touch the
first and the last column in every row class, results against the CPU oracle -- indptr and indices bit for bit, values
bit for bit under exact=True and within 1e-12 of the sum of the magnitudes of the terms otherwise (at most 6 products
meet per entry: the rounding bound is 6 * 2^-53 of that sum) -- and the launch counts of the path the case is named for.
tests/test_width_cases_cpu.py shows without a GPU that the operands are what this module takes them for."""
import functools

import numpy as np
import pytest

import width_cases as wc
from helpers import signed

pytestmark = pytest.mark.gpu

PAIR_WIDTHS = (63456, 63457, 65504, 65505, 65534, 65535, 65536)
COUNTED = ("smm_slab_rowcnt", "smm_ccs_fill", "smm_idx16", "smm_symbolic_hash", "smm_symbolic_tiny", "smm_numeric_general")


def _run(ctx, A, B, product=None, **kw):
    """product(a, b) -- by default the sparse product -- of fresh handles (no cached copy of B survives from another
    case), and the launches it made."""
    a = b = None
    ctx.timing(True); ctx.timing_reset()
    try:
        a = ctx.csr_from_scipy(A)
        b = ctx.csr_from_scipy(B)
        got = product(a, b) if product else ctx.spgemm_host(a, b, **kw)
        ran = {name: ctx.kernel_time(name)[1] for name in COUNTED}
    finally:
        ctx.timing(False)
        for h in (a, b):
            if h is not None:
                h.close()
    return got, ran


def _check(got, want, mag, exact):
    assert np.array_equal(np.asarray(got[0], np.int64), np.asarray(want[0], np.int64)), "indptr differs"
    assert np.array_equal(got[1], want[1]), "indices differ (first-touch order)"
    if exact:
        assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64)), "values differ bitwise"
    else:
        err = np.abs(got[2] - want[2])
        assert np.all(err <= 1e-12 * mag), f"values: {float(np.max(err / np.maximum(mag, 1e-300))):.3e} of the terms' magnitudes"


def _check_launches(ran, path):
    for name, expected in wc.expected_launches(path).items():
        assert (ran[name] >= 1) == expected, f"{name}: {ran[name]} launches, path {path.walk} " \
                                             f"(list16 {path.list16}, hash {path.n_hash}, tiny {path.n_tiny}, rest {path.n_rest})"
    # one launch per hash class that exists at this width and has rows
    assert ran["smm_symbolic_hash"] == wc.hash_launches(path), f"hash classes {path.hash_classes}, rows {path.n_hash}"


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("pop", wc.POPULATIONS)
@pytest.mark.parametrize("n", wc.WIDTHS)
def test_width_boundary(ctx, oracle, n, pop, exact):
    A, B = wc.operands(n, pop)
    want = wc.oracle_result(n, pop)
    got, ran = _run(ctx, A, B, exact=exact)
    _check(got, want, None if exact else wc.oracle_magnitude(n, pop), exact)
    _check_launches(ran, wc.expected_path(n, A, B, exact=exact))
    assert ran["smm_numeric_general"] == 0


@functools.lru_cache(maxsize=2)
def _symmetric_case(n, row0):
    from oracle import oracle
    A, B = wc.symmetric_operands(n, row0)
    Ap = wc.zero_padded(A, n, row0)
    want = oracle.sparse(wc.arrays(Ap), wc.arrays(B), n, symmetric=True)
    mag = oracle.sparse(wc.abs_arrays(Ap), wc.abs_arrays(B), n, symmetric=True)[2]
    lo, hi = int(want[0][row0]), int(want[0][row0 + A.shape[0]])
    return A, B, (want[0][row0:row0 + A.shape[0] + 1] - lo, want[1][lo:hi], want[2][lo:hi]), mag[lo:hi]


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("where", ["last-rows", "slab-boundary"])
@pytest.mark.parametrize("n", PAIR_WIDTHS)
def test_symmetric_row_shard(ctx, oracle, n, where, exact):
    """A 256-row shard of the symmetric product whose diagonal runs into the last columns, and one whose diagonal crosses
    the end of the first column slab of this width and mode (31 730 columns at 63 457 by default; two tiles at 63 456, where
    there is one slab), against the slice of the oracle's product of the zero-padded A."""
    ws = wc.slab_geometry(n, exact)[1]
    row0 = n - 256 if where == "last-rows" else ws - 128
    A, B, want, mag = _symmetric_case(n, row0)
    assert len(want[1]) > 0 and want[1].max() == n - 1
    got, ran = _run(ctx, A, B, symmetric=True, row_offset=row0, exact=exact)
    _check(got, want, mag, exact)
    path = wc.expected_path(n, A, B, exact=exact, symmetric=True, row_offset=row0)
    if where == "slab-boundary":
        assert row0 < ws < row0 + 256 and (path.walk == "slab") == (n > wc.CCS_MAX_WS) and path.ws in (None, ws)
    _check_launches(ran, path)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("n", PAIR_WIDTHS)
def test_unsorted_b_with_a_repeated_column(ctx, oracle, n, exact):
    """The safe path: no hash classes, no column stream; rows of C beyond the hash kernels go to smm_numeric_general,
    whose global atomics keep default AND exact mode within the rounding bound (indices bit for bit)."""
    A, B = wc.operands(n, "heavy")
    U = wc.unsorted_with_repeat(B, wc.layout(n, "heavy"))
    want = oracle.sparse(wc.arrays(A), wc.arrays(U), n)
    mag = oracle.sparse(wc.abs_arrays(A), wc.abs_arrays(U), n)[2]
    assert np.any(np.diff(U.indices[:U.indptr[1]]) < 0) and U.nnz == B.nnz + 1         # still as built
    got, ran = _run(ctx, A, U, exact=exact)
    _check(got, want, mag, False)
    _check_launches(ran, wc.expected_path(n, A, U, exact=exact, safe=True))
    assert ran["smm_numeric_general"] >= 1


@pytest.mark.parametrize("n", [65534, 65536])
def test_plan_replay_after_update_values(ctx, oracle, n):
    """One plan on the column-slab walk, run twice: as built, and after both operands got new values."""
    A, B = wc.operands(n, "heavy")
    A2, B2 = signed(A, n + 1), signed(B, n + 2)

    def replay(a, b):
        plan = ctx.spgemm_plan(a, b, exact=True)
        try:
            first = plan.numeric_host()
            a.update_values(A2.data); b.update_values(B2.data)
            return first, plan.numeric_host()
        finally:
            plan.close()

    (first, second), ran = _run(ctx, A, B, product=replay)
    _check(first, wc.oracle_result(n, "heavy"), None, True)
    _check(second, oracle.sparse(wc.arrays(A2), wc.arrays(B2), n), None, True)
    path = wc.expected_path(n, A, B, exact=True)
    assert path.walk == "slab"
    _check_launches(ran, path)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("pop", wc.POPULATIONS)
def test_32bit_lists_at_a_width_that_defaults_to_16bit(ctx, oracle, pop, exact):
    n = 65534
    A, B = wc.operands(n, pop)
    ctx.tune_narrow(False)
    try:
        got, ran = _run(ctx, A, B, exact=exact)
    finally:
        ctx.tune_narrow(True)
    _check(got, wc.oracle_result(n, pop), None if exact else wc.oracle_magnitude(n, pop), exact)
    _check_launches(ran, wc.expected_path(n, A, B, exact=exact, narrow=False))
