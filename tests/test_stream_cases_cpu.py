"""The late-producer cases of tests/stream_cases.py, proved on the CPU with the references alone: a call that read its
late buffer too early -- the sentinel instead of the final values -- would return a result that differs from the right one
in every stored entry (products, solves) or in at least one entry of every row (builders), and every sentinel is a legal
input of its call."""
import numpy as np
import pytest

import stream_cases
from stream_cases import LATE_NAMES, late_cases, rows_of


def test_the_names_are_the_cases(oracle):
    assert tuple(late_cases(oracle)) == LATE_NAMES


@pytest.mark.parametrize("name", LATE_NAMES)
def test_an_early_read_changes_the_result(oracle, name):
    case = late_cases(oracle)[name]
    assert np.all(np.isfinite(case.sentinel)) and case.sentinel.shape == case.final.shape
    assert not np.any(case.sentinel == case.final)
    right, early = case.reference(case.final), case.reference(case.sentinel)
    if case.kind == "product":
        r, e = np.asarray(right[case.main]), np.asarray(early[case.main])
        assert r.shape == e.shape and r.size > 0
        assert np.all(r != e), f"{name}: {int((r == e).sum())} of {r.size} entries do not see the late buffer"
        if len(right) == 3 and case.main == 2:                      # a CSR: the pattern does not depend on the values
            assert np.array_equal(right[0], early[0]) and np.array_equal(right[1], early[1])
    else:
        a, b = rows_of(*right), rows_of(*early)
        assert len(a) == len(b) == case.final.shape[0]
        same = [r for r in range(len(a)) if a[r] == b[r]]
        assert not same, f"{name}: rows {same[:10]} do not see the late buffer"


def test_sentinel_points_are_legal_inputs(oracle):
    """interp_into's sentinel lies inside the grid (the policy is "error": a point outside would raise), and the
    taper's sentinel coordinates are finite and inside the unit box."""
    import interp_restatement
    cases = late_cases(oracle)
    axes = stream_cases.interp_axes()
    for pts in (cases["interp_into"].sentinel, cases["interp_into"].final):
        assert interp_restatement.outside_count(pts, axes) == 0
    t = cases["taper_into"].sentinel
    assert t.min() >= 0.0 and t.max() <= 1.0


def test_parity_operands_have_the_properties_their_tests_name():
    A, B = stream_cases.product_operands()
    U = stream_cases.unsorted_b()
    assert U.shape == B.shape and U.nnz > B.nnz
    lens = np.diff(U.indptr)
    r = int(np.flatnonzero(lens >= 3)[0])
    row = U.indices[U.indptr[r]:U.indptr[r + 1]]
    assert row[0] == row[-1] and np.any(np.diff(row[:-1]) < 0), "unsorted, with a repeated column"
    H, Q, L, M = stream_cases.triple_operands()
    assert abs(Q - Q.T).nnz == 0 and H.shape == (200, 300) and L.shape == (200, 200) and M.shape == (300, 300)
