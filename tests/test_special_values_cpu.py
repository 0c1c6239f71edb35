"""The cases of tests/special_values.py checked on the CPU, so that tests/test_gpu_special_values.py compares against a
reference that is known to be right and on inputs that are known to be fair.

Oracle against the plain loop: on every case, oracle.sparse / oracle.dense (plain and symmetric), oracle.triple (upper,
full, and a row range) equal the plain numpy loops bit for bit, NaN matching NaN.  No difference was found, so the GPU
tests compare with the plain loops.  One thing to know about the triple product: the reference keeps T = H*Q as a dense
row, so a stored entry of H multiplies +0.0 where T holds nothing, and an inf or NaN in row k of H makes column k of the
result non-finite (0.0 * inf); the library's sparse and masked triple products promise the same ("a miss reads +0.0").

Order independence: every default-mode case gives every output the same class when each row's terms are added backwards.

Honesty conditions: each case produces every class it claims, at most 25 % of its outputs are non-finite, every stored
zero has its finite twin, and every forced dispatch configuration finds a row of each class it is meant to reach.
triple_product_apply runs on a windowed H and a band Q so that the rule holds for k = 1 as well."""
import numpy as np
import pytest

import special_values as sv
from helpers import arrays
from special_values import DEFAULT_PLANTS, FINITE, PLANTS, cls, same_bits_nan

AB_SHAPES = ["small", "tiny", "large"]
TRIPLE = [(s, n, "Q") for s in ("n60", "n300", "window") for n in PLANTS if n != "edge_lower"] + \
         [(s, n, "H") for s in ("n60", "n300", "window") for n in ("inf_reached_by_some", "nan_in_left", "stored_zero_times_inf")] + \
         [("n1100", n, w) for n, w in sv.BIG_TRIPLE_CASES]


def _claims(name, symmetric=False):
    if name == "edge_lower":
        return {"finite"} if symmetric else {"finite", "inf"}
    return PLANTS[name]


# an inf, a NaN or a zero stored in row k of H itself: T's +0.0 and infinities meet it in stage 2
H_CLAIMS = {"inf_reached_by_some": {"finite", "inf", "nan"}, "nan_in_left": {"finite", "nan"},
            "stored_zero_times_inf": {"finite", "nan"}}


def _check_classes(values, name, symmetric=False, limit=0.25, claims=None):
    c = cls(values)
    for claim in claims or _claims(name, symmetric):
        assert sv.present(c, claim), f"{name}: no output of class {claim}"
    assert np.mean(c != FINITE) <= limit, f"{name}: {np.mean(c != FINITE):.1%} of the outputs are not finite"
    if name == "subnormal":
        v = np.abs(np.ravel(values))
        assert np.any((v > 0) & (v < np.finfo(np.float64).tiny)) and np.any(v >= np.finfo(np.float64).tiny)


@pytest.mark.parametrize("name", list(PLANTS))
@pytest.mark.parametrize("shape", AB_SHAPES)
def test_sparse_and_dense_oracle_equals_the_plain_loop(oracle, shape, name):
    A, B, note = sv.ab_case(shape, name)
    n = B.shape[1]
    for symmetric in (False, True):
        wp, wi, wv = sv.plain_sparse(A, B, symmetric)
        op, oi, ov = oracle.sparse(arrays(A), arrays(B), n, symmetric=symmetric)
        assert np.array_equal(op, wp) and np.array_equal(oi, wi) and same_bits_nan(ov, wv)
        _check_classes(wv, name, symmetric)
        D = sv.plain_dense(A, B, symmetric)
        assert same_bits_nan(oracle.dense(arrays(A), arrays(B), n, symmetric=symmetric), D)
        assert same_bits_nan(oracle.dense(arrays(A), arrays(B), n, symmetric=symmetric, row_begin=5, row_end=77), D[5:77])
        # the dense output holds the sparse one (a first product stored as it is, or added to +0.0: the same but for -0.0)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(wp))
        assert np.array_equal(cls(D[rows, wi]), cls(wv)) and np.all((D[rows, wi] == wv) | np.isnan(wv))
        assert not sv.bits(D)[sv.term_counts(A, B) == 0].any()
        if name in DEFAULT_PLANTS:                          # the same terms added backwards: the same classes
            R = sv.plain_dense(sv.reverse_rows(A), sv.reverse_rows(B), symmetric)
            assert np.array_equal(cls(R), cls(D)), f"{shape} {name}: the class of an output depends on the order"
    if name == "edge_lower":                                # below the diagonal: no trace in the upper-triangle variants
        assert np.all(np.isfinite(sv.plain_sparse(A, B, True)[2])) and not np.all(np.isfinite(sv.plain_sparse(A, B, False)[2]))


@pytest.mark.parametrize("shape", AB_SHAPES)
def test_the_stored_zero_has_its_finite_twin(shape):
    A1, B1, n1 = sv.ab_case(shape, "stored_zero_times_inf")
    A0, B0, n0 = sv.ab_case(shape, "unstored_zero_times_inf")
    assert n1 == n0 and A1.nnz == A0.nnz + 1 and same_bits_nan(B1.data, B0.data)
    i, c = n1["row"], n1["col"]
    assert np.isnan(sv.plain_dense(A1, B1)[i, c]) and np.isfinite(sv.plain_dense(A0, B0)[i, c])
    assert sv.term_counts(A0, B0)[i, c] > 0, "the twin's position must stay in the pattern"


@pytest.mark.parametrize("name", list(PLANTS))
@pytest.mark.parametrize("shape", AB_SHAPES)
def test_every_forced_configuration_reaches_its_row_classes(shape, name):
    A, B, _ = sv.ab_case(shape, name)
    for symmetric in (False, True):
        ptr = sv.plain_sparse(A, B, symmetric)[0]
        for config, thresholds in sv.HASH_CONFIGS.items():
            have = set(sv.row_classes(A, B, ptr, thresholds))
            need = sv.REQUIRED_CLASSES[(shape, thresholds)]
            assert need <= have, f"{shape} {name} sym={symmetric} {config}: no row of class {sorted(need - have)}"


@pytest.mark.parametrize("shape,name,where", TRIPLE)
def test_triple_oracle_equals_the_plain_loop(oracle, shape, name, where):
    H, Q, _ = sv.triple_case(shape, name, where)
    K, n = Q.shape[0], H.shape[0]
    with np.errstate(all="ignore"):
        S = sv._stage2(sv._t_rows(H, Q), H)
        R = sv._stage2(sv._t_rows(sv.reverse_rows(H), sv.reverse_rows(Q)), sv.reverse_rows(H)) if name in DEFAULT_PLANTS else None
    for full in (0, 1):
        want = sv.triple_from_sums(S, full)
        assert same_bits_nan(oracle.triple(arrays(H), arrays(Q), K, full), want)
        seen = want if full else want[np.triu_indices(n)]
        _check_classes(seen, name, claims=H_CLAIMS[name] if where == "H" else None)
        if R is not None:
            assert np.array_equal(cls(sv.triple_from_sums(R, full)), cls(want)), f"{shape} {name}: the class depends on the order"
    part = oracle.triple(arrays(H), arrays(Q), K, 0, 21, min(203, n))
    assert same_bits_nan(part[21:min(203, n)], sv.triple_from_sums(S, 0)[21:min(203, n)])


@pytest.mark.parametrize("shape", ["n60", "n300", "window"])
def test_triple_stored_zero_has_its_finite_twin(shape):
    H1, Q1, n1 = sv.triple_case(shape, "stored_zero_times_inf")
    H0, Q0, _ = sv.triple_case(shape, "unstored_zero_times_inf")
    assert H1.nnz == H0.nnz + 1
    i = n1["row"]
    assert np.any(np.isnan(sv.plain_triple(H1, Q1)[i])) and not np.any(np.isnan(sv.plain_triple(H0, Q0)))


@pytest.mark.parametrize("name", list(PLANTS))
def test_masked_cases(name):
    A, B, M = sv.masked_case(name)
    assert M.has_canonical_format and 0.09 < sv.random_mask(*M.shape).nnz / np.prod(M.shape) < 0.13
    want = sv.plain_masked(A, B, M)
    _check_classes(want, name)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    assert not sv.bits(want)[sv.term_counts(A, B)[rows, M.indices] == 0].any()


SPMM_CLAIMS = {"inf_reached_by_some": {"finite", "inf"}, "inf_minus_inf": {"finite", "nan"}, "unstored_zero_times_inf": {"finite", "inf"},
               "edge_first_row": {"finite", "inf"}, "edge_last_row": {"finite", "inf"}, "stored_zero_times_inf": {"finite", "nan"},
               "nan_in_left": {"finite", "nan"}, "edge_nan_first": {"finite", "nan"}, "edge_nan_last": {"finite", "nan"},
               "subnormal": {"finite"}, "huge": {"finite", "inf"}}


@pytest.mark.parametrize("name", sv.SPMM_PLANTS)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("k", [1, 5, 65])
def test_sparse_times_dense_cases(k, transpose, name):
    A, X, col = sv.spmm_case(name, k, transpose)
    Y = sv.plain_spmm(A, X, transpose)
    c = cls(Y)
    for claim in SPMM_CLAIMS[name]:
        assert sv.present(c, claim), f"{name}: no output of class {claim}"
    assert np.mean(c != FINITE) <= 0.25
    if name in sv.SPMM_X_PLANTS and k > 1:
        assert np.all(np.delete(c, col, axis=1) == FINITE)
    if name == "stored_zero_times_inf":
        A0, X0, _ = sv.spmm_case("unstored_zero_times_inf", k, transpose)
        assert np.array_equal(X0, X) and A0.nnz == A.nnz - 1
        Y0 = sv.plain_spmm(A0, X0, transpose)
        assert np.sum(np.isnan(Y)) == 1 and np.all(np.isfinite(Y0[np.isnan(Y)]))
    if name != "huge":                                      # every default-mode case
        L = sv.transpose_csr(A) if transpose else A         # the rows of op(A) walked backwards
        assert np.array_equal(cls(sv.plain_spmm(sv.reverse_rows(L), X)), c)


@pytest.mark.parametrize("name", sv.SPMM_PLANTS)
@pytest.mark.parametrize("k", [1, 5, 65])
def test_triple_product_apply_cases(k, name):
    """H (Q (H^T X)) on the windowed H and the band Q: every claimed class is there, at most 25 % of Y is not finite for
    every k (k = 1 included: the plant reaches only the rows of H next to it), a plant in one column of X leaves the
    other columns finite, and each of the three loops run backwards gives the same classes."""
    H, X, col = sv.spmm_case(name, k, True, apply=True)
    Q = sv.apply_q(H.shape[1])
    Z = sv.plain_apply(H, Q, X)
    c = cls(Z)
    for claim in SPMM_CLAIMS[name]:
        assert sv.present(c, claim), f"{name}: no output of class {claim}"
    assert np.mean(c != FINITE) <= 0.25, f"{name} k={k}: {np.mean(c != FINITE):.1%} of Y is not finite"
    if name in sv.SPMM_X_PLANTS and k > 1:
        assert np.all(np.delete(c, col, axis=1) == FINITE)
    if name != "huge":
        rev = sv.reverse_rows
        with np.errstate(all="ignore"):
            back = sv.restate_spmm(rev(H), sv.restate_spmm(rev(Q), sv.restate_spmm(rev(sv.transpose_csr(H)), X)))
        assert np.array_equal(cls(back), c)


@pytest.mark.parametrize("name", DEFAULT_PLANTS)
def test_unsorted_b_with_a_repeated_column_keeps_its_classes_in_any_order(name):
    """The general-path case of the GPU tests (B shuffled, a column stored twice): same classes with the terms backwards."""
    A, B, _ = sv.ab_case("small", name)
    B = sv.unsorted_with_repeat(B, 31)
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    assert len(set(zip(rows.tolist(), B.indices.tolist()))) < B.nnz, "no column is stored twice"
    for symmetric in (False, True):
        D = sv.plain_dense(A, B, symmetric)
        R = sv.plain_dense(sv.reverse_rows(A), sv.reverse_rows(B), symmetric)
        assert np.array_equal(cls(R), cls(D))


def _exact_in_any_order(values, granule):
    """Every finite value is a multiple of the granule and fits 53 bits of it: sums of such terms do not round."""
    v = np.ravel(values)
    v = v[np.isfinite(v)] / granule
    return bool(np.all(v == np.round(v)) and np.all(np.abs(v) < 2.0 ** 52))


@pytest.mark.parametrize("name", DEFAULT_PLANTS)
@pytest.mark.parametrize("shape", AB_SHAPES)
def test_exact_sum_inputs_of_the_two_runs_tests(shape, name):
    """The same pattern and the same non-finite plants as the case they narrow; every product is a multiple of one
    granule, so is every partial sum in any order, and the loop run backwards gives the same bits."""
    A, B = sv.exact_ab_case(shape, name)
    A0, B0 = sv.ab_case(shape, name)[:2] if name != "subnormal" else sv.ab_base(shape)
    for M, M0 in ((A, A0), (B, B0)):
        assert np.array_equal(M.indptr, M0.indptr) and np.array_equal(M.indices, M0.indices)
        assert np.array_equal(cls(M.data), cls(M0.data)) and np.array_equal(M.data == 0, M0.data == 0)
    sub = name == "subnormal"
    granule = (sv.GRANULE * sv.SUBNORMAL_SCALE[False]) ** 2 if sub else sv.GRANULE ** 2
    mag = sv.magnitudes(A, B)
    assert _exact_in_any_order(mag, granule), "a sum of magnitudes (the largest any partial sum can get) rounds"
    for symmetric in (False, True):
        D = sv.plain_dense(A, B, symmetric)
        R = sv.plain_dense(sv.reverse_rows(A), sv.reverse_rows(B), symmetric)
        assert same_bits_nan(D, R) and _exact_in_any_order(D, granule)
        if sub:
            assert np.all(np.abs(D) < np.finfo(np.float64).tiny) and np.any(D != 0)
        else:
            assert np.array_equal(cls(D), cls(sv.plain_dense(A0, B0, symmetric)))


@pytest.mark.parametrize("shape,name,where", [c for c in TRIPLE if c[1] != "huge"])
def test_exact_sum_inputs_of_the_two_runs_tests_triple(shape, name, where):
    H, Q = sv.exact_triple_case(shape, name, where)
    sub = name == "subnormal"
    s = sv.SUBNORMAL_SCALE[True] if sub else 1.0
    granule = (sv.GRANULE * s) ** 3
    assert granule >= 2.0 ** -1074
    assert _exact_in_any_order(sv.triple_magnitudes(H, Q, 1), granule)
    with np.errstate(all="ignore"):
        S = sv._stage2(sv._t_rows(H, Q), H)
        R = sv._stage2(sv._t_rows(sv.reverse_rows(H), sv.reverse_rows(Q)), sv.reverse_rows(H))
    assert same_bits_nan(S, R) and _exact_in_any_order(S, granule)
    if sub:
        assert np.all(np.abs(S) < np.finfo(np.float64).tiny) and np.any(S != 0)


def test_transpose_operand_and_reference():
    A = sv.transpose_operand()
    tp, ti, tv = sv.plain_transpose(A)
    C = A.tocsc()
    assert np.array_equal(tp, C.indptr) and np.array_equal(ti, C.indices) and np.array_equal(sv.bits(tv), sv.bits(C.data))
    v = A.data
    tiny = np.finfo(np.float64).tiny
    assert np.isnan(v).sum() == 4 and len(set(sv.bits(v[np.isnan(v)]).tolist())) == 4         # four NaN payloads
    assert np.any(v == np.inf) and np.any(v == -np.inf) and np.any((v != 0) & (np.abs(v) < tiny))
    assert np.any((v == 0) & np.signbit(v)) and np.any((v == 0) & ~np.signbit(v))
    assert A.shape == (257, 130)


def test_classifier():
    assert cls([1.0, -0.0, 5e-324, np.inf, -np.inf, np.nan]).tolist() == [0, 0, 0, sv.PINF, sv.NINF, sv.NAN]
