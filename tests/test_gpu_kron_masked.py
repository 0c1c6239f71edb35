"""Masked products with the factor form Q = D (x) E, Q never formed (smm_triple_product_sparse_masked_kron,
smm_spgemm_masked_kron[_host], sparse_triple_product(H, KroneckerOperand(D, E), mask=L), masked_matrix_multiply(A,
KroneckerOperand(D, E), mask)).

Contract checked here: each call is its CSR twin on kronecker_product(D, E).  SMM_EXACT: the twin's bits and the bits of
tests/kron_masked_restatement.py.  Default mode: |got - exact| <= 1e-10 (|H| |Q| |H|^T)[i,k] resp. (|A| |Q|)[i,c], the class
of every value (finite, +inf, -inf, NaN) kept, two runs bit-equal.  A value does not depend on the mask or the row range."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import shuffle_rows, upper_mask
from kron_masked_restatement import (aq_bound, band_mask, bits, factor_cases, h_for, positions, rand_rows, random_mask,
                                     restate_masked_aq, restate_masked_triple, same_bits_nan, special_system, taper_like,
                                     triple_bound, unsorted_dup_system)
from kron_restatement import kron_system, tridiag

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
RTOL = 1e-10
MODES = pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])


def _classes(v):
    return np.where(np.isnan(v), 3, np.where(np.isposinf(v), 1, np.where(np.isneginf(v), 2, 0)))


def _assert_values(got, again, twin, want, bound, exact, what):
    """got / again: two runs of the factor form; twin: the CSR form on the explicit operand in the same mode; want: the
    restatement (the exact values); bound: what 1e-10 is relative to."""
    assert np.array_equal(bits(got), bits(again)), f"{what}: two runs differ"
    if exact:
        assert same_bits_nan(got, twin), f"{what}: differs from the CSR twin on kronecker_product(D, E)"
        assert same_bits_nan(got, want), f"{what}: differs from the restatement"
        return
    assert np.array_equal(_classes(got), _classes(want)), f"{what}: default mode changed a value's class"
    fin = np.isfinite(want) & np.isfinite(bound)
    with np.errstate(all="ignore"):
        for name, v in (("the factor form", got), ("the CSR twin", twin)):
            err = np.abs(v[fin] - want[fin])
            assert np.all(err <= RTOL * bound[fin]), f"{what}: {name} is off by {np.max(err - RTOL * bound[fin]):.3e} beyond the bound"


class _Sys:
    """H (or A), the factors and the explicit operand uploaded once on a context."""

    def __init__(self, ctx, H, D, E):
        self.ctx, self.H, self.D, self.E = ctx, H, D, E
        self.h, self.d, self.e = (ctx.csr_from_scipy(M) for M in (H, D, E))
        self.q = ctx.kron_build(self.d, self.e)
        self.handles = [self.h, self.d, self.e, self.q]

    def close(self):
        for hd in self.handles:
            hd.close()

    def triple(self, L, exact, kron=True, full=False, rows=(0, None)):
        mk = self.ctx.csr_from_scipy(L)
        try:
            return self.ctx.triple_sparse_host(self.h, (self.d, self.e) if kron else self.q, full=full, row_begin=rows[0],
                                               row_end=rows[1], exact=exact, mask=mk)
        finally:
            mk.close()

    def aq(self, M, exact, kron=True):
        mk = self.ctx.csr_from_scipy(M)
        try:
            if kron:
                return self.ctx.spgemm_masked_kron_host(self.h, self.d, self.e, mk, exact=exact)
            return self.ctx.spgemm_masked_host(self.h, self.q, mk, exact=exact)
        finally:
            mk.close()

    def check_triple(self, L, exact, what, rows=(0, None)):
        """The upper part on the canonical mask L: pattern, values; returns (indptr, indices, data)."""
        U = upper_mask(L, *rows)
        got, again, twin = self.triple(L, exact, rows=rows), self.triple(L, exact, rows=rows), self.triple(L, exact, kron=False, rows=rows)
        for res in (got, twin):
            assert np.array_equal(res[0], U.indptr.astype(np.int64)) and np.array_equal(res[1], U.indices), f"{what}: pattern is not triu(L)'s"
        want = restate_masked_triple(self.H, self.D, self.E, U, rows[0])
        _assert_values(got[2], again[2], twin[2], want, triple_bound(self.H, self.D, self.E, U, rows[0]), exact, what)
        return got

    def check_aq(self, M, exact, what):
        got, again, twin = self.aq(M, exact), self.aq(M, exact), self.aq(M, exact, kron=False)
        want = restate_masked_aq(self.H, self.D, self.E, M)
        _assert_values(got, again, twin, want, aq_bound(self.H, self.D, self.E, M), exact, what)
        return got


def _full(n, m=None):
    return sp.csr_matrix(np.ones((n, n if m is None else m)))


# ------------------------------------------------------------------------------ 1. what the parent refuses
@MODES
def test_identity_mask_through_the_public_call(ctx, exact):
    """diag(H Q H^T) with Q given by its factors: a ValueError before this entry existed."""
    from sparse_matrix_mult_amd import KroneckerOperand, kronecker_product, set_exact, sparse_triple_product
    H, D, E, _, _ = kron_system()
    L = sp.identity(H.shape[0], format="csr")
    old = set_exact(exact)
    try:
        S = sparse_triple_product(H, KroneckerOperand(D, E), mask=L)
        S2 = sparse_triple_product(H, KroneckerOperand(D, E), mask=L)
        T = sparse_triple_product(H, kronecker_product(D, E), mask=L)
    finally:
        set_exact(old)
    assert sp.isspmatrix_csr(S) and S.shape == T.shape
    assert np.array_equal(S.indptr, T.indptr) and np.array_equal(S.indices, T.indices)
    want = restate_masked_triple(H, D, E, upper_mask(L))
    _assert_values(S.data, S2.data, T.data, want, triple_bound(H, D, E, upper_mask(L)), exact, "diag(S)")


# ------------------------------------------------------------------------------ 2 - 4, 8, 9. factor shapes, row lengths, lookup edges
@pytest.mark.parametrize("name", list(factor_cases()))
@MODES
def test_factor_shapes_row_lengths_and_lookup_edges(ctx, name, exact):
    """Every position of an H whose rows have the lengths 0, 1, 8, 63, 64, 65 and 300 (cut to K) in both orders; for the
    lookup-edge factors two rows hold every column, so every (row, column) of D and of E is searched."""
    D, E = factor_cases()[name]
    K = D.shape[0] * E.shape[0]
    H = h_for(D, E, lens=[K, 0, 1, 8, 65, K]) if name.startswith("edges") else h_for(D, E)
    n = H.shape[0]
    s = _Sys(ctx, H, D, E)
    try:
        up = s.check_triple(_full(n), exact, f"{name}: S")
        F = s.triple(_full(n), exact, full=True)
        Fd = sp.csr_matrix((F[2], F[1], F[0]), shape=(n, n)).toarray()
        Ud = sp.csr_matrix((up[2], up[1], up[0]), shape=(n, n)).toarray()
        assert F[0][-1] == n * n and all(np.all(np.diff(F[1][F[0][i]:F[0][i + 1]]) > 0) for i in range(n))
        assert same_bits_nan(Fd, Fd.T), f"{name}: the full matrix is not symmetric bit for bit"
        assert same_bits_nan(np.triu(Fd), Ud), f"{name}: the full matrix is not the upper part mirrored"
        s.check_aq(random_mask(n, K, 0.3, 5), exact, f"{name}: A Q")
    finally:
        s.close()


@MODES
def test_unsorted_rows_with_repeated_columns(ctx, exact):
    H, D, E = unsorted_dup_system()
    s = _Sys(ctx, H, D, E)
    try:
        s.check_triple(band_mask(H.shape[0], 3), exact, "unsorted_dup: S")
        s.check_aq(random_mask(H.shape[0], H.shape[1], 0.05, 8), exact, "unsorted_dup: A Q")
        Hs = shuffle_rows(h_for(D, E), 4)
        s2 = _Sys(ctx, Hs, D, E)
        try:
            s2.check_triple(_full(Hs.shape[0]), exact, "shuffled rows: S")
        finally:
            s2.close()
    finally:
        s.close()


def test_rectangular_factors_in_the_masked_product(ctx):
    """A (5 x 7 (x) 33 x 29): the mask is m x p'r' and columns divide by r', rows by r."""
    from kron_restatement import canonical_pair
    D, E = canonical_pair()
    A = rand_rows(20, 7 * 33, [0, 1, 8, 65, 231] * 4, 12)
    s = _Sys(ctx, A, D, E)
    try:
        for exact in (True, False):
            s.check_aq(random_mask(20, 5 * 29, 0.4, 13), exact, "rectangular: A Q")
            s.check_aq(_full(20, 5 * 29), exact, "rectangular: A Q, every position")
    finally:
        s.close()


# ------------------------------------------------------------------------------ 5, 7. masks; a value depends on its position only
@functools.lru_cache(maxsize=None)
def _mask_system():
    D, E = factor_cases()["tridiag5_taper33"]
    lens = [8] * 48
    for i in (5, 20, 41):
        lens[i] = 0                                         # rows of H without entries: positions no product reaches
    lens[9], lens[30] = 1, 70
    return rand_rows(48, 165, lens, 31), D, E


def _masks(n):
    rnd = random_mask(n, n, 0.15, 32)
    holes = rnd.tolil()
    holes[3] = 0
    holes[17] = 0
    holes[n - 1] = 0
    holes = holes.tocsr()
    holes.sort_indices()
    return {"identity": sp.identity(n, format="csr"), "band": band_mask(n, 4), "random": rnd, "rows_without_entries": holes,
            "lower_only": sp.tril(_full(n), -1, format="csr")}


@MODES
def test_masks_and_independence_of_the_mask_and_the_row_range(ctx, exact):
    H, D, E = _mask_system()
    n = H.shape[0]
    s = _Sys(ctx, H, D, E)
    try:
        whole = s.check_triple(_full(n), exact, "every position")
        W = sp.csr_matrix((whole[2], whole[1], whole[0]), shape=(n, n))
        at = {(i, k): v for i, k, v in zip(*positions(W), bits(whole[2]).tolist())}
        zero_rows = [5, 20, 41]
        for i in zero_rows:
            assert at[(i, i)] == 0 and at[(min(i, 7), max(i, 7))] == 0, "a position no product reaches is not +0.0"
        for kind, L in _masks(n).items():
            res = s.check_triple(L, exact, f"mask {kind}")
            rows, cols = positions(upper_mask(L))
            assert [at[p] for p in zip(rows.tolist(), cols.tolist())] == bits(res[2]).tolist(), f"mask {kind}: a value depends on the mask"
            if kind == "lower_only":
                assert res[0][-1] == 0, "entries below the diagonal are ignored"
        for r0, r1 in ((0, n), (0, 7), (7, n), (n, n)):
            res = s.check_triple(band_mask(n, 4), exact, f"rows [{r0}, {r1})", rows=(r0, r1))
            rows, cols = positions(upper_mask(band_mask(n, 4), r0, r1))
            assert [at[p] for p in zip((rows + r0).tolist(), cols.tolist())] == bits(res[2]).tolist(), "a value depends on the row range"
        # A Q: the same value under two masks
        every = s.check_aq(_full(n, 165), exact, "A Q: every position").reshape(n, 165)
        M = random_mask(n, 165, 0.1, 33)
        part = s.check_aq(M, exact, "A Q: random mask")
        assert np.array_equal(bits(part), bits(every[positions(M)])), "A Q: a value depends on the mask"
        assert np.array_equal(bits(every[zero_rows]), np.zeros((3, 165), np.int64))
    finally:
        s.close()


# ------------------------------------------------------------------------------ 6. special values
@pytest.mark.parametrize("kind", ["unreached", "reached", "negzero"])
@MODES
def test_special_values(ctx, kind, exact):
    H, D, E = special_system(kind)
    n, K = H.shape
    s = _Sys(ctx, H, D, E)
    try:
        S = s.check_triple(_full(n), exact, f"{kind}: S")[2]
        C = s.check_aq(_full(n, K), exact, f"{kind}: A Q")
        if kind == "unreached":
            # the inf of row 3 and the NaN of row 6 sit where row AND column t = 2 of D hold nothing: A Q never meets them,
            # and S meets them only as (unstored T = +0.0) * H[k, .] in the columns k = 3 and k = 6 of the recipe's second sum
            assert np.all(np.isfinite(C)), "a value of H reached A Q through a pair the factors do not store"
            rows, cols = positions(upper_mask(_full(n)))
            assert np.all(np.isfinite(S[~np.isin(cols, [3, 6])]))
        elif kind == "reached":
            assert np.isinf(C).any() and np.isnan(C).any() and np.isnan(S).any()
        else:
            assert np.all(C == 0) and np.signbit(C).any() and not np.signbit(C).all(), "both zeros occur"
    finally:
        s.close()


# ------------------------------------------------------------------------------ 10. refusals and failed allocations
def test_refusals_leave_nothing_allocated(ctx):
    from sparse_matrix_mult_amd.engine import SmmError
    H, D, E = _mask_system()
    n = H.shape[0]
    s = _Sys(ctx, H, D, E)
    extra = {k: ctx.csr_from_scipy(v) for k, v in dict(
        d_unsorted=shuffle_rows(D, 1), e_unsorted=shuffle_rows(E, 2), d_rect=sp.csr_matrix(np.ones((5, 4))), e_small=taper_like(32, 2),
        big=sp.identity(46341, format="csr"), ident=sp.identity(n, format="csr"), wrong=sp.identity(n + 1, format="csr"),
        m_unsorted=shuffle_rows(band_mask(n, 3), 3), am=random_mask(n, 165, 0.1, 4), am_wrong=random_mask(n, 164, 0.1, 4),
        am_unsorted=shuffle_rows(random_mask(n, 165, 0.2, 5), 6)).items()}
    x = extra
    try:
        ctx.release_pool()
        live = ctx.live_bytes()
        triple = [((x["d_unsorted"], s.e), x["ident"], "sum_duplicates"), ((s.d, x["e_unsorted"]), x["ident"], "sum_duplicates"),
                  ((x["d_rect"], s.e), x["ident"], "square"), ((s.d, x["e_small"]), x["ident"], "columns"),
                  ((x["big"], x["big"]), x["ident"], "2\\^31"), ((s.d, s.e), x["wrong"], "mask"), ((s.d, s.e), x["m_unsorted"], "canonical")]
        for q, mk, text in triple:
            with pytest.raises(SmmError, match=text) as err:
                ctx.triple_sparse_host(s.h, q, mask=mk, exact=True)
            assert err.value.code == -2 and ctx.live_bytes() == live and ctx.pool_bytes() == 0, text
        with pytest.raises(ValueError, match="mask"):
            ctx.triple_sparse_host(s.h, (s.d, s.e), exact=True)
        masked = [(x["d_unsorted"], s.e, x["am"], "sum_duplicates"), (s.d, x["e_small"], x["am"], "columns"), (x["big"], x["big"], x["am"], "2\\^31"),
                  (s.d, s.e, x["am_wrong"], "mask"), (s.d, s.e, x["am_unsorted"], "canonical")]
        for d, e, mk, text in masked:
            with pytest.raises(SmmError, match=text) as err:
                ctx.spgemm_masked_kron_host(s.h, d, e, mk, exact=True)
            assert err.value.code == -2 and ctx.live_bytes() == live and ctx.pool_bytes() == 0, text
        s.check_triple(band_mask(n, 2), True, "after the refusals")
    finally:
        for hd in extra.values():
            hd.close()
        s.close()


@pytest.mark.parametrize("which", ["triple", "triple_full", "aq"])
def test_a_failed_allocation_leaves_no_pool_block_handed_out(which):
    """Each device allocation of a call failed in turn (hard) until the call succeeds: every failure is SMM_ERR_ALLOC with
    nothing handed out, and the call that succeeds is exact."""
    from sparse_matrix_mult_amd.engine import Context, SmmError
    c = Context(0)
    H, D, E = _mask_system()
    n = H.shape[0]
    s = _Sys(c, H, D, E)
    L, M = band_mask(n, 3), random_mask(n, 165, 0.1, 7)
    mk = c.csr_from_scipy(M if which == "aq" else L)
    try:
        if which == "aq":
            call, want = (lambda: c.spgemm_masked_kron_host(s.h, s.d, s.e, mk, exact=True)), restate_masked_aq(H, D, E, M)
        else:
            call = lambda: c.triple_sparse_host(s.h, (s.d, s.e), mask=mk, exact=True, full=which == "triple_full")[2]
            want = restate_masked_triple(H, D, E, upper_mask(L))
        call()                                              # (validates the operands: their flags are cached on the handles)
        failures = 0
        for nth in range(1, 65):
            c.release_pool()
            c.inject_alloc_failure(nth, hard=True)
            try:
                got = call()
            except SmmError as e:
                assert e.code == -3, f"allocation {nth}: {e}"
                assert c.live_bytes() == 0, f"allocation {nth}: {c.live_bytes()} bytes still handed out"
                failures += 1
                continue
            finally:
                c.inject_alloc_failure(0)
            if which == "triple_full":
                assert len(got) == 2 * len(want) - n
            else:
                assert same_bits_nan(got, want), f"after {failures} failed allocations"
            assert c.live_bytes() == 0
            break
        else:
            pytest.fail("never succeeded")
        assert failures >= (2 if which == "aq" else 5), f"only {failures} allocations failed"
    finally:
        mk.close()
        s.close()
        c.close()


# ------------------------------------------------------------------------------ 11. pinned operands, device results, a caller's stream
def test_pinned_operands_device_results_and_non_canonical_factors(ctx):
    import torch

    from sparse_matrix_mult_amd import (DeviceCSRResult, KroneckerOperand, masked_matrix_multiply, pin_operand, set_exact,
                                        set_result_device, sparse_triple_product)
    H, D, E = _mask_system()
    n = H.shape[0]
    L, M = band_mask(n, 3), random_mask(n, 165, 0.1, 9)
    want_s, want_c = restate_masked_triple(H, D, E, upper_mask(L)), restate_masked_aq(H, D, E, M)
    old = set_exact(True)
    try:
        S = sparse_triple_product(H, KroneckerOperand(D, E), mask=L)
        C = masked_matrix_multiply(H, KroneckerOperand(D, E), M)
        assert same_bits_nan(S.data, want_s) and same_bits_nan(C.data, want_c)
        assert np.array_equal(C.indptr, M.indptr) and np.array_equal(C.indices, M.indices)
        F = sparse_triple_product(H, KroneckerOperand(D, E), mask=L, compute_full_matrix=True).toarray()
        assert same_bits_nan(F, F.T) and same_bits_nan(np.triu(F), S.toarray())
        # scipy factors that are not canonical are canonicalised on a host copy; pinned ones are refused
        Du, Eu = shuffle_rows(D, 5), shuffle_rows(E, 6)
        assert not Du.has_canonical_format
        S2 = sparse_triple_product(H, KroneckerOperand(Du, Eu), mask=L)
        assert same_bits_nan(S2.data, want_s) and not Du.has_sorted_indices, "the caller's factor was modified"
        pins = [pin_operand(X) for X in (H, D, E, upper_mask(L), M, Du, shuffle_rows(L, 7))]
        ph, pd, pe, pl, pm, pdu, plu = pins
        try:
            with pytest.raises(ValueError, match="canonical"):
                sparse_triple_product(ph, KroneckerOperand(pdu, pe), mask=pl)
            with pytest.raises(ValueError, match="canonical"):
                masked_matrix_multiply(ph, KroneckerOperand(pdu, pe), pm)
            with pytest.raises(ValueError, match="canonical"):
                sparse_triple_product(ph, KroneckerOperand(pd, pe), mask=plu)
            Sp = sparse_triple_product(ph, KroneckerOperand(pd, pe), mask=pl)
            Cp = masked_matrix_multiply(ph, KroneckerOperand(pd, pe), pm)
            assert same_bits_nan(Sp.data, want_s) and same_bits_nan(Cp.data, want_c)
            oldd = set_result_device(True)
            try:
                for h, q, l, m in ((H, KroneckerOperand(D, E), L, M), (ph, KroneckerOperand(pd, pe), pl, pm)):
                    Sd = sparse_triple_product(h, q, mask=l)
                    Cd = masked_matrix_multiply(h, q, m)
                    assert isinstance(Sd, DeviceCSRResult) and isinstance(Cd, DeviceCSRResult) and Sd.indptr.dtype == torch.int64
                    assert np.array_equal(Sd.indices.cpu().numpy(), S.indices) and np.array_equal(Cd.indices.cpu().numpy(), M.indices)
                    assert same_bits_nan(Sd.data.cpu().numpy(), want_s) and same_bits_nan(Cd.data.cpu().numpy(), want_c)
            finally:
                set_result_device(oldd)
        finally:
            for p in pins:
                p.unpin()
    finally:
        set_exact(old)


def test_on_a_callers_stream_with_a_pending_write_to_the_operands(ctx):
    """A context on torch's side stream; H's and D's values are borrowed torch tensors that still hold NaN when the calls are
    issued: the copy of the real values is queued on that stream behind a long chain of kernels.  Stream order alone must
    make the calls read the real values."""
    import torch

    from sparse_matrix_mult_amd.engine import Context
    H, D, E = _mask_system()
    n = H.shape[0]
    L, M = band_mask(n, 3), random_mask(n, 165, 0.1, 9)
    want_s, want_c = restate_masked_triple(H, D, E, upper_mask(L)), restate_masked_aq(H, D, E, M)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    c = Context(0, side.cuda_stream)
    handles = []
    try:
        with torch.cuda.stream(side):
            def borrowed(X):
                ptr, idx = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (X.indptr, X.indices))
                val = torch.full((X.nnz,), float("nan"), dtype=torch.float64, device=dev)
                handles.append(c.csr_from_torch(X.shape[0], X.shape[1], ptr, idx, val))
                return handles[-1], val, torch.from_numpy(np.ascontiguousarray(X.data)).to(dev)
            (h, hv, hfinal), (d, dv, dfinal) = borrowed(H), borrowed(D)
            e, lm, mm = (c.csr_from_scipy(X) for X in (E, upper_mask(L), M))
            handles += [e, lm, mm]
            out = torch.empty(M.nnz, dtype=torch.float64, device=dev)
            big = torch.zeros(1 << 24, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            for _ in range(40):
                big.add_(1.0)
            hv.copy_(hfinal)
            dv.copy_(dfinal)
            ptr, idx, val = c.triple_sparse_torch(h, (d, e), mask=lm, exact=True)
            c.spgemm_masked_kron_into(h, d, e, mm, out.data_ptr(), exact=True)
            assert same_bits_nan(val.cpu().numpy(), want_s), "the triple product read H or D before the pending write"
            assert np.array_equal(idx.cpu().numpy(), upper_mask(L).indices)
            assert same_bits_nan(out.cpu().numpy(), want_c), "A Q read A or D before the pending write"
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        for hd in handles:
            hd.close()
        c.close()
