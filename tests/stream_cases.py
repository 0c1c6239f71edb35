"""Operands and late-producer cases of the caller's-stream tests (tests/test_gpu_caller_stream.py), and the references
that tests/test_stream_cases_cpu.py proves them with on the CPU.

A late-producer case names ONE device buffer of values that is still being written when the library call is issued: the
buffer holds `sentinel` until a delayed copy on torch's current stream brings `final`.  Row pointers, column indices and
sizes are never late, and every sentinel is a legal input of its call (finite values, points inside the grid, finite
coordinates), so a call that reads too early returns a different result -- never an index outside an array.
`reference(values)` is the call's result from the given values by the references the sibling tests use (the oracle, the
restatements); the CPU test shows that reference(sentinel) differs from reference(final) in every stored entry of a
product and in at least one entry of every row of a builder, so that an early read cannot go unnoticed."""
import functools

import numpy as np
import scipy.sparse as sp

import interp_restatement
import taper_restatement
from cg_restatement import diag_csr, dominant_diagonal, gaussian_band, local_h, restate_cg, rhs
from helpers import arrays, rand_csr, signed
from sddmm_restatement import entries, restate_exact
from spmm_restatement import restate_spmm

TOL = 1e-8


# ------------------------------------------------------------------------------ operands of the parity tests
@functools.lru_cache(maxsize=None)
def product_operands():
    """A (300 x 400), B (400 x 300), density 0.05, signed values."""
    return signed(rand_csr(300, 400, 0.05, 141), 142), signed(rand_csr(400, 300, 0.05, 143), 144)


@functools.lru_cache(maxsize=None)
def unsorted_b():
    """B of product_operands with every row reversed and, in every row of two entries or more, the first column stored a
    second time at the end: unsorted rows with a repeated column."""
    B = product_operands()[1]
    ptr, idx, val = [0], [], []
    for r in range(B.shape[0]):
        s, e = B.indptr[r], B.indptr[r + 1]
        ci, cv = B.indices[s:e][::-1].tolist(), B.data[s:e][::-1].tolist()
        if len(ci) >= 2:
            ci.append(ci[0]); cv.append(0.375)
        idx += ci; val += cv
        ptr.append(len(idx))
    M = sp.csr_matrix(B.shape, dtype=np.float64)
    M.indptr, M.indices, M.data = np.asarray(ptr, np.int32), np.asarray(idx, np.int32), np.asarray(val, np.float64)
    M.has_sorted_indices = False
    M.has_canonical_format = False
    return M


@functools.lru_cache(maxsize=None)
def triple_operands():
    """H (200 x 300, density 0.03), a symmetric Q (300 x 300), both signed, and the canonical masks L (200 x 200) and
    M (300 x 300)."""
    H = signed(rand_csr(200, 300, 0.03, 145), 146)
    S = signed(rand_csr(300, 300, 0.01, 147), 148)
    Q = (S + S.T).tocsr()
    return H, Q, rand_csr(200, 200, 0.1, 149), rand_csr(300, 300, 0.05, 150)


@functools.lru_cache(maxsize=None)
def solve_system():
    """(H, Q, R) with H 200 x 300 local, Q a Gaussian band and R a dominant diagonal: S + R is positive definite."""
    H, Q = local_h(200, 300, 151), gaussian_band(300, 8)
    return H, Q, diag_csr(dominant_diagonal(H, Q, 152))


@functools.lru_cache(maxsize=None)
def kron_factors():
    """(H, D, E, R): D = tridiag(0.4, 1, 0.4) of order 6, E a Gaussian band of order 50, H 200 x 300."""
    D = sp.diags([np.full(5, 0.4), np.ones(6), np.full(5, 0.4)], [-1, 0, 1], shape=(6, 6), format="csr")
    E = gaussian_band(50, 8)
    H = local_h(200, 300, 153)
    return H, D, E, diag_csr(dominant_diagonal(H, sp.kron(D, E, format="csr"), 154))


def interp_axes():
    return [interp_restatement.nonuniform(17, 161), interp_restatement.nonuniform(9, 162, 0.0, 3.0)]


# ------------------------------------------------------------------------------ late-producer cases
class LateCase:
    """name; final and sentinel (float64 arrays of one shape: the late buffer's contents); kind ("product": every entry of
    array `main` of the result must differ, "builder": an entry of every row must differ); reference(values): the result
    as a tuple of arrays -- (indptr, indices, data) for a CSR; other: an operand of the call that is not late."""

    def __init__(self, name, kind, final, sentinel, reference, main=0, other=None):
        self.name, self.kind, self.reference, self.main, self.other = name, kind, reference, main, other
        self.final, self.sentinel = np.ascontiguousarray(final, np.float64), np.ascontiguousarray(sentinel, np.float64)
        assert self.final.shape == self.sentinel.shape and np.all(np.isfinite(self.sentinel))


@functools.lru_cache(maxsize=None)
def late_operands():
    """A and B with values in (0, 1): every product is positive, so raising every value of B or X raises every stored
    entry of the result.  No row of A or B is empty."""
    A, B = rand_csr(300, 400, 0.05, 171), rand_csr(400, 300, 0.05, 172)
    assert np.diff(A.indptr).min() > 0 and np.diff(B.indptr).min() > 0 and A.data.min() > 0 and B.data.min() > 0
    return A, B


def _with_values(M, values):
    out = M.copy()
    out.data = np.ascontiguousarray(values, np.float64)
    return out


@functools.lru_cache(maxsize=None)
def late_cases(oracle):
    A, B = late_operands()
    rng = np.random.default_rng(173)
    cases = []

    def product(values):
        return oracle.sparse(arrays(A), arrays(_with_values(B, values)), B.shape[1])

    # the values of a borrowed B: csr_from_torch, then the exact product
    cases.append(LateCase("csr_from_torch", "product", B.data, B.data + 1.0, product, main=2))
    # a borrowed B whose payload a first product cached from `sentinel`, rewritten in place: values_changed, then a replay
    cases.append(LateCase("values_changed", "product", rng.uniform(0.0, 1.0, B.nnz), B.data + 1.0, product, main=2))
    for k in (1, 8):
        X = rng.uniform(0.5, 1.5, (A.shape[1], k))
        cases.append(LateCase(f"spmm_into k={k}", "product", X, X + 1.0, lambda x: (restate_spmm(A, x),)))
    rows, cols, _ = entries(A)
    X, Y = rng.uniform(0.5, 1.5, (A.shape[0], 8)), rng.uniform(0.5, 1.5, (A.shape[1], 8))
    cases.append(LateCase("sddmm_into", "product", X, X + 1.0, lambda x: (restate_exact(x, Y, rows, cols),), other=Y))
    P = taper_restatement.uniform(300, 2, 5)
    cases.append(LateCase("taper_into", "builder", P, 0.5 * P + 0.125,
                          lambda p: taper_restatement.restate(p, None, TAPER_CUTOFF, "gaspari_cohn")))
    axes = interp_axes()
    cases.append(LateCase("interp_into", "builder", interp_restatement.inside(300, axes, 174), interp_restatement.inside(300, axes, 175),
                          lambda p: interp_restatement.restate(p, axes, "linear", "error")))
    H, Q, R = solve_system()
    for k in (1, 8):
        D = rhs(H.shape[0], k, 176 + k)

        def solve(d):
            Z, info = restate_cg(H, Q, R, d, TOL)
            return Z, info.iterations, info.status, info.residual_sq, info.rhs_sq

        cases.append(LateCase(f"innovation_solve_into k={k}", "product", D, 1.0 - 2.0 * D[::-1], solve))
    return {c.name: c for c in cases}


TAPER_CUTOFF = 0.2
LATE_NAMES = ("csr_from_torch", "values_changed", "spmm_into k=1", "spmm_into k=8", "sddmm_into", "taper_into", "interp_into",
              "innovation_solve_into k=1", "innovation_solve_into k=8")


def rows_of(ptr, *arrays_):
    """Row r of a CSR as one tuple of bytes: its columns and values in stored order."""
    ptr = np.asarray(ptr, np.int64)
    return [tuple(np.ascontiguousarray(a[ptr[r]:ptr[r + 1]]).tobytes() for a in arrays_) for r in range(ptr.size - 1)]
