"""The contract of smm_cov_eval (include/smm_hip.h) restated in numpy, in the contract's order: every operation is one IEEE
double operation, and exp is taken in np.longdouble and rounded once to double -- so the spherical model is compared bit
for bit and the others within the device exp's error.  Also the patterns and point sets that the CPU and GPU tests share."""
import functools

import numpy as np
import scipy.sparse as sp

import taper_restatement
from sddmm_restatement import raw_csr

MODELS = ("spherical", "exponential", "gaussian", "matern32", "matern52")
SQRT3, SQRT5 = 1.7320508075688772, 2.23606797749979
CV_RUN = 256                       # consecutive entries per wave and run (csrc/smm_cov.hpp)
ULPS = 8                           # 3 (device exp) + 0.5 (this file's rounding of exp) + 4 rounded operations after it


def as_points(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(-1, 1) if x.ndim == 1 else x


def lengths_of(length, dim):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(length, dtype=np.float64), (dim,)))


def exp_rounded(x):
    """exp in extended precision, rounded once to double."""
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, dtype=np.longdouble)).astype(np.float64)


def entries(M):
    """(rows, cols, weights) of every stored entry of a CSR, in stored order."""
    nnz = int(M.indptr[-1])
    return (np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), np.asarray(M.indices[:nnz], dtype=np.int64),
            np.asarray(M.data[:nnz], dtype=np.float64))


def scaled(a, b, rows, cols, lengths):
    """(u, h2, h): u[:, t] = (a[i,t] - b[j,t]) / length[t]; h2 = +0.0; h2 = h2 + u_t * u_t for t = 0 .. dim-1; h = sqrt(h2)."""
    a, b = as_points(a), as_points(b)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.stack([(a[rows, t] - b[cols, t]) / lengths[t] for t in range(a.shape[1])], axis=1)
        h2 = np.zeros(len(rows), dtype=np.float64)
        for t in range(a.shape[1]):
            h2 = h2 + u[:, t] * u[:, t]
        return u, h2, np.sqrt(h2)


def correlation(model, h2, h):
    """(c, g) with g = -dc/dh, in the contract's order."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if model == "spherical":
            c = ((0.5 * h) * h - 1.5) * h + 1.0
            g = 1.5 - 1.5 * (h * h)
            beyond = np.where(h >= 1.0, 0.0, h)                  # (a NaN distance stays a NaN)
            return np.where(h < 1.0, c, beyond), np.where(h < 1.0, g, beyond)
        if model == "exponential":
            e = exp_rounded(-h)
            return e, e
        if model == "gaussian":
            e = exp_rounded(-h2)
            return e, (2.0 * h) * e
        if model == "matern32":
            s = SQRT3 * h
            e = exp_rounded(-s)
            return (1.0 + s) * e, (3.0 * h) * e
        assert model == "matern52"
        s = SQRT5 * h
        e = exp_rounded(-s)
        return ((1.0 + s) + (5.0 / 3.0) * h2) * e, (((5.0 / 3.0) * h) * (1.0 + s)) * e


def restate(a, b, rows, cols, model, length, variance=1.0, wrt=None, weights=None):
    """(val, dval) at the entries (rows, cols); dval None without wrt.  wrt: None, "length" (the common length) or a
    coordinate's index; weights: the pattern's values for SMM_COV_SCALE_BY_PATTERN, else None."""
    a = as_points(a)
    b = a if b is None else as_points(b)
    lengths = lengths_of(length, a.shape[1])
    u, h2, h = scaled(a, b, rows, cols, lengths)
    c, g = correlation(model, h2, h)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        val = variance * c
        dval = None
        if wrt is not None:
            vg = variance * g
            if isinstance(wrt, str):
                assert wrt == "length" and np.all(lengths == lengths[0])
                d = (vg * h) / lengths[0]
            else:
                d = (vg * (u[:, wrt] * u[:, wrt])) / (h * lengths[wrt])
            dval = np.where(h == 0.0, 0.0, d)
        if weights is not None:
            val = val * weights
            dval = None if dval is None else dval * weights
    return val, dval


def dense_covariance(p, model, length, variance=1.0):
    """The full matrix variance * c of one point set (no pattern)."""
    n = as_points(p).shape[0]
    rows, cols = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    return restate(p, None, rows, cols, model, length, variance)[0].reshape(n, n)


def ulps(got, want):
    """|got - want| in units of the spacing of doubles at want; 0 where both are the same bits or both NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want))
    return np.where(same, 0.0, np.where(np.isnan(d), np.inf, d))


# ------------------------------------------------------------------------------ patterns and points
def points(n, dim, seed=0):
    """n points of a box of a few correlation lengths, some of them coincident (distance exactly 0)."""
    p = np.random.default_rng(500 + 10 * dim + seed).random((n, dim)) * 2.5
    if n >= 8:
        p[n // 2] = p[1]
        p[n - 1] = p[3]
    return p


def flat_pattern(nnz, m, n, seed):
    """Exactly nnz entries in an m x n CSR: rows of random lengths (many empty), columns unsorted and repeated."""
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.integers(0, m, nnz))
    ptr = np.searchsorted(rows, np.arange(m + 1))
    return raw_csr(ptr, rng.integers(0, n, nnz), rng.uniform(0.25, 1.5, nnz), (m, n))


@functools.lru_cache(maxsize=None)
def taper_pattern(dim):
    """The Gaspari-Cohn taper of points(300, dim), cutoff 0.9: the pattern and its weights (canonical, symmetric)."""
    return taper_restatement.restate_csr(points(300, dim), None, 0.9, "gaspari_cohn")


@functools.lru_cache(maxsize=None)
def named_patterns():
    """name -> (pattern, n_rows, n_cols): the shapes beside the taper at which the flat split can go wrong."""
    rng = np.random.default_rng(601)
    out = {}
    n = 700                                                        # one row holds every column, beside empty rows
    ptr = np.zeros(41, dtype=np.int64)
    ptr[18:] = n
    ptr[30:] += 1
    ptr[40:] += 1
    out["arrow"] = raw_csr(ptr, np.concatenate([np.arange(n), [5, 699]]), rng.uniform(0.25, 1.5, n + 2), (40, n))
    r = np.repeat(np.arange(5000), 2)
    c = np.stack([rng.integers(0, 2500, 5000), rng.integers(2500, 5000, 5000)], axis=1).ravel()
    out["two_per_row"] = sp.csr_matrix((rng.uniform(0.25, 1.5, 10000), (r, c)), shape=(5000, 5000))
    # an unsorted row with a repeated column, between empty rows
    out["unsorted_repeated"] = raw_csr([0, 0, 6, 6, 8], [7, 2, 7, 0, 9, 2, 4, 4], rng.uniform(0.25, 1.5, 8), (4, 10))
    out["rectangular"] = flat_pattern(900, 37, 300, 602)
    return out
