"""The contract of smm_variogram (include/smm_hip.h) restated in numpy, in the contract's order: every operation is one IEEE
double operation, every slot adds its entries one after another, and the tree adds adjacent pairs.  np.sum / np.add.reduce
are never used on floats: they add pairwise in an order of numpy's own.  SMM_VG_SLOTS and SMM_VG_RUN come from the header
(through _lib, which parses it).  Also the independent evaluation (np.searchsorted + math.fsum) and the inputs that the CPU
and GPU tests share."""
import functools
import math

import numpy as np

from cov_restatement import entries, flat_pattern, points, taper_pattern  # noqa: F401  (shared with the tests)
from sparse_matrix_mult_amd._lib import SMM_VG_MAX_BINS, SMM_VG_RUN, SMM_VG_SLOTS
from taper_restatement import as_points

T, RUN, MAX_BINS = SMM_VG_SLOTS, SMM_VG_RUN, SMM_VG_MAX_BINS
WAVES = T // 64


def per_entry(a, y, rows, cols, edges, upper=True):
    """(h, s, b, take) of every entry: the distance, the squared increment, the bin by comparisons alone, and whether the
    entry takes part."""
    a, y = as_points(a), as_points(y)
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = np.zeros(len(rows), dtype=np.float64)
        for t in range(a.shape[1]):
            df = a[rows, t] - a[cols, t]
            d2 = d2 + df * df
        h = np.sqrt(d2)
        s = np.zeros(len(rows), dtype=np.float64)
        for c in range(y.shape[1]):
            dv = y[rows, c] - y[cols, c]
            s = s + dv * dv
        b = np.zeros(len(rows), dtype=np.int64)
        for q in range(1, nb + 1):
            b += edges[q] <= h
        take = (edges[0] <= h) & (h < edges[nb])
    if upper:
        take &= np.asarray(cols) > np.asarray(rows)
    return h, s, b, take


def slots(nnz):
    e = np.arange(nnz, dtype=np.int64)
    return ((e // RUN) % WAVES) * 64 + e % 64


def ordered_slot_sums(key, value, size):
    """out[key] = +0.0, then out[key] = out[key] + value for the entries in the order given, entry by entry: round r adds the
    r-th entry of every key at once."""
    order = np.argsort(key, kind="stable")
    key, value = key[order], value[order]
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    start = np.maximum.accumulate(np.where(first, np.arange(key.size), 0))
    pos = np.arange(key.size) - start                              # the entry's place among those of its key
    out = np.zeros(size, dtype=np.float64)
    by_round = np.argsort(pos, kind="stable")
    bounds = np.searchsorted(pos[by_round], np.arange(int(pos.max()) + 2 if key.size else 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(bounds) - 1):
            sel = by_round[bounds[r]:bounds[r + 1]]
            out[key[sel]] = out[key[sel]] + value[sel]              # (the keys of one round are distinct)
    return out


def tree(p):
    """p: (T, nb).  p[t] = p[t] + p[t + g] for every t that is a multiple of 2 g, g = 1, 2, 4, ..., T / 2; the result p[0]."""
    p = p.copy()
    g = 1
    with np.errstate(invalid="ignore", over="ignore"):
        while g < p.shape[0]:
            p[0::2 * g] += p[g::2 * g]
            g *= 2
    return p[0].copy()


def restate(a, y, rows, cols, edges, upper=True):
    """(count int64, sum_h, sum_sq) per bin, bit for bit what the contract gives."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    h, s, b, take = per_entry(a, y, rows, cols, edges, upper)
    sel = np.flatnonzero(take)                                      # ascending e
    key = slots(len(rows))[sel] * nb + b[sel]
    count = np.bincount(b[sel], minlength=nb).astype(np.int64)
    sum_h = tree(ordered_slot_sums(key, h[sel], T * nb).reshape(T, nb))
    sum_sq = tree(ordered_slot_sums(key, s[sel], T * nb).reshape(T, nb))
    return count, sum_h, sum_sq


def independent(a, y, rows, cols, edges, upper=True):
    """The same three arrays by another route: the per-entry terms in the contract's order, bins by np.searchsorted, sums
    by math.fsum (the correctly rounded sum of the terms)."""
    a, y = as_points(a), as_points(y)
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    d2 = np.zeros(len(rows))
    for t in range(a.shape[1]):
        d2 = d2 + (a[rows, t] - a[cols, t]) * (a[rows, t] - a[cols, t])
    h = np.sqrt(d2)
    s = np.zeros(len(rows))
    for c in range(y.shape[1]):
        s = s + (y[rows, c] - y[cols, c]) * (y[rows, c] - y[cols, c])
    b = np.searchsorted(edges, h, side="right") - 1
    keep = (b >= 0) & (b < nb) & ((cols > rows) if upper else True)
    count = np.zeros(nb, dtype=np.int64)
    sum_h, sum_sq = np.zeros(nb), np.zeros(nb)
    for q in range(nb):
        m = keep & (b == q)
        count[q] = int(m.sum())
        sum_h[q], sum_sq[q] = math.fsum(h[m].tolist()), math.fsum(s[m].tolist())
    return count, sum_h, sum_sq


def bound(nnz):
    """Relative distance of a contract sum from math.fsum of the same terms.  Every term is >= 0, so an add's rounding error
    is at most 2^-53 of the partial sum it produces, which is at most the total: a term passes through at most
    ceil(nnz / T) adds in its slot and log2(T) = 16 in the tree, and fsum rounds once more -- to first order
    (ceil(nnz / T) + 17) * 2^-53 of the total."""
    return (-(-nnz // T) + 17) * 2.0 ** -53


# ------------------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def values(n, k, seed=0):
    v = np.random.default_rng(900 + 10 * k + seed).standard_normal((n, k))
    v.setflags(write=False)
    return v


def edges_of(nb, top=0.9):
    """nb bins of unequal widths from 0 to `top`."""
    return top * (np.arange(nb + 1) / nb) ** 1.5


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
