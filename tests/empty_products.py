"""Products that are structurally empty although both operands hold entries, and the thresholds of the dispatch that the
cases aim at.  Every builder returns scipy CSR operands with nnz > 0 (tests/test_empty_products_cpu.py shows, with the
references alone, that each case is what it claims); shapes stay at a few hundred rows.  Cached: do not modify.

  missed_rows      A (300 x 200) stores entries only in a column set J, B (200 x 300) only in rows outside J: every row of
                   A*B has 0 products.  Row 0 of A is empty, row 1 holds one entry, row 2 all of J.
  strictly_lower   A strictly lower triangular, B lower triangular with its diagonal (400 x 400): A*B is strictly lower, so
                   with symmetric=True every row walks its products and stores nothing; symmetric=False is the control.
                   Rows TARGET_ROWS hold exactly the product counts on both sides of every threshold of the dispatch.
  lower_plus_one   strictly_lower with one entry A[r, r]: the single product A[r, r] * B[r, r] is the only output entry of
                   the symmetric product (nnz == 1, so no nnz == 0 early return can pass it).
  vectors          "inner": 1 x k times k x 1 with disjoint support (a 1 x 1 result without entries).  "outer": the m x m
                   result without entries.  A one-column A against a one-row B cannot be empty when both hold entries
                   (every stored A[i, 0] meets every stored B[0, j]), so the inner dimension is 2: A (m x 2) stores only
                   its column 0, B (2 x m) only its row 1.
  triple_t_empty   H (n x K) and a symmetric Q (K x K) whose stored rows are disjoint from H's columns: T = H*Q is empty.
  triple_s_empty   Q maps H's columns J onto J' with no common element (and J' back onto J: Q is symmetric): T = H*Q has
                   entries, T*H^T has none.
  masked_unreached A*B is not empty; the canonical mask lies entirely on positions no product reaches.
"""
import functools
import os
import re

import numpy as np
import scipy.sparse as sp

from helpers import shuffle_rows
from spmm_restatement import raw_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ the dispatch's own thresholds
def _kernel_source():
    return open(os.path.join(ROOT, "sparse_matrix_mult_amd", "csrc", "smm_kernels.hpp")).read()


def _engine_source():
    return open(os.path.join(ROOT, "sparse_matrix_mult_amd", "engine.py")).read()


@functools.lru_cache(maxsize=None)
def thresholds():
    """(tiny, small, medium): TINY_G of csrc/smm_kernels.hpp (smm_ctx::tiny_max: a row of at most tiny / 2 * tiny products
    goes to the 16- / 32-lane tiny-row kernels) and the defaults of Context.tune_hash (rows of C of at most small / medium
    nonzeros use the LDS-hash kernels), read from the sources."""
    tiny = int(re.search(r"constexpr\s+int\s+TINY_G\s*=\s*(\d+)\s*;", _kernel_source()).group(1))
    m = re.search(r"def tune_hash\(self,\s*small_max=(\d+),\s*medium_max=(\d+)\)", _engine_source())
    return tiny, int(m.group(1)), int(m.group(2))


def product_classes():
    """name -> (lo, hi]: the classes of a row's product count that strictly_lower must reach.  "far" is well above the
    last threshold: more than twice as many."""
    tiny, small, medium = thresholds()
    return {"tiny16": (0, tiny), "tiny32": (tiny, 2 * tiny), "small": (2 * tiny, small), "medium": (small, medium),
            "large": (medium, 2 * medium), "far": (2 * medium, np.inf)}


def row_products(A, B):
    """Products per row of A*B (the loop's trip count)."""
    lens = np.diff(B.indptr).astype(np.int64)
    per = np.concatenate([[0], np.cumsum(lens[A.indices])])
    return per[A.indptr[1:]] - per[A.indptr[:-1]]


def arrays(m):
    return (np.ascontiguousarray(m.indptr, dtype=np.int32), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float64))


def abs_arrays(m):
    """arrays(|m|) without scipy's abs(), which would canonicalise an unsorted matrix in place."""
    ptr, idx, val = arrays(m)
    return ptr, idx, np.abs(val)


def _values(rng, size):
    """Signed values with every magnitude in [0.25, 1): no product is zero, subnormal or rounded to zero."""
    return rng.uniform(0.25, 1.0, size) * rng.choice([-1.0, 1.0], size)


def frozen(M):
    """M with read-only arrays: scipy canonicalises an unsorted matrix IN PLACE in abs() and in comparisons such as
    M != 0, which on a cached case would quietly turn it into another one.  Such a call now raises; use M.copy()."""
    for a in (M.data, M.indices, M.indptr):
        a.setflags(write=False)
    return M


def _from_rows(rows_cols, n_cols, rng):
    lens = [len(c) for c in rows_cols]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.asarray(c, np.int64) for c in rows_cols]) if ptr[-1] else np.zeros(0, np.int64)
    M = raw_csr(ptr, idx, _values(rng, int(ptr[-1])), (len(rows_cols), n_cols))
    M.has_sorted_indices = True
    M.has_canonical_format = True
    return M


def unsorted_with_repeat(B, seed):
    """B with the first entry of every other non-empty row stored a second time (another value) and every row shuffled."""
    ptr, idx, val = np.asarray(B.indptr, np.int64), np.asarray(B.indices), np.asarray(B.data)
    ci, cv, cp = [], [], [0]
    for r in range(B.shape[0]):
        i, v = idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]
        if len(i) and r % 2 == 0:
            i, v = np.concatenate([i, i[:1]]), np.concatenate([v, [0.375]])
        ci.append(i); cv.append(v); cp.append(cp[-1] + len(i))
    out = shuffle_rows(raw_csr(cp, np.concatenate(ci), np.concatenate(cv), B.shape), seed)
    out.has_canonical_format = False
    return out


# ------------------------------------------------------------------------------ missed_rows
MISSED_VARIANTS = ("sorted", "unsorted")


@functools.lru_cache(maxsize=None)
def missed_rows(variant="sorted"):
    """(A, B, J).  variant "unsorted": B's rows shuffled, with repeated columns."""
    rng = np.random.default_rng(3100)
    m, k, n = 300, 200, 300
    J = np.sort(rng.choice(k, 60, replace=False))
    rows = [np.zeros(0, np.int64), J[:1], J]                                   # lengths 0, 1 and all of J
    for i in range(3, m):
        rows.append(np.sort(rng.choice(J, int(rng.integers(0, 25)), replace=False)))
    A = _from_rows(rows, k, rng)
    inJ = np.zeros(k, bool)
    inJ[J] = True
    brows = [np.zeros(0, np.int64) if inJ[r] else np.sort(rng.choice(n, int(rng.integers(1, 40)), replace=False)) for r in range(k)]
    B = _from_rows(brows, n, rng)
    if variant == "unsorted":
        B = unsorted_with_repeat(B, 3101)
    elif variant != "sorted":
        raise KeyError(variant)
    return frozen(A), frozen(B), J


# ------------------------------------------------------------------------------ strictly_lower, lower_plus_one
N_LOWER = 400
HEAD = 64                        # rows 0 .. HEAD-1 of B are full lower-triangular rows: row k holds k + 1 entries
EMPTY_ROWS = (0, 5, 77, 300)     # rows of A without entries (row 0 of a strictly lower matrix always is)
SHARDS = ((0, 120), (120, 260), (260, 400))
BEARING_SHARD = 1                # every row of this shard has products (and, symmetric, no output)
FAR_ROWS = (120, 200, N_LOWER - 1)          # rows with products well above the last threshold (every column left of the diagonal)


def _pick_lengths(target):
    """Distinct lengths among 1 .. HEAD that sum to target (row k of B's head has k + 1 entries): largest first."""
    out, cap, rem = [], HEAD, int(target)
    assert 0 < rem <= HEAD * (HEAD + 1) // 2
    while rem:
        step = min(rem, cap)
        out.append(step)
        rem -= step
        cap = step - 1
        assert rem == 0 or cap > 0
    return out


def target_counts():
    """The exact product counts of TARGET_ROWS: one, and both sides of every threshold."""
    tiny, small, medium = thresholds()
    return (1, tiny, tiny + 1, 2 * tiny, 2 * tiny + 1, small, small + 1, medium, medium + 1)


def target_rows():
    """row -> its exact product count.  The rows lie right below B's head, where a symmetric row still has more than
    `small` columns right of the diagonal."""
    return {HEAD + 1 + t: c for t, c in enumerate(target_counts())}


@functools.lru_cache(maxsize=None)
def strictly_lower():
    """(A, B), both N_LOWER x N_LOWER."""
    rng = np.random.default_rng(3200)
    n = N_LOWER
    assert thresholds()[2] + 1 <= HEAD * (HEAD + 1) // 2, "B's head no longer reaches the last threshold: raise HEAD"
    brows = []
    for k in range(n):
        if k < HEAD:
            brows.append(np.arange(k + 1))
        else:                                                   # the diagonal and half to all of the columns left of it
            brows.append(np.sort(np.concatenate([rng.choice(k, int(rng.integers(k // 2, k)), replace=False), [k]])))
    B = _from_rows(brows, n, rng)
    targets = target_rows()
    arows = []
    for i in range(n):
        if i in EMPTY_ROWS:
            arows.append(np.zeros(0, np.int64))
        elif i in targets:
            arows.append(np.sort(np.asarray(_pick_lengths(targets[i])) - 1))       # length L is row L - 1 of the head
        elif i in FAR_ROWS:
            arows.append(np.arange(i))                                             # every column left of the diagonal
        else:
            arows.append(np.sort(rng.choice(i, min(i, int(rng.integers(1, 30))), replace=False)))
    A = _from_rows(arows, n, rng)
    return frozen(A), frozen(B)


PLUS_ONE_VARIANTS = {"last_row": N_LOWER - 1, "row0": 0, "highest_class": FAR_ROWS[0]}


@functools.lru_cache(maxsize=None)
def lower_plus_one(variant):
    """(A, B, r): strictly_lower with A[r, r] = 0.75 stored (the row's last entry: rows stay ascending)."""
    A, B = strictly_lower()
    r = PLUS_ONE_VARIANTS[variant]
    ptr, idx, val = np.asarray(A.indptr, np.int64), np.asarray(A.indices), np.asarray(A.data)
    at = int(ptr[r + 1])
    new_ptr = ptr.copy()
    new_ptr[r + 1:] += 1
    A1 = raw_csr(new_ptr, np.insert(idx, at, r), np.insert(val, at, 0.75), A.shape)
    A1.has_sorted_indices = True
    A1.has_canonical_format = True
    return frozen(A1), B, r


# ------------------------------------------------------------------------------ vectors
VECTOR_VARIANTS = ("inner", "outer")


@functools.lru_cache(maxsize=None)
def vectors(variant):
    """(A, B): "inner" 1 x 70 times 70 x 1, "outer" 130 x 2 times 2 x 130 (see the module's docstring)."""
    rng = np.random.default_rng(3300)
    if variant == "inner":
        k = 70
        J = np.sort(rng.choice(k, 30, replace=False))
        rest = np.setdiff1d(np.arange(k), J)[::2]
        A = _from_rows([J], k, rng)
        B = _from_rows([np.zeros(1, np.int64) if r in set(rest.tolist()) else np.zeros(0, np.int64) for r in range(k)], 1, rng)
        return frozen(A), frozen(B)
    if variant == "outer":
        m = 130
        have = rng.random(m) < 0.6
        have[[0, m - 1]] = True, False                                            # a first row with an entry, a last without
        A = _from_rows([np.zeros(1, np.int64) if h else np.zeros(0, np.int64) for h in have], 2, rng)
        B = _from_rows([np.zeros(0, np.int64), np.sort(rng.choice(m, 50, replace=False))], m, rng)
        return frozen(A), frozen(B)
    raise KeyError(variant)


# ------------------------------------------------------------------------------ triple products
TRIPLE_CASES = ("triple_t_empty", "triple_s_empty")
N_TRIPLE, K_TRIPLE = 200, 300


def _h_in(cols, rng):
    """H (N_TRIPLE x K_TRIPLE) with 0 .. 8 entries per row, all in `cols`; rows 0 and 1 hold 1 and 8, row 2 none."""
    lens = [1, 8, 0] + [int(rng.integers(0, 9)) for _ in range(N_TRIPLE - 3)]
    return _from_rows([np.sort(rng.choice(cols, L, replace=False)) for L in lens], K_TRIPLE, rng)


@functools.lru_cache(maxsize=None)
def triple_case(name):
    """(H, Q) of TRIPLE_CASES: H is N_TRIPLE x K_TRIPLE, Q symmetric in pattern and values."""
    rng = np.random.default_rng(3400 + TRIPLE_CASES.index(name))
    K = K_TRIPLE
    perm = rng.permutation(K)
    J, Jp = np.sort(perm[:120]), np.sort(perm[120:240])
    H = _h_in(J, rng)
    if name == "triple_t_empty":                               # Q lives on J' x J' alone
        r, c = rng.choice(Jp, 600), rng.choice(Jp, 600)
    else:                                                      # Q lives on J x J' and J' x J: J -> J' -> J
        r, c = rng.choice(J, 600), rng.choice(Jp, 600)
    S = sp.csr_matrix((np.ones(600), (r, c)), shape=(K, K))
    S.sum_duplicates()
    S.data = _values(rng, S.nnz)
    Q = (S + S.T).tocsr()
    Q.sum_duplicates()
    Q.sort_indices()
    assert np.all(Q.data != 0)
    return frozen(H), frozen(Q)


@functools.lru_cache(maxsize=None)
def triple_mask():
    """A canonical N_TRIPLE x N_TRIPLE mask: 5 % at random, the diagonal, row 0 and the last column."""
    M = sp.random(N_TRIPLE, N_TRIPLE, density=0.05, format="lil", random_state=np.random.default_rng(3450))
    M.setdiag(1.0)
    M[0, :] = 1.0
    M[:, N_TRIPLE - 1] = 1.0
    M = M.tocsr()
    M.sum_duplicates()
    M.sort_indices()
    M.data[:] = 1.0
    return frozen(M)


def solve_diagonal():
    """R's diagonal for the two systems: three distinct values, so that CG on R alone ends after a few iterations."""
    return np.array([1.0, 2.0, 4.0])[np.arange(N_TRIPLE) % 3]


def solve_rhs(k=3):
    return np.random.default_rng(3460).standard_normal((N_TRIPLE, k))


# ------------------------------------------------------------------------------ masked product
def structural(A, B):
    """The pattern A*B reaches, as a boolean dense array."""
    ones = lambda M: sp.csr_matrix((np.ones(len(M.indices)), M.indices.copy(), M.indptr.copy()), shape=M.shape)  # noqa: E731
    return np.asarray((ones(A) @ ones(B)).toarray()) > 0


def _mask_of(free, rng, density):
    """A canonical mask of about `density` on the True positions of `free`."""
    pick = free & (rng.random(free.shape) < density)
    M = sp.csr_matrix(pick.astype(np.float64))
    M.sort_indices()
    M.has_canonical_format = True
    return frozen(M)


@functools.lru_cache(maxsize=None)
def masked_unreached():
    """(A, B, M): A (130 x 70), B (70 x 257), about a third of the positions reached; M on unreached positions only, rows
    of 0 to about 30 positions, row 3 of M empty."""
    rng = np.random.default_rng(3500)
    A = _from_rows([np.sort(rng.choice(70, int(rng.integers(0, 6)), replace=False)) for _ in range(130)], 70, rng)
    B = _from_rows([np.sort(rng.choice(257, int(rng.integers(1, 30)), replace=False)) for _ in range(70)], 257, rng)
    free = ~structural(A, B)
    free[3, :] = False
    return frozen(A), frozen(B), _mask_of(free, rng, 0.1)


@functools.lru_cache(maxsize=None)
def missed_rows_mask():
    """A canonical mask for missed_rows (no position is reached): 5 % at random."""
    A, B, _ = missed_rows()
    rng = np.random.default_rng(3510)
    return _mask_of(np.ones((A.shape[0], B.shape[1]), bool), rng, 0.05)
