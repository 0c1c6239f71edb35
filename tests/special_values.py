"""Non-finite, subnormal and huge values: the operands, the plants and the plain float64 reference of every product.

Every product of the library promises the values of the plain loop over STORED entries in stored order, each product
rounded and then added (no fused multiply-add).  The references below are that loop in numpy, one per operation; they
never skip a stored entry and never touch one that is not stored:

  plain_sparse   A*B in the reference's first-touch order (the first product of a column is stored, not added to 0.0),
                 optionally only the columns >= the row (symmetric)
  plain_dense    the same products added into a row of +0.0
  plain_triple   H*Q*H^T as T = H*Q (a dense row of +0.0 per row of H, as the reference's temp_values[K]) and then
                 sum = +0.0; sum += T[i, c] * H[k, c] over the stored entries of row k of H.  T is a DENSE row: a stored
                 entry of H meets +0.0 where T holds nothing, so an inf or NaN stored in row k of H makes the whole column
                 k of the result non-finite.  That is the reference's loop, the oracle's, and what the dense, the sparse
                 and the masked triple products of the library promise ("a miss reads +0.0").
  plain_masked   plain_sparse scattered to a mask; a position no product reaches is +0.0
  plain_spmm     Y = op(A) X (tests/spmm_restatement.py), plain_apply = H (Q (H^T X))
  plain_transpose  the arrays of scipy's tocsc(), values moved bit for bit

reverse_rows(M) stores every row backwards: the plain loops on reversed operands add the same terms in exactly the
opposite order, which is how the tests show that the CLASS (finite, +inf, -inf, NaN) of every default-mode output does
not depend on the order of summation.

The default-mode rule.  A default-mode input makes each output's class independent of summation order and of fusion:
non-finite results come only from planted inf / NaN entries, every other magnitude lies in [1e-3, 1e3].  Sums that
overflow are left to exact mode: a fused multiply-add legitimately gives fma(-1e300, 1e300, +inf) = +inf where the plain
loop gives NaN.
"""
import functools

import numpy as np
import scipy.sparse as sp

from helpers import rand_csr, shuffle_rows, signed
from spmm_restatement import raw_csr, restate_spmm, transpose_csr

FINITE, PINF, NINF, NAN = 0, 1, 2, 3
SUB = 2.0 ** -1074                      # the smallest subnormal: the ulp of every subnormal number


def cls(v):
    """Class of every element: FINITE, PINF, NINF or NAN (int8 array of v's shape)."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape, dtype=np.int8)
    out[v == np.inf] = PINF
    out[v == -np.inf] = NINF
    out[np.isnan(v)] = NAN
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits_nan(a, b):
    """Bit for bit, any NaN matching any NaN (the payload of a computed NaN is not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


# ------------------------------------------------------------------------------ CSR helpers
def csr(M):
    """(indptr int64, indices, data) of a scipy CSR, its own arrays."""
    return np.asarray(M.indptr, dtype=np.int64), np.asarray(M.indices), np.asarray(M.data, dtype=np.float64)


def reverse_rows(M):
    """The same matrix with every row stored backwards."""
    ptr, idx, val = csr(M)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(ptr))
    t = np.arange(len(idx)) - ptr[rows]                     # entry t of a row comes from the row's entry len-1-t
    src = ptr[rows + 1] - 1 - t
    return raw_csr(ptr, idx[src], val[src], M.shape)


def with_entries(M, entries):
    """Canonical CSR equal to M with (row, col, value) stored at each given position (added to the pattern if absent).
    Explicit zeros, inf and NaN stay stored."""
    ptr, idx, val = csr(M)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(ptr))
    r, c, v = list(rows), list(idx), list(val)
    where = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(rows, idx))}
    for (i, j, x) in entries:
        if (i, j) in where:
            v[where[(i, j)]] = x
        else:
            where[(i, j)] = len(v)
            r.append(i); c.append(j); v.append(x)
    r, c, v = np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(v, np.float64)
    o = np.lexsort((c, r))
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M.shape[0]))])
    out = raw_csr(out_ptr, c[o], v[o], M.shape)
    out.has_sorted_indices = True
    out.has_canonical_format = True
    return out


def without_entry(M, i, j):
    ptr, idx, val = csr(M)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(ptr))
    keep = ~((rows == i) & (idx == j))
    assert keep.sum() == len(idx) - 1
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=M.shape[0]))])
    out = raw_csr(out_ptr, idx[keep], val[keep], M.shape)
    out.has_sorted_indices = True
    out.has_canonical_format = True
    return out


def stored(M, i, j):
    ptr, idx, _ = csr(M)
    return bool(np.any(idx[ptr[i]:ptr[i + 1]] == j))


def bounded(M, seed):
    """helpers.signed values with every magnitude in [1e-3, 1): the default-mode rule."""
    M = signed(M, seed)
    small = np.abs(M.data) < 1e-3
    M.data[small] = np.copysign(0.5, M.data[small])
    return M


# ------------------------------------------------------------------------------ the plain loops
def _row_terms(A, B, i):
    """(columns, products) of row i of A*B in the loop's order: for p in A_i (stored order): for q in B_row(p)."""
    ap, ai, av = A
    bp, bi, bv = B
    cols, prods = [], []
    for p in range(ap[i], ap[i + 1]):
        s, e = bp[ai[p]], bp[ai[p] + 1]
        cols.append(bi[s:e])
        prods.append(av[p] * bv[s:e])
    if not cols:
        return np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(cols).astype(np.int64), np.concatenate(prods)


def _add_in_order(cols, prods, start_at_zero):
    """Terms added per column in their order.  Returns (columns in first-touch order, sums).  start_at_zero: the sum
    starts at +0.0 (dense outputs); otherwise the first product is stored as it is (sparse outputs)."""
    if len(cols) == 0:
        return cols, prods
    o = np.argsort(cols, kind="stable")
    sc = cols[o]
    new = np.concatenate([[True], sc[1:] != sc[:-1]])
    starts = np.flatnonzero(new)
    group = np.cumsum(new) - 1
    rank = np.arange(len(sc)) - starts[group]
    ucols = sc[starts]
    first = o[starts]                                     # position of each column's first term
    acc = np.zeros(len(ucols)) if start_at_zero else None
    sp_ = prods[o]
    for r in range(int(rank.max()) + 1):
        sel = rank == r
        g = group[sel]
        if r == 0 and not start_at_zero:
            acc = sp_[sel].copy()
        else:
            acc[g] = acc[g] + sp_[sel]
    touch = np.argsort(first, kind="stable")
    return ucols[touch], acc[touch]


def plain_sparse(A, B, symmetric=False):
    """(indptr int64, indices int32, data) of A*B, first-touch order."""
    a, b = csr(A), csr(B)
    ptr, idx, val = [0], [], []
    with np.errstate(all="ignore"):
        for i in range(A.shape[0]):
            cols, prods = _row_terms(a, b, i)
            if symmetric:
                keep = cols >= i
                cols, prods = cols[keep], prods[keep]
            c, v = _add_in_order(cols, prods, False)
            idx.append(c); val.append(v); ptr.append(ptr[-1] + len(c))
    return (np.asarray(ptr, np.int64), np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32),
            np.concatenate(val) if val else np.zeros(0))


def plain_dense(A, B, symmetric=False):
    a, b = csr(A), csr(B)
    C = np.zeros((A.shape[0], B.shape[1]))
    with np.errstate(all="ignore"):
        for i in range(A.shape[0]):
            cols, prods = _row_terms(a, b, i)
            if symmetric:
                keep = cols >= i
                cols, prods = cols[keep], prods[keep]
            c, v = _add_in_order(cols, prods, True)
            C[i, c] = v
    return C


def row_products(A, B):
    """Products per row of A*B (the loop's trip count)."""
    lens = np.diff(B.indptr).astype(np.int64)
    per = np.concatenate([[0], np.cumsum(lens[A.indices])])
    return per[A.indptr[1:]] - per[A.indptr[:-1]]


def term_counts(A, B):
    """Dense array: number of products that land on each position of A*B."""
    return np.asarray((_ones(A) @ _ones(B)).toarray())


def _ones(M):
    ptr, idx, val = csr(M)
    return sp.csr_matrix((np.ones(len(idx)), idx.copy(), ptr.copy()), shape=M.shape)


def _finite_abs(M):
    ptr, idx, val = csr(M)
    return sp.csr_matrix((np.where(np.isfinite(val), np.abs(val), 0.0), idx.copy(), ptr.copy()), shape=M.shape)


def magnitudes(A, B):
    """(|A| |B|)[i, j] over the finite entries: the scale of the default-mode bound at a finite output (a finite output
    has finite terms only)."""
    return np.asarray((_finite_abs(A) @ _finite_abs(B)).toarray())


def _t_rows(H, Q):
    """T = H*Q as dense rows of +0.0 (n x K)."""
    h, q = csr(H), csr(Q)
    T = np.zeros((H.shape[0], Q.shape[1]))
    for i in range(H.shape[0]):
        cols, prods = _row_terms(h, q, i)
        c, v = _add_in_order(cols, prods, True)
        T[i, c] = v
    return T


def _stage2(T, H):
    """S[i, k] = (+0.0, then += T[i, c] * H[k, c] over row k's stored entries in stored order), every i and k."""
    ptr, idx, val = csr(H)
    n = H.shape[0]
    S = np.zeros((T.shape[0], n))
    lens = np.diff(ptr)
    for s in range(int(lens.max()) if n else 0):
        rows = np.flatnonzero(lens > s)
        p = ptr[rows] + s
        S[:, rows] = S[:, rows] + T[:, idx[p]] * val[p][None, :]
    return S


def triple_from_sums(S, full=0):
    """The n x n result from the stage-2 sums S[i, k]: the upper triangle (full=0, the rest +0.0) or the reference's
    full matrix, C[i, k] = (0.0 + S[min, max]) + S[max, min] off the diagonal (row min(i, k) writes both mirror images
    first, row max(i, k) adds to both)."""
    n = S.shape[0]
    with np.errstate(all="ignore"):
        C = np.zeros_like(S)
        iu = np.triu_indices(n, 0 if not full else 1)
        if not full:
            C[iu] = 0.0 + S[iu]                             # c[i][k] += sum on a calloc'd row
            return C
        off = (0.0 + S[iu]) + S.T[iu]
        C[iu] = off
        C.T[iu] = off
        d = np.arange(n)
        C[d, d] = 0.0 + S[d, d]
        return C


def plain_triple(H, Q, full=0):
    with np.errstate(all="ignore"):
        return triple_from_sums(_stage2(_t_rows(H, Q), H), full)


def triple_magnitudes(H, Q, full=0):
    with np.errstate(all="ignore"):                        # (the huge case: magnitudes overflow; exact mode does not use them)
        M = np.asarray((_finite_abs(H) @ _finite_abs(Q) @ _finite_abs(H).T).toarray())
        return M + M.T - np.diag(np.diag(M)) if full else M


def triple_term_counts(H, Q, full=0):
    """Products (both stages) behind each position: stage 2 adds nnz(H_k) products, each a sum of stage-1 terms."""
    M = np.asarray((_ones(H) @ _ones(Q) @ _ones(H).T).toarray()) + np.diff(H.indptr)[None, :]
    return M + M.T if full else M


def plain_masked(A, B, M):
    """Values of A*B at the positions of the canonical mask M, in M's order; +0.0 where no product lands."""
    ptr, idx, val = plain_sparse(A, B)
    out = np.zeros(M.nnz)
    mp, mi, _ = csr(M)
    for i in range(M.shape[0]):
        have = dict(zip(idx[ptr[i]:ptr[i + 1]].tolist(), val[ptr[i]:ptr[i + 1]].tolist()))
        out[mp[i]:mp[i + 1]] = [have.get(c, 0.0) for c in mi[mp[i]:mp[i + 1]].tolist()]
    return out


def plain_spmm(A, X, transpose=False):
    with np.errstate(all="ignore"):
        return restate_spmm(A, X, transpose)


def plain_apply(H, Q, X):
    with np.errstate(all="ignore"):
        return restate_spmm(H, restate_spmm(Q, restate_spmm(H, X, True)))


def plain_transpose(A):
    """(indptr, indices, data) of A^T: entries of column j in the order the row loop meets them, values bit for bit."""
    ptr, idx, val = csr(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(ptr))
    o = np.argsort(idx, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=A.shape[1]))])
    return tptr.astype(np.int64), rows[o].astype(np.int32), val[o]


# ------------------------------------------------------------------------------ operands
SHAPES = {"small": (130, 70, 257, 0.08, 0.05), "large": (300, 2000, 20000, 0.01, 0.004)}


def _set_row(M, i, cols):
    """M with row i replaced by ones at the given columns."""
    L = M.tolil()
    L[i, :] = 0
    for c in cols:
        L[i, c] = 1.0
    out = L.tocsr()
    out.sort_indices()
    return out


@functools.lru_cache(maxsize=None)
def ab_base(shape):
    """A, B of the CSR x CSR tests with bounded signed values.  Besides the random rows:
    small: rows 10, 11, 12 of B share 12 columns and row 3 of A names exactly those rows (36 products on 12 columns: a
    hash-class row even with the threshold at 24); row 5 of A has 30 entries (beyond 150 nonzeros: a tile row next to
    the 24 / 150 hash kernels).  large: row 3 of A has one entry, row 4 three, row 5 sixty (<= 150, <= 256 and > 2048
    nonzeros; the random rows hold about 1500).  tiny: 300 rows of 1-5 entries against rows of 2-6."""
    rng = np.random.default_rng(900)
    if shape == "tiny":
        la, lb = rng.integers(1, 6, 300), rng.integers(2, 7, 300)
        A = _rows_of(la, 300, rng)
        B = _rows_of(lb, 300, rng)
    else:
        m, k, n, da, db = SHAPES[shape]
        A, B = rand_csr(m, k, da, 901), rand_csr(k, n, db, 902)
        if shape == "small":
            share = np.sort(rng.choice(n, 12, replace=False))
            for r in (10, 11, 12):
                B = _set_row(B, r, share)
            A = _set_row(A, 3, [10, 11, 12])
            A = _set_row(A, 5, np.sort(rng.choice(k, 30, replace=False)))
        else:
            A = _set_row(A, 3, [17])
            A = _set_row(A, 4, [40, 900, 1777])
            A = _set_row(A, 5, np.sort(rng.choice(k, 60, replace=False)))
    return bounded(A, 903), bounded(B, 904)


def _rows_of(lens, n, rng):
    cols = [np.sort(rng.choice(n, int(L), replace=False)) for L in lens]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    M = raw_csr(ptr, np.concatenate(cols), np.ones(int(ptr[-1])), (len(lens), n))
    M.has_sorted_indices = True
    M.has_canonical_format = True
    return M


def _q(k, d, seed):
    S = sp.random(k, k, density=d / 2, format="csr", random_state=np.random.default_rng(seed))
    Q = (S + S.T).tocsr()
    Q.sort_indices()
    return Q


TRIPLE_SHAPES = {"n60": (60, 90, 0.1, 0.1), "n300": (300, 2500, 0.02, 0.004), "n1100": (1100, 1200, 0.02, 0.004)}


# (1100, 1200) is more than one k-group of 1024 rows of H.  A time trade-off: the plain reference of this shape takes
# seconds per case, so it runs 11 of the 17 cases -- every kind of plant, and the edges that differ at this size (first and
# last stored entry, column 0, the last column, a column that is a multiple of 64); the remaining edges and the H plants
# of inf and NaN run on the two smaller shapes and, with a row range that starts inside a block, on (300, 2500).
BIG_TRIPLE_CASES = [("inf_reached_by_some", "Q"), ("inf_minus_inf", "Q"), ("nan_in_left", "Q"), ("edge_first", "Q"),
                    ("edge_last", "Q"), ("edge_col0", "Q"), ("edge_last_col", "Q"), ("edge_col64", "Q"), ("subnormal", "Q"),
                    ("huge", "Q"), ("stored_zero_times_inf", "H")]


@functools.lru_cache(maxsize=None)
def triple_base(shape):
    """H (n x K), Q (K x K, symmetric pattern), bounded signed values."""
    if shape == "window":                                   # sparse / masked triple: 4 entries in a 16-column window, band Q
        rng = np.random.default_rng(910)
        n, K = 400, 1500
        start = rng.integers(0, K - 16, n)
        cols = [np.sort(s + rng.choice(16, 4, replace=False)) for s in start]
        H = raw_csr(np.arange(0, 4 * n + 1, 4), np.concatenate(cols), np.ones(4 * n), (n, K))
        H.has_sorted_indices = True
        H.has_canonical_format = True
        Q = sp.diags([np.ones(K - abs(o)) for o in range(-4, 5)], list(range(-4, 5)), shape=(K, K), format="csr")
        Q.sort_indices()
    else:
        n, K, dh, dq = TRIPLE_SHAPES[shape]
        H, Q = rand_csr(n, K, dh, 911), _q(K, dq, 912)
    return bounded(H, 913), bounded(Q, 914)


# ------------------------------------------------------------------------------ the plants
#   name -> classes the case claims to produce ("inf" = +inf or -inf)
PLANTS = {
    "inf_reached_by_some": {"finite", "inf"},
    "inf_minus_inf": {"finite", "nan"},
    "stored_zero_times_inf": {"finite", "nan"},
    "unstored_zero_times_inf": {"finite"},                 # the finite twin of stored_zero_times_inf
    "nan_in_left": {"finite", "nan"},
    "edge_first": {"finite", "inf"}, "edge_last": {"finite", "inf"}, "edge_row_end": {"finite", "inf"},
    "edge_col0": {"finite", "inf"}, "edge_last_col": {"finite", "inf"}, "edge_col50": {"finite", "inf"},
    "edge_col64": {"finite", "inf"}, "edge_lower": {"finite"},
    "subnormal": {"finite"},
    "huge": {"finite", "inf", "nan"},
}
DEFAULT_PLANTS = [p for p in PLANTS if p != "huge"]          # huge: sums that overflow, exact mode only
EXACT_PLANTS = list(PLANTS)


def _named_by(A):
    """For every column of A: the rows that store it."""
    ptr, idx, _ = csr(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(ptr))
    out = [[] for _ in range(A.shape[1])]
    for r, c in zip(rows.tolist(), idx.tolist()):
        out[c].append(r)
    return out


def _pick_pair(A, B, min_row=0):
    """(i, r1, r2): a row i >= min_row of A with at least two entries whose rows r1, r2 of B are not empty and which few
    other rows name (keeps the non-finite share small)."""
    ap, ai, _ = csr(A)
    bl = np.diff(B.indptr)
    pop = np.bincount(ai, minlength=A.shape[1])
    best = None
    for i in range(min_row, A.shape[0]):
        cs = [c for c in ai[ap[i]:ap[i + 1]].tolist() if bl[c] > 0]
        if len(cs) >= 2:
            cs = sorted(cs, key=lambda c: pop[c])[:2]
            cost = pop[cs[0]] + pop[cs[1]]
            if best is None or cost < best[0]:
                best = (cost, i, cs[0], cs[1])
    assert best is not None
    return best[1], best[2], best[3]


def plant(A, B, name, triple=False):
    """(A', B', note) for left operand A and right operand B (B, Q; for H*Q*H^T: A = H, B = Q).  note: dict with the
    planted positions.  Columns are taken at or right of the rows that reach them, so that the upper-triangle variants see
    the plant too (edge_lower: strictly left).  triple: the planted column of Q is one that H names (Q's diagonal at a
    column of the planted row of H), so that stage 2 reads the planted T."""
    m, n = A.shape[0], B.shape[1]
    ap, ai, av = csr(A)
    bp, bi, bv = csr(B)
    if name == "subnormal":
        A2, B2 = A.copy(), B.copy()
        ra = np.repeat(np.arange(m), np.diff(ap))
        rb = np.repeat(np.arange(B.shape[0]), np.diff(bp))
        A2.data = np.where(ra % 3 == 0, av * 1e-160, np.where(np.arange(len(av)) % 5 == 0, av * 1e-160, av))
        B2.data = np.where(rb % 2 == 0, bv * 1e-160, bv)
        return A2, B2, {}
    if name == "huge":
        i, r1, r2 = _pick_pair(A, B)
        c = r1 if triple else int(bi[bp[r1]])               # first column of row r1 of B
        B2 = B.copy()
        B2.data[bp[r1]:bp[r1 + 1]] *= 1e200                 # the whole row: (i, its columns) overflow one by one
        B2 = with_entries(B2, [(r1, c, 1e200), (r2, c, 1e200)])
        A2 = with_entries(A, [(i, r1, 1e200), (i, r2, -1e200)])   # column c: +inf from r1, then -inf from r2
        return A2, B2, {"row": i, "col": c}
    if name.startswith("edge_"):
        pop = np.bincount(ai, minlength=A.shape[1])
        full = np.flatnonzero(np.diff(bp) > 0)              # rows of B that store something
        busy = int(full[np.argmax(pop[full])])              # ... the one most rows of A name
        if name == "edge_first":
            r = int(full[0]); c = int(bi[0])
        elif name == "edge_last":
            r = int(full[-1]); c = int(bi[-1])
        elif name == "edge_row_end":
            r = busy; c = int(bi[bp[r + 1] - 1])
        elif name == "edge_lower":                          # column 0, reached only by rows below row 0
            r = int(next(x for x in full[np.argsort(-pop[full], kind="stable")] if pop[x] and min(_named_by(A)[x]) > 0)); c = 0
        else:
            r = busy
            c = {"edge_col0": 0, "edge_last_col": n - 1, "edge_col50": 19200 if n > 19200 else 50 * ((n - 1) // 50),
                 "edge_col64": 64 * ((n - 1) // 64)}[name]  # 19200 = 50 * 384 = 64 * 300
        A2 = A
        if name != "edge_lower":                            # reached, and by a row at or above the column (upper triangle)
            A2 = with_entries(A, [(min(c, m - 1), r, 0.75)] + ([(min(c, m - 1), c, 0.75)] if triple else []))
        return A2, with_entries(B, [(r, c, np.inf)]), {"brow": r, "col": c}
    i, r1, r2 = _pick_pair(A, B, min_row=0)
    c = int(bi[bp[r1 + 1] - 1])                             # last column of row r1 of B
    if c < i:
        c = n - 1
    if triple:
        c = r1
    if name == "inf_reached_by_some":
        return A, with_entries(B, [(r1, c, np.inf)]), {"row": i, "brow": r1, "col": c}
    if name == "inf_minus_inf":
        a1, a2 = (float(av[ap[i]:ap[i + 1]][ai[ap[i]:ap[i + 1]] == r][0]) for r in (r1, r2))
        # the products are +inf and -inf whatever the signs of A's entries
        return A, with_entries(B, [(r1, c, np.copysign(np.inf, a1)), (r2, c, -np.copysign(np.inf, a2))]), {"row": i, "col": c}
    if name in ("stored_zero_times_inf", "unstored_zero_times_inf"):
        # (i, r1) stored as 0.0 meets B[r1, c] = inf; B[r2, c] finite keeps (i, c) in the pattern of the twin
        B2 = with_entries(B, [(r1, c, np.inf), (r2, c, 0.625)] if not stored(B, r2, c) else [(r1, c, np.inf)])
        A2 = with_entries(A, [(i, r1, 0.0)])
        if name == "unstored_zero_times_inf":
            A2 = without_entry(A2, i, r1)
        return A2, B2, {"row": i, "col": c}
    if name == "nan_in_left":
        return with_entries(A, [(i, r1, np.nan)]), B, {"row": i, "brow": r1}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ab_case(shape, name):
    A, B = ab_base(shape)
    A2, B2, note = plant(A, B, name)
    return A2, B2, note


@functools.lru_cache(maxsize=None)
def triple_case(shape, name, where="Q"):
    """where = "Q": the plant goes into Q (and, for the stored zero and the NaN, into H: the left operand of H*Q);
    where = "H": the inf / NaN / zero is stored in H itself and is met by T in stage 2."""
    H, Q = triple_base(shape)
    if where == "Q":
        H2, Q2, note = plant(H, Q, name, triple=True)
        return H2, Q2, note
    hp, hi, _ = csr(H)
    k = H.shape[0] // 2
    while hp[k + 1] - hp[k] < 2:
        k += 1
    c = int(hi[hp[k]])
    value = {"inf_reached_by_some": np.inf, "nan_in_left": np.nan, "stored_zero_times_inf": 0.0}[name]
    if name == "stored_zero_times_inf":                     # H[k, c] = 0.0 meets T[i, c] = inf for the rows i that reach it
        i, r1, _ = _pick_pair(H, Q)
        qc = int(Q.indices[Q.indptr[r1]])
        return with_entries(H, [(k, qc, 0.0)]), with_entries(Q, [(r1, qc, np.inf)]), {"row": i, "col": k}
    return with_entries(H, [(k, c, value)]), Q, {"col": k}


# ------------------------------------------------------------------------------ inputs whose sums are exact
#   Default mode lets the waves of a workgroup add to one accumulator at once (CSR x CSR, dense output, dense triple
#   product), so the ORDER of a sum is not fixed and, where a sum rounds, neither is its last bit.  "Two default-mode
#   runs agree bit for bit" is therefore asked on inputs on which no sum and no product rounds: every finite value a
#   multiple of 2^-8 (times one power of two per operand), so that every partial sum in any order, fused or not, is a
#   multiple of one granule within 53 bits and hence exact.  On such inputs the bits cannot depend on the order, and a
#   difference between two runs is a lost or doubled update, a race or an uninitialised accumulator.  The same plants,
#   shapes and patterns as the other tests; only the finite values are narrowed.
GRANULE = 2.0 ** -8
SUBNORMAL_SCALE = {False: 2.0 ** -525, True: 2.0 ** -350}    # per operand: A*B and H*Q*H^T (H enters twice) end subnormal


def quantised(M, scale=1.0):
    """M with every finite nonzero value rounded to a nonzero multiple of 2^-8 (sign kept), times scale; zeros, inf and
    NaN stay as they are."""
    M = M.copy()
    v = M.data
    q = np.copysign(np.maximum(np.round(np.abs(v) / GRANULE), 1.0) * GRANULE, v) * scale
    M.data = np.where(np.isfinite(v) & (v != 0), q, v)
    return M


@functools.lru_cache(maxsize=None)
def exact_ab_case(shape, name):
    """ab_case with exact sums.  subnormal: the whole of A and of B scaled by 2^-525 (every product and sum a subnormal
    multiple of 2^-1066); rows that mix subnormal and normal terms round, so they stay with the other tests."""
    if name == "subnormal":
        A, B = ab_base(shape)
        return quantised(A, SUBNORMAL_SCALE[False]), quantised(B, SUBNORMAL_SCALE[False])
    A, B, _ = ab_case(shape, name)
    return quantised(A), quantised(B)


@functools.lru_cache(maxsize=None)
def exact_triple_case(shape, name, where="Q"):
    """triple_case with exact sums.  subnormal: H and Q scaled by 2^-350: T = H*Q is normal (multiples of 2^-716) and
    every term and sum of stage 2 is a subnormal multiple of 2^-1074."""
    if name == "subnormal":
        H, Q = triple_base(shape)
        return quantised(H, SUBNORMAL_SCALE[True]), quantised(Q, SUBNORMAL_SCALE[True])
    H, Q, _ = triple_case(shape, name, where)
    return quantised(H), quantised(Q)


# ------------------------------------------------------------------------------ row classes of the CSR x CSR dispatch
HASH_CONFIGS = {"hash+tiles": (256, 2048), "tiles-only": (0, 0), "small-hash": (24, 150), "slab-all": (0, 0),
                "slab-narrow": (24, 150), "idx32": (24, 150), "dense-runs": (0, 0)}
# the classes each (shape, hash thresholds) is meant to reach; a tiny row (<= 16 / <= 32 products from as many entries of
# A) goes to the tiny-row kernels whatever the thresholds
REQUIRED_CLASSES = {
    ("small", (256, 2048)): {"hash_small"},
    ("small", (24, 150)): {"hash_small", "hash_medium", "tiles"},
    ("small", (0, 0)): {"tiles"},
    ("large", (256, 2048)): {"hash_small", "hash_medium", "tiles"},
    ("large", (24, 150)): {"hash_medium", "tiles"},
    ("large", (0, 0)): {"tiles"},
    ("tiny", (256, 2048)): {"tiny16", "tiny32"},
    ("tiny", (24, 150)): {"tiny16", "tiny32"},
    ("tiny", (0, 0)): {"tiny16", "tiny32"},
}


def row_classes(A, B, indptr, thresholds):
    """Class of every row of C from its products, its entries of A and its nonzeros (the plain result's indptr)."""
    small, medium = thresholds
    prod, na, nc = row_products(A, B), np.diff(A.indptr), np.diff(indptr)
    out = []
    for p, a, c in zip(prod.tolist(), na.tolist(), nc.tolist()):
        if c == 0:
            out.append("empty")
        elif p <= 16 and a <= 16:
            out.append("tiny16")
        elif p <= 32 and a <= 32:
            out.append("tiny32")
        elif c <= small:
            out.append("hash_small")
        elif c <= medium:
            out.append("hash_medium")
        else:
            out.append("tiles")
    return out


def unsorted_with_repeat(B, seed):
    """B with the first entry of every other non-empty row stored a second time (another value) and every row shuffled:
    the general path for unsorted operands with repeated columns."""
    ptr, idx, val = csr(B)
    rng = np.random.default_rng(seed)
    ci, cv, cp = [], [], [0]
    for r in range(B.shape[0]):
        i, v = idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]
        if len(i) and r % 2 == 0:
            i, v = np.concatenate([i, i[:1]]), np.concatenate([v, [0.375]])
        ci.append(i); cv.append(v); cp.append(cp[-1] + len(i))
    return shuffle_rows(raw_csr(cp, np.concatenate(ci), np.concatenate(cv), B.shape), seed)


def present(classes, claim):
    """Does an array of classes hold what a claim names?"""
    if claim == "finite":
        return bool(np.any(classes == FINITE))
    if claim == "inf":
        return bool(np.any((classes == PINF) | (classes == NINF)))
    return bool(np.any(classes == NAN))


# ------------------------------------------------------------------------------ masked A*B, sparse x dense, transpose
@functools.lru_cache(maxsize=None)
def random_mask(m, n):
    """A canonical random mask of 10 % that also holds row 0, column 0 and the last column (the edge plants)."""
    M = rand_csr(m, n, 0.1, 920).tolil()
    M[0, :] = 1.0
    M[:, 0] = 1.0
    M[:, n - 1] = 1.0
    M = M.tocsr()
    M.sort_indices()
    return M


@functools.lru_cache(maxsize=None)
def masked_case(name):
    """(A, B, M): the small operands with the plant, and a canonical mask: 10 % at random, row 0, column 0, the last
    column, and every position whose plain value is not finite (and the stored zero's position in its finite twin), so
    that the mask sees the plant."""
    A, B, note = ab_case("small", name)
    D = plain_dense(A, B)
    r, c = np.nonzero(~np.isfinite(D))
    extra = [(int(i), int(j), 1.0) for i, j in zip(r, c)] + ([(note["row"], note["col"], 1.0)] if "row" in note and "col" in note else [])
    return A, B, with_entries(random_mask(A.shape[0], B.shape[1]), extra)


@functools.lru_cache(maxsize=None)
def exact_masked_case(name):
    """masked_case on the exact-sum operands (the row path's longer classes add from several waves in default mode)."""
    A, B = exact_ab_case("small", name)
    return A, B, masked_case(name)[2]


SPMM_X_PLANTS = ["inf_reached_by_some", "inf_minus_inf", "unstored_zero_times_inf", "edge_first_row", "edge_last_row"]
SPMM_PLANTS = SPMM_X_PLANTS + ["stored_zero_times_inf", "nan_in_left", "edge_nan_first", "edge_nan_last", "subnormal", "huge"]


@functools.lru_cache(maxsize=None)
def spmm_base():
    return bounded(rand_csr(200, 300, 0.05, 930), 931)


@functools.lru_cache(maxsize=None)
def apply_h():
    """H of triple_product_apply, 200 x 300: 4 entries per row in a 16-column window.  With the band Q below, a plant
    in X or in H reaches only the rows of H whose windows lie next to it, so most of Y stays finite even for k = 1."""
    rng = np.random.default_rng(934)
    start = rng.integers(0, 300 - 16, 200)
    cols = [np.sort(s + rng.choice(16, 4, replace=False)) for s in start]
    H = raw_csr(np.arange(0, 801, 4), np.concatenate(cols), np.ones(800), (200, 300))
    H.has_sorted_indices = True
    H.has_canonical_format = True
    return bounded(H, 935)


@functools.lru_cache(maxsize=None)
def apply_q(K):
    """Q of triple_product_apply: a band of half-width 1 (not symmetric in its values)."""
    Q = sp.diags([np.ones(K - abs(o)) for o in (-1, 0, 1)], [-1, 0, 1], shape=(K, K), format="csr")
    Q.sort_indices()
    return bounded(Q, 933)


def spmm_case(name, k, transpose, apply=False):
    """(A, X, col): Y = op(A) X with the plant in A or in column col of X (op(A) = A^T when transpose).  Positions are
    chosen on L = op(A); an entry (i, r) of L is the entry (r, i) of A when transposed.  apply: A is apply_h(), the H of
    Y = H (Q (H^T X)) (transpose must be set: X has H.rows rows)."""
    A = apply_h() if apply else spmm_base()
    L = transpose_csr(A) if transpose else A
    L.has_sorted_indices = True
    lp, li, lv = csr(L)
    rng = np.random.default_rng(940 + k)
    X = rng.uniform(0.25, 1.0, (L.shape[1], k)) * rng.choice([-1.0, 1.0], (L.shape[1], k))
    col = k // 2
    pop = np.bincount(li, minlength=L.shape[1])
    i = int(np.argmax(np.diff(lp) >= 2))                    # a row of L with two entries
    r1, r2 = int(li[lp[i]]), int(li[lp[i] + 1])
    a1, a2 = float(lv[lp[i]]), float(lv[lp[i] + 1])

    def left(entries, drop=None):
        M = with_entries(A, [((r, i_) if transpose else (i_, r)) + (v,) for (i_, r, v) in entries])
        if drop:
            M = without_entry(M, *((drop[1], drop[0]) if transpose else drop))
        return M
    if name == "inf_reached_by_some":
        X[r1, col] = np.inf
    elif name == "inf_minus_inf":
        X[r1, col], X[r2, col] = np.copysign(np.inf, a1), -np.copysign(np.inf, a2)
    elif name == "stored_zero_times_inf":
        A = left([(i, r1, 0.0)]); X[r1, col] = np.inf
    elif name == "unstored_zero_times_inf":
        A = left([], drop=(i, r1)); X[r1, col] = np.inf
    elif name == "nan_in_left":
        A = left([(i, r1, np.nan)])
    elif name == "edge_first_row":
        X[int(np.flatnonzero(pop)[0]), col] = -np.inf
    elif name == "edge_last_row":
        X[int(np.flatnonzero(pop)[-1]), col] = np.inf
    elif name in ("edge_nan_first", "edge_nan_last"):       # the first / last stored entry of A itself
        A = A.copy()
        A.data[0 if name == "edge_nan_first" else -1] = np.nan
    elif name == "subnormal":
        A = A.copy()
        A.data = np.where(np.arange(A.nnz) % 3 == 0, A.data * 1e-160, A.data)
        X[::2] *= 1e-160
    elif name == "huge":
        A = left([(i, r1, 1e200), (i, r2, -1e200)])
        X[r1, :], X[r2, :] = 1e200, 1e200                   # row i: +inf then -inf in every column
        X[r2, 0] = 0.5                                      # ... but +inf alone in column 0
    else:
        raise KeyError(name)
    return A, X, col


@functools.lru_cache(maxsize=None)
def transpose_operand():
    """257 x 130 with +-inf, NaNs of several payloads, -0.0, stored +0.0 and subnormals among signed values, at the
    first and the last stored entry, in column 0, in the last column and at row ends."""
    A = signed(rand_csr(257, 130, 0.1, 950), 951)
    A = with_entries(A, [(0, 0, -0.0), (0, 129, 5e-324), (256, 0, 0.0), (256, 129, -np.inf), (100, 64, np.inf), (128, 50, -2.5e-310)])
    nan = np.array([0x7FF8000000000000, 0x7FF8000000000123, 0xFFF8000000000001, 0x7FF4000000000000 | 0x0008000000000000],
                   dtype=np.uint64).view(np.float64)
    at = [0, A.nnz - 1, int(A.indptr[7 + 1]) - 1, int(A.indptr[200])]
    special = np.array([-0.0, 0.0, 5e-324, -1e-310, np.inf, -np.inf])
    A.data[np.arange(3, A.nnz, 11)[:600]] = np.resize(special, len(np.arange(3, A.nnz, 11)[:600]))
    A.data[at] = nan
    return A
