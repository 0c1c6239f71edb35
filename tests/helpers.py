"""Shared input generators and comparison helpers of the test-suite."""
import numpy as np
import scipy.sparse as sp


def rand_csr(m, n, density, seed, dtype=np.float64):
    """BASELINE's generator: uniform[0,1) values, sorted unique indices."""
    return sp.random(m, n, density=density, format="csr", random_state=np.random.default_rng(seed), dtype=dtype)


def wide_csr(m, n, per_row, seed):
    """~per_row distinct random columns per row for very wide matrices (scipy.sparse.random permutes all
    m*n positions, which is hopeless at 1e6 columns)."""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.integers(0, n, size=(m, per_row)), axis=1)
    keep = np.ones_like(cols, dtype=bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    indptr = np.zeros(m + 1, np.int32)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    return sp.csr_matrix((rng.standard_normal(int(indptr[-1])), cols[keep].astype(np.int32), indptr), shape=(m, n))


def arrays(m):
    return (np.ascontiguousarray(m.indptr, dtype=np.int32), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float64))


def signed(m, seed):
    """Same pattern, values in [-1,1): exercises cancellation and signed zeros."""
    r = np.random.default_rng(seed)
    out = m.copy()
    out.data = r.uniform(-1.0, 1.0, size=out.nnz)
    return out


def shuffle_rows(m, seed):
    """Same matrix with the entries of every row in random order (non-canonical CSR)."""
    r = np.random.default_rng(seed)
    m = m.tocsr().copy()
    for i in range(m.shape[0]):
        s, e = m.indptr[i], m.indptr[i + 1]
        p = r.permutation(e - s)
        m.indices[s:e] = m.indices[s:e][p]
        m.data[s:e] = m.data[s:e][p]
    m.has_sorted_indices = False
    return m


def assert_csr_equal(got, want, values="bits", rtol=1e-10):
    """indptr and indices bit-exact (reference first-touch order); values bit-exact or within
    the north star's tolerance (1e-10 relative)."""
    gp, gi, gv = got
    wp, wi, wv = want
    assert np.array_equal(np.asarray(gp, dtype=np.int64), np.asarray(wp, dtype=np.int64)), "indptr differs"
    assert np.array_equal(gi, wi), "indices differ (first-touch order)"
    if values == "bits":
        assert np.array_equal(gv.view(np.int64), wv.view(np.int64)), \
            f"values differ bitwise (max rel {rel_err(gv, wv):.3e})"
    else:
        assert rel_err(gv, wv) <= rtol, f"values differ: max rel {rel_err(gv, wv):.3e}"


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    if a.size == 0:
        return 0.0
    d = np.abs(a - b)
    s = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
    ok = d == 0
    return float(np.max(np.where(ok, 0.0, d / s)))


RTOL = 1e-10               # default mode: relative to the sum of the magnitudes of the terms


# ------------------------------------------------------------------------------ masked SpGEMM against the oracle
def masked_want(oracle, A, B):
    """The oracle's unmasked product scattered to dense arrays: values and the stored-position map."""
    m, n = A.shape[0], B.shape[1]
    ptr, idx, val = oracle.sparse(arrays(A), arrays(B), n)
    rows = np.repeat(np.arange(m), np.diff(ptr))
    W = np.zeros((m, n))
    S = np.zeros((m, n), dtype=bool)
    W[rows, idx] = val
    S[rows, idx] = True
    return W, S


def check_masked_values(got, M, A, B, W, S, exact):
    """got: values in the canonical mask M's order."""
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    cols = M.indices
    assert got.shape == (M.nnz,)
    want, stored = W[rows, cols], S[rows, cols]
    assert np.array_equal(got[~stored].view(np.int64), np.zeros(int((~stored).sum()), dtype=np.int64)), \
        "a mask position no product reaches is not +0.0"
    g, w = got[stored], want[stored]
    if exact:
        assert np.array_equal(g.view(np.int64), w.view(np.int64)), f"values differ bitwise (max rel {rel_err(g, w):.3e})"
    else:
        mag = np.asarray((abs(A) @ abs(B))[rows[stored], cols[stored]]).ravel()
        assert np.all(np.abs(g - w) <= RTOL * mag), f"values: max rel {rel_err(g, w):.3e}"


# ------------------------------------------------------------------------------ sparse triple product against the oracle
def _ones(m):
    m = m.copy()
    m.data = np.ones_like(m.data)
    return m


def triple_pattern(H, Q, row_begin=0, row_end=None):
    """(indptr, indices) of triu(Hb @ Qb @ Hb.T)[row_begin:row_end], canonical."""
    n = H.shape[0]
    row_end = n if row_end is None else row_end
    Hb, Qb = _ones(H), _ones(Q)
    P = sp.triu((Hb @ Qb @ Hb.T).tocsr()).tocsr()[row_begin:row_end]
    P.sum_duplicates()
    P.sort_indices()
    return P.indptr.astype(np.int64), P.indices


def check_triple_sparse(res, H, Q, want, exact, row_begin=0, row_end=None):
    """res: (indptr, indices, data) of rows [row_begin, row_end); want: the oracle's dense n x n triple (full=0)."""
    n = H.shape[0]
    row_end = n if row_end is None else row_end
    ptr, idx, val = res
    pp, pi = triple_pattern(H, Q, row_begin, row_end)
    assert np.array_equal(ptr, pp), "indptr differs from the structural pattern"
    assert np.array_equal(idx.astype(np.int64), pi.astype(np.int64)), "indices differ from the structural pattern"
    for i in range(row_end - row_begin):
        assert np.all(np.diff(idx[ptr[i]:ptr[i + 1]]) > 0), f"row {i}: columns not strictly ascending"
    rows = np.repeat(np.arange(row_begin, row_end), np.diff(ptr))
    w = want[rows, idx]
    if exact:
        assert np.array_equal(val.view(np.int64), w.view(np.int64)), f"values differ bitwise (max rel {rel_err(val, w):.3e})"
    else:
        # relative to the sum of the magnitudes of the terms (signed values cancel: a near-zero sum has no own scale)
        mag = (abs(H) @ abs(Q) @ abs(H).T).toarray()[rows, idx]
        assert np.all(np.abs(val - w) <= RTOL * mag), f"values: max rel {rel_err(val, w):.3e}"
    stored = np.zeros((row_end - row_begin, n), dtype=bool)
    stored[rows - row_begin, idx] = True
    upper = np.triu(np.ones((n, n), dtype=bool))[row_begin:row_end]
    assert not np.any(want[row_begin:row_end][upper & ~stored]), "a nonzero of the oracle is missing from the pattern"


# ------------------------------------------------------------------------------ masked triple product against the oracle
def upper_mask(L, row_begin=0, row_end=None):
    L = L.tocsr().copy()
    L.sum_duplicates()
    U = sp.triu(L, format="csr")
    U.sort_indices()
    row_end = L.shape[0] if row_end is None else row_end
    return U[row_begin:row_end]


def check_triple_masked(res, U, want, H, Q, exact, row_begin=0):
    ptr, idx, val = res
    assert np.array_equal(ptr.astype(np.int64), U.indptr.astype(np.int64)), "indptr is not triu(L)'s"
    assert np.array_equal(idx.astype(np.int64), U.indices.astype(np.int64)), "indices are not triu(L)'s"
    rows = np.repeat(np.arange(U.shape[0]), np.diff(U.indptr)) + row_begin
    w = want[rows, idx]
    if exact:
        assert np.array_equal(val.view(np.int64), w.view(np.int64)), f"values differ bitwise (max rel {rel_err(val, w):.3e})"
    else:
        mag = (abs(H) @ abs(Q) @ abs(H).T).toarray()[rows, idx]
        assert np.all(np.abs(val - w) <= RTOL * mag), f"values: max rel {rel_err(val, w):.3e}"
    if exact:                                                  # positions the oracle holds as zero are zeros
        assert np.array_equal(val[w == 0].view(np.int64) & np.int64(0x7FFFFFFFFFFFFFFF), np.zeros(int((w == 0).sum()), np.int64))
