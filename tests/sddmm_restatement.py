"""The contract of the sampled dense product restated in numpy, and the operands its tests share.

Entry p = (i, j) of the mask, in the mask's stored order:
  exact     s = +0.0; s = s + X[i, e] * Y[j, e] for e = 0 .. k-1, every product rounded before its add.
  default   NP = 2 G with G = ceil(k / 2) rounded up to a power of two in [4, 64]; partial q of NP starts at +0.0 and takes
            s[q] = fma(X[i, e], Y[j, e], s[q]) for e = q, q + NP, ... in ascending e; then s[q] = s[q] + s[q + h] for every
            q that is a multiple of 2 h, for h = 1, 2, 4, ..., NP / 2; the result is s[0].
With scale the stored value is w[p] * s, the multiply always carried out."""
import functools

import numpy as np
import scipy.sparse as sp


def entries(mask):
    """(rows, cols, weights) of the stored entries of a CSR, in stored order (repeats stay)."""
    ptr = np.asarray(mask.indptr, dtype=np.int64)
    nnz = int(ptr[-1])
    rows = np.repeat(np.arange(mask.shape[0]), np.diff(ptr))
    return rows, np.asarray(mask.indices[:nnz], dtype=np.int64), np.asarray(mask.data[:nnz], dtype=np.float64)


def restate_exact(X, Y, rows, cols, weights=None):
    """The exact contract, vectorised over the entries: one rounded product and one add per e."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    s = np.zeros(len(rows))
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(X.shape[1]):
            prod = X[rows, e] * Y[cols, e]
            s = s + prod
        return s if weights is None else weights * s


def partials(k):
    """NP of the default mode's order: it depends on k alone."""
    g = 4
    while g < 64 and 2 * g < k:
        g *= 2
    return 2 * g


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a * b + c) with one rounding, for finite arrays far from overflow and underflow (Boldo and Melquiond,
    "Emulation of FMA and correctly rounded sums", 2008): a * b and the sums are split without error, the two low parts
    are added with rounding to odd, and the last add rounds once."""
    a, b, c = (np.asarray(t, dtype=np.float64) for t in (a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    s, err = _two_sum(tl, vl)
    bits = np.array(s, dtype=np.float64, copy=True).view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)                       # inexact and even: one step towards the error
    bits = np.where(fix, np.where((err > 0) == (s > 0), bits + 1, bits - 1), bits)
    return vh + bits.view(np.float64)


def restate_default(X, Y, rows, cols, weights=None):
    """The documented default-mode order, vectorised over the entries (finite operands)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    k, npart = X.shape[1], partials(X.shape[1])
    s = np.zeros((len(rows), npart))
    for e in range(k):
        q = e % npart
        s[:, q] = fma(X[rows, e], Y[cols, e], s[:, q])
    h = 1
    while h < npart:
        s[:, ::2 * h] = s[:, ::2 * h] + s[:, h::2 * h]
        h *= 2
    return s[:, 0] if weights is None else weights * s[:, 0]


def bound(X, Y, rows, cols, weights=None):
    """(|X| |Y|^T)[i, j] per entry, times |w| when scaled: what the default mode's 1e-10 is relative to."""
    b = np.einsum("pe,pe->p", np.abs(X)[rows], np.abs(Y)[cols]) if len(rows) else np.zeros(0)
    return b if weights is None else np.abs(weights) * b


def raw_csr(indptr, indices, data, shape):
    """A CSR on exactly these arrays (no sort, no merge of repeated columns)."""
    M = sp.csr_matrix(shape, dtype=np.float64)
    M.data, M.indices, M.indptr = (np.asarray(data, np.float64), np.asarray(indices, np.int32), np.asarray(indptr, np.int32))
    M.has_sorted_indices = False
    M.has_canonical_format = False
    return M


def dense(rows, k, seed):
    """rows x k of signed values with exact zeros, negative zeros and a wide range of magnitudes."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((rows, k)) * 10.0 ** rng.integers(-3, 4, (rows, k))
    A[rng.random((rows, k)) < 0.05] = 0.0
    A[rng.random((rows, k)) < 0.02] = -0.0
    return A


KS = [1, 2, 3, 8, 63, 64, 65, 130, 257]


@functools.lru_cache(maxsize=None)
def masks():
    """name -> CSR mask with weights (signed, some zero).  All canonical but 'noncanonical'; m, n <= 600."""
    rng = np.random.default_rng(77)
    out = {}

    def weigh(M):
        M = M.tocsr()
        M.sort_indices()
        M.data = rng.uniform(-2, 2, M.nnz)
        M.data[rng.random(M.nnz) < 0.05] = 0.0
        return M

    out["empty"] = sp.csr_matrix((120, 90))
    E = sp.random(400, 350, density=0.03, format="lil", random_state=rng)
    E[::3] = 0
    E[390:] = 0
    out["empty_rows"] = weigh(E)
    out["identity"] = weigh(sp.identity(513, format="csr"))
    r = np.repeat(np.arange(600), 2)
    c = np.stack([rng.integers(0, 250, 600), rng.integers(250, 500, 600)], axis=1).ravel()
    out["two_per_row"] = weigh(sp.csr_matrix((np.ones(1200), (r, c)), shape=(600, 500)))
    n = 500
    out["band"] = weigh(sp.diags([np.ones(n - abs(d)) for d in range(-9, 10)], list(range(-9, 10)), format="csr"))
    out["random"] = weigh(sp.random(577, 431, density=0.05, format="csr", random_state=rng))
    A = sp.lil_matrix((300, 300))
    A.setdiag(1.0)
    A[0, :] = 1.0
    A[:, 0] = 1.0
    out["arrow"] = weigh(A)
    # unsorted rows, repeated positions, an empty row at either end and in the middle
    lens = rng.integers(0, 12, 150)
    lens[[0, 70, 149]] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)])
    idx = rng.integers(0, 20, int(ptr[-1]))
    out["noncanonical"] = raw_csr(ptr, idx, rng.uniform(-2, 2, idx.size), (150, 170))
    return out


def operands(name, k):
    """(mask, X, Y) of one named mask at width k; square masks get Y = X (the covariance case) for odd-numbered k."""
    M = masks()[name]
    m, n = M.shape
    X = dense(m, k, 1000 + k)
    Y = X if (m == n and k % 2 == 1) else dense(n, k, 2000 + k)
    return M, X, Y
