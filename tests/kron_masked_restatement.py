"""The contract of the masked products with Q = D (x) E restated in numpy, and the operands their tests share.

(A Q)[i, c], c = t' r' + j': over row i of A in stored order a, (t, j) = divmod(A.idx[a], r), the term A.val[a] * q with
q = D[t, t'] * E[j, j'] rounded once, taken only when both factors store their entry; the first term lands unchanged, later
ones are added one rounded product at a time.  S[i, k]: T = H Q as above ("stored" iff some a reaches it), then sum = 0.0;
sum += T[i, H.idx[a2]] * H.val[a2] over row k of H in stored order, an unstored T read as +0.0 and still multiplied
(include/smm_hip.h).  numpy never fuses a multiply with an add, so this file is the SMM_EXACT result bit for bit.  The
factors are canonical; H and A may hold unsorted rows and repeated columns."""
import functools

import numpy as np
import scipy.sparse as sp

from kron_restatement import tridiag
from spmm_restatement import operands, raw_csr


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits_nan(a, b):
    """Bit for bit, any NaN matching any NaN (the payload of a computed NaN is not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def factor_table(F):
    """(values, stored) of a canonical factor as dense arrays; an explicitly stored zero is stored."""
    assert F.has_canonical_format or all(np.all(np.diff(F.indices[F.indptr[i]:F.indptr[i + 1]]) > 0) for i in range(F.shape[0]))
    rows = np.repeat(np.arange(F.shape[0]), np.diff(F.indptr))
    val = np.zeros(F.shape)
    has = np.zeros(F.shape, dtype=bool)
    val[rows, F.indices] = F.data
    has[rows, F.indices] = True
    return val, has


def restate_aq(A, D, E):
    """(T, stored): A (D (x) E) as dense m x p'r' arrays by the first-touch loop over every row of A in stored order."""
    (p, pc), (r, rc) = D.shape, E.shape
    assert A.shape[1] == p * r
    dv, dh = factor_table(D)
    ev, eh = factor_table(E)
    m = A.shape[0]
    T = np.zeros((m, pc * rc))
    stored = np.zeros((m, pc * rc), dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(m):
            for a in range(A.indptr[i], A.indptr[i + 1]):
                t, j = divmod(int(A.indices[a]), r)
                hit = np.logical_and.outer(dh[t], eh[j]).ravel()
                q = np.multiply.outer(dv[t], ev[j]).ravel()            # one rounded multiply: the entry of D (x) E
                term = A.data[a] * q
                first = hit & ~stored[i]
                later = hit & stored[i]
                T[i, later] = T[i, later] + term[later]
                T[i, first] = term[first]
                stored[i] |= hit
    return T, stored


def positions(M):
    """(rows, cols) of a canonical pattern."""
    return np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), np.asarray(M.indices)


def restate_masked_aq(A, D, E, M):
    """The values of A (D (x) E) in the canonical mask M's order: +0.0 where no product reaches."""
    T, stored = restate_aq(A, D, E)
    rows, cols = positions(M)
    return np.where(stored[rows, cols], T[rows, cols], 0.0)


def restate_triple_at(H, T, rows, cols):
    """S[i, k] at the positions (rows, cols), from T = H Q (unstored entries +0.0): the ordered sum over row k of H."""
    out = np.empty(len(rows))
    with np.errstate(all="ignore"):
        for n, (i, k) in enumerate(zip(rows.tolist(), cols.tolist())):
            s = 0.0
            for a2 in range(H.indptr[k], H.indptr[k + 1]):
                s = s + T[i, H.indices[a2]] * H.data[a2]
            out[n] = s
    return out


def restate_masked_triple(H, D, E, U, row_begin=0):
    """The values of H (D (x) E) H^T on the pattern U = helpers.upper_mask(L, row_begin, row_end), in its order."""
    T, stored = restate_aq(H, D, E)
    T = np.where(stored, T, 0.0)
    rows, cols = positions(U)
    return restate_triple_at(H, T, rows + row_begin, cols)


def abs_csr(M):
    """|M| on arrays of its own (scipy's abs() merges repeated columns of its operand in place)."""
    return sp.csr_matrix((np.abs(M.data), np.array(M.indices), np.array(M.indptr)), shape=M.shape)


def kron_abs(D, E):
    return sp.kron(abs_csr(D), abs_csr(E), format="csr")


def aq_bound(A, D, E, M):
    """(|A| |Q|)[i, c] at the mask's positions: what the default mode's 1e-10 is relative to."""
    rows, cols = positions(M)
    return np.asarray((abs_csr(A) @ kron_abs(D, E)).toarray())[rows, cols]


def triple_bound(H, D, E, U, row_begin=0):
    """(|H| |Q| |H|^T)[i, k] at the pattern's positions."""
    rows, cols = positions(U)
    return np.asarray((abs_csr(H) @ kron_abs(D, E) @ abs_csr(H).T).toarray())[rows + row_begin, cols]


# ------------------------------------------------------------------------------ operands
def rand_rows(m, K, lens, seed, dup=False):
    """m x K CSR whose row i holds lens[i] entries: distinct ascending columns, or (dup) any columns in any order."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    idx = np.concatenate([rng.integers(0, K, ln) if dup else np.sort(rng.permutation(K)[:ln]) for ln in lens] + [np.empty(0, np.int64)])
    M = raw_csr(ptr, idx, rng.uniform(-1, 1, idx.size), (m, K))
    M.has_sorted_indices = not dup
    return M


def taper_like(r, half, seed=0):
    """A banded symmetric r x r factor with entries decaying off the diagonal (and a few signs), canonical."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(r), np.arange(r), indexing="ij")
    keep = np.abs(i - j) <= half
    val = np.exp(-0.5 * ((i - j) / max(half, 1)) ** 2) * np.where(rng.random((r, r)) < 0.1, -1.0, 1.0)
    return sp.csr_matrix((val[keep], (i[keep], j[keep])), shape=(r, r))


def dense_factor(p, seed):
    rng = np.random.default_rng(seed)
    return sp.csr_matrix(rng.uniform(-1, 1, (p, p)))


def with_explicit_zeros(F, every=5):
    F = F.copy()
    F.data[::every] = 0.0                                 # entries, not holes: they make a T "stored" and may store +-0.0
    return F


def with_empty_rows(F, rows):
    L = F.tolil()
    for i in rows:
        L[i] = 0
    out = L.tocsr()
    out.sort_indices()
    return out


def edge_factor(r):
    """A canonical r x r factor whose rows have the lengths 0, 1, 2, 64, 65 and 300 (cut to r) in turn, at columns that leave
    a gap below the first, above the last and inside: every outcome of the search -- first, last, below all, above all, in a
    gap -- occurs for some pair."""
    lens = [0, 1, 2, 64, 65, 300]
    rng = np.random.default_rng(r)
    ptr, idx = [0], []
    for i in range(r):
        ln = min(lens[i % len(lens)], r - 3)
        cols = np.sort(rng.permutation(np.arange(1, r - 1))[:ln + 1])
        cols = np.delete(cols, (ln + 1) // 2) if ln else cols[:0]     # (ln entries, and a gap inside where one was taken out)
        idx.append(cols)
        ptr.append(ptr[-1] + len(cols))
    idx = np.concatenate(idx)
    F = sp.csr_matrix((rng.uniform(-1, 1, idx.size), idx.astype(np.int32), np.asarray(ptr, np.int32)), shape=(r, r))
    assert F.has_canonical_format and F.nnz == idx.size
    return F


def band_mask(n, half):
    return sp.diags([np.ones(n - abs(o)) for o in range(-half, half + 1)], list(range(-half, half + 1)), shape=(n, n), format="csr")


def random_mask(m, n, density, seed):
    M = sp.random(m, n, density=density, format="csr", random_state=np.random.default_rng(seed))
    M.sort_indices()
    return M


H_LENGTHS = [0, 1, 8, 63, 64, 65, 300]


@functools.lru_cache(maxsize=None)
def factor_cases():
    """name -> (D, E), square and canonical: the factor shapes of the contract."""
    out = {
        "tridiag5_taper33": (tridiag(5), taper_like(33, 4)),
        "tridiag10_taper33": (tridiag(10), taper_like(33, 4, 8)),     # K = 330: the H row of 300 entries is not cut
        "dense40_e3": (dense_factor(40, 3), taper_like(3, 1, 1)),
        "d1": (sp.csr_matrix(np.array([[0.75]])), taper_like(33, 4, 2)),
        "e1": (tridiag(6), sp.csr_matrix(np.array([[-1.25]]))),
        "d_empty_rows": (with_empty_rows(tridiag(7), [0, 3]), taper_like(12, 3, 3)),
        "explicit_zeros": (with_explicit_zeros(tridiag(5), 4), with_explicit_zeros(taper_like(20, 3, 4), 5)),
        "edges_e": (tridiag(2), edge_factor(330)),
        "edges_d": (edge_factor(330), taper_like(2, 1, 5)),
    }
    for d, e in out.values():
        assert d.has_canonical_format and e.has_canonical_format
    return out


def h_for(D, E, seed=11, dup=False, lens=None):
    """An H over the columns of D (x) E with rows of every length in H_LENGTHS (cut to K), twice, so that a short row meets a
    long one on both sides of the diagonal."""
    K = D.shape[0] * E.shape[0]
    lens = [min(ln, K) for ln in (H_LENGTHS + H_LENGTHS[::-1] if lens is None else lens)]
    return rand_rows(len(lens), K, lens, seed, dup=dup)


def unsorted_dup_system():
    """(H, D, E): H the unsorted_dup operand of spmm_restatement (250 x 180, repeated columns in any order)."""
    return operands()["unsorted_dup"], tridiag(5), taper_like(36, 4, 6)


def special_system(kind):
    """(H, D, E, note) for kind in 'unreached', 'reached', 'negzero'.
    unreached: an inf and a NaN in H at columns whose row AND column of Q hold nothing (t = 2 is an empty row and column of
               D), in rows that store nothing else there; they meet only unstored T, so off the two rows' own diagonal entries
               they must not appear.
    reached:   an inf and a NaN in H at columns Q does store.
    negzero:   values whose products are all -0.0 or +0.0."""
    E = taper_like(6, 1, 7)
    D = tridiag(4).tolil()
    D[2] = 0
    D[:, 2] = 0
    D = D.tocsr()
    D.sort_indices()
    K = 24
    H = rand_rows(10, K, [3] * 10, 21)
    H.indices = np.where((H.indices >= 12) & (H.indices < 18), H.indices - 12, H.indices).astype(np.int32)   # nothing in block t = 2 ...
    for i in range(10):
        s = slice(H.indptr[i], H.indptr[i + 1])
        H.indices[s] = np.sort(H.indices[s])
    H = sp.csr_matrix(H.toarray())                      # (merges what the remap made equal)
    H = H.tolil()
    if kind == "unreached":
        H[3, 13] = np.inf                                 # ... but these two
        H[6, 16] = np.nan
    elif kind == "reached":
        H[3, 1] = np.inf
        H[6, 20] = np.nan
    H = H.tocsr()
    H.sort_indices()
    if kind == "negzero":
        H.data = np.where(np.arange(H.nnz) % 2 == 0, -0.0, 0.0)
        H = raw_csr(H.indptr, H.indices, H.data, H.shape)
    return H, D, E
