"""The contract of the Kronecker operand Q = D (x) E restated in numpy, and the system its tests share.

D is p x p', E is r x r'; row t * r + j of Q is the pair (t, j), column t' * r' + j' the pair (t', j') (include/smm_hip.h).
Build: row (t, j) holds, for a over row t of D and b over row j of E in stored order, column D.idx[a] * r' + E.idx[b] with
the one rounded product D.val[a] * E.val[b].  Apply: E first -- U[t'] = E @ X[t'] for every block t' of X, then
Y = D @ U.reshape(p', r k) -- both by the stored-order loop of tests/spmm_restatement.py.  numpy never fuses a multiply with
an add, so this file is the SMM_EXACT result bit for bit."""
import functools

import numpy as np
import scipy.sparse as sp

import cg_restatement
from cg_restatement import diag_csr, dominant_diagonal, gaussian_band, local_h, rhs
from spmm_restatement import raw_csr, restate_spmm


def restate_kron_build(D, E):
    """(indptr, indices, data) of D (x) E by the nested loop: int32, int32, float64."""
    (p, pc), (r, rc) = D.shape, E.shape
    ptr = np.zeros(p * r + 1, dtype=np.int64)
    idx, val = [], []
    with np.errstate(all="ignore"):
        for t in range(p):
            da = slice(D.indptr[t], D.indptr[t + 1])
            for j in range(r):
                eb = slice(E.indptr[j], E.indptr[j + 1])
                for a in range(da.start, da.stop):                   # a outside, b inside
                    idx.append(np.int64(D.indices[a]) * rc + E.indices[eb])
                    val.append(D.data[a] * E.data[eb])
                ptr[t * r + j + 1] = ptr[t * r + j] + (da.stop - da.start) * (eb.stop - eb.start)
    idx = np.concatenate(idx) if idx else np.empty(0, np.int64)
    val = np.concatenate(val) if val else np.empty(0, np.float64)
    return ptr.astype(np.int32), idx.astype(np.int32), np.asarray(val, np.float64)


def closed_form_indptr(D, E):
    """ptr[t r + j] = D.ptr[t] nnz(E) + len_D(t) E.ptr[j], and nnz(D) nnz(E) at the end."""
    dp, ep = np.asarray(D.indptr, np.int64), np.asarray(E.indptr, np.int64)
    nnz_e = int(ep[-1])
    body = (dp[:-1, None] * nnz_e + np.diff(dp)[:, None] * ep[None, :-1]).ravel()
    return np.concatenate([body, [int(dp[-1]) * nnz_e]])


def restate_kron_apply(D, E, X):
    """(D (x) E) @ X by the two stored-order loops, E first; X 1-D or 2-D."""
    (p, pc), (r, rc) = D.shape, E.shape
    X = np.asarray(X, dtype=np.float64)
    x3 = X.reshape(pc, rc, -1)
    k = x3.shape[2]
    # U[t'] = E @ X[t'] for every t' at once: the blocks side by side as columns (every element is its own sum)
    U = restate_spmm(E, np.ascontiguousarray(x3.transpose(1, 0, 2)).reshape(rc, pc * k)).reshape(r, pc, k)
    U = np.ascontiguousarray(U.transpose(1, 0, 2)).reshape(pc, r * k)
    Y = restate_spmm(D, U).reshape(p * r, k)
    return Y.reshape((p * r,) + X.shape[1:])


def kron_bound(D, E, X):
    """((|D| (x) |E|) |X|)[i, c]: what the default mode's 1e-10 is relative to."""
    ad = raw_csr(D.indptr, D.indices, np.abs(D.data), D.shape)
    ae = raw_csr(E.indptr, E.indices, np.abs(E.data), E.shape)
    X = np.abs(np.asarray(X, np.float64))
    return restate_kron_apply(ad, ae, X)


def restate_triple_kron(H, D, E, X):
    """H @ ((D (x) E) @ (H.T @ X)) by stored-order loops."""
    return restate_spmm(H, restate_kron_apply(D, E, restate_spmm(H, X, True)))


def restate_cg_kron(H, D, E, R, rhs_, tol=1e-8, maxiter=None):
    """cg_restatement.restate_cg with Q applied through its factors: that module's loop, its apply swapped for the call."""
    def apply(H_, Q_, R_, P):
        W = restate_triple_kron(H_, D, E, P)
        return W if R_ is None else W + restate_spmm(R_, P)

    old = cg_restatement.restate_apply
    cg_restatement.restate_apply = apply
    try:
        return cg_restatement.restate_cg(H, None, R, rhs_, tol, maxiter)
    finally:
        cg_restatement.restate_apply = old


def tridiag(p, off=0.4):
    return sp.diags([np.full(p - 1, off), np.ones(p), np.full(p - 1, off)], [-1, 0, 1], shape=(p, p), format="csr")


@functools.lru_cache(maxsize=None)
def kron_system():
    """(H, D, E, R, rhs): p = 6, r = 50, n = 400; D = tridiag(0.4, 1, 0.4), E a Gaussian band; S + R positive definite."""
    D, E = tridiag(6), gaussian_band(50, 8)
    H = local_h(400, 300, 7)
    Q = sp.kron(D, E, format="csr")
    R = diag_csr(dominant_diagonal(H, Q, 8))
    return H, D, E, R, rhs(400, 5, 9, zero_column=2)


def random_csr(rows, cols, density, seed, signed=True):
    rng = np.random.default_rng(seed)
    M = sp.random(rows, cols, density=density, format="csr", random_state=rng)
    M.data = rng.uniform(-1, 1, M.nnz) if signed else rng.uniform(0.5, 1.5, M.nnz)
    M.sort_indices()
    return M


@functools.lru_cache(maxsize=None)
def canonical_pair():
    """D 7 x 5 (density 0.5) and E 33 x 29 (0.2) with one explicitly stored zero and one empty row."""
    D, E = random_csr(7, 5, 0.5, 71), random_csr(33, 29, 0.2, 72).tolil()
    E[4] = 0
    E = E.tocsr()
    E.data[3] = 0.0                                    # an explicit zero: it stays an entry
    assert E.nnz and (np.diff(E.indptr) == 0).any() and (E.data == 0).sum() == 1
    return D, E
