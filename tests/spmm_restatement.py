"""The contract of the sparse x dense product restated in numpy, and the operands its tests share.

Y[i, j] starts at +0.0 and adds A[i, p] * X[col_p, j] for p in row i's stored order, one product at a time (no fused
multiply-add): the loop of scipy's csr_matvec / csr_matvecs.  A^T X is the same loop over the rows of A.tocsc()."""
import functools

import numpy as np
import scipy.sparse as sp


def op_rows(A, transpose):
    """Rows of op(A): A.T when transpose."""
    return A.shape[1] if transpose else A.shape[0]


def transpose_csr(A):
    """A^T as a CSR whose arrays are those of scipy's A.tocsc() (repeated columns stay repeated)."""
    C = A.tocsc()
    return sp.csr_matrix((C.data, C.indices, C.indptr), shape=(A.shape[1], A.shape[0]))


def restate_spmm(A, X, transpose=False):
    """op(A) @ X by the stored-order loop; X 1-D or 2-D; walks entry slot s of every row at once."""
    if transpose:
        A = transpose_csr(A)
    X = np.asarray(X, dtype=np.float64)
    x2 = X.reshape(X.shape[0], -1)
    m = A.shape[0]
    Y = np.zeros((m, x2.shape[1]))
    ptr = np.asarray(A.indptr, dtype=np.int64)
    lens = np.diff(ptr)
    order = np.argsort(-lens, kind="stable")           # rows by decreasing length: slot s touches a prefix
    sl = lens[order]
    for s in range(int(sl[0]) if m else 0):
        rows = order[:int(np.searchsorted(-sl, -s, side="left"))]     # (the rows longer than s)
        p = ptr[rows] + s
        Y[rows] = Y[rows] + A.data[p][:, None] * x2[A.indices[p]]
    return Y.reshape((m,) + X.shape[1:])


def restate_triple(H, Q, X):
    """H @ (Q @ (H.T @ X)) by three stored-order loops."""
    return restate_spmm(H, restate_spmm(Q, restate_spmm(H, X, True)))


def raw_csr(indptr, indices, data, shape):
    """A CSR on exactly these arrays (no sort, no merge of repeated columns)."""
    M = sp.csr_matrix(shape, dtype=np.float64)
    M.data, M.indices, M.indptr = (np.asarray(data, np.float64), np.asarray(indices, np.int32), np.asarray(indptr, np.int32))
    M.has_sorted_indices = False
    M.has_canonical_format = False
    return M


BOUNDARY_LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097]


@functools.lru_cache(maxsize=None)
def operands():
    """name -> CSR: uniform random, unsorted rows with repeated columns, empty rows, power-law row lengths with one row of
    100 000 entries, hypersparse, tall-skinny, one row of every boundary length.  Values signed (cancellation, signed
    zeros)."""
    rng = np.random.default_rng(2024)
    out = {}
    U = sp.random(300, 200, density=0.05, format="csr", random_state=rng)
    U.data = rng.uniform(-1, 1, U.nnz)
    out["uniform"] = U
    lens = rng.integers(0, 40, 250)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    idx = rng.integers(0, 30, int(ptr[-1]))                # 30 columns: many repeats inside a row, in any order
    out["unsorted_dup"] = raw_csr(ptr, idx, rng.uniform(-1, 1, idx.size), (250, 180))
    E = sp.random(400, 300, density=0.03, format="csr", random_state=rng).tolil()
    E[::3] = 0
    E = E.tocsr()
    E.data = rng.uniform(-1, 1, E.nnz)
    out["empty_rows"] = E
    n_pl, k_pl = 3000, 120000
    lens = np.minimum((rng.pareto(1.2, n_pl) * 3).astype(np.int64), 20000)
    lens[n_pl // 2] = 100000
    ptr = np.concatenate([[0], np.cumsum(lens)])
    idx = np.concatenate([rng.permutation(k_pl)[:ln] if ln > 5000 else rng.integers(0, k_pl, ln) for ln in lens])
    out["power_law"] = raw_csr(ptr, idx, rng.uniform(-1, 1, idx.size), (n_pl, k_pl))
    r, c = rng.integers(0, 20000, 60), rng.integers(0, 15000, 60)
    out["hypersparse"] = sp.csr_matrix((rng.uniform(-1, 1, 60), (r, c)), shape=(20000, 15000))
    T = sp.random(20000, 9, density=0.3, format="csr", random_state=rng)
    T.data = rng.uniform(-1, 1, T.nnz)
    out["tall_skinny"] = T
    # one row on either side of every length at which a kernel changes its path (class thresholds 16, 1024 and 4096,
    # batches of 64 lanes and of 8 waves x 64), and an empty one; 50 columns drawn with a power-law weight, so rows hold
    # repeats in any order and the transposed operand has rows beyond 4096 and 1024 entries too
    lens = np.array([0] + BOUNDARY_LENGTHS)[rng.permutation(len(BOUNDARY_LENGTHS) + 1)]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    wgt = 1.0 / np.arange(1, 51) ** 1.5
    idx = rng.choice(50, size=int(ptr[-1]), p=wgt / wgt.sum())
    out["boundaries"] = raw_csr(ptr, idx, rng.uniform(-1, 1, idx.size), (len(lens), 50))
    return out
