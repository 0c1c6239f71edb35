"""The contract of innovation_solve restated in numpy, and the operands its tests share.

Conjugate gradients on (H Q H^T + R) Z = D from x0 = 0, one CG per column (include/smm_hip.h states the iteration).  The
three products are the stored-order loop of tests/spmm_restatement.py; every vector update is a rounded multiply followed
by an add or subtract; dot(u, v) keeps LANES partial sums (partial t adds u[i] v[i] for i = t, t + LANES, ... in ascending
i, from +0.0) and combines them by the tree s[t] = s[t] + s[t + h], h = LANES/2 .. 1.  numpy never fuses a multiply with
an add, so this file is the SMM_EXACT result bit for bit."""
import functools
import os
import re
import types

import numpy as np
import scipy.sparse as sp

from spmm_restatement import restate_spmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = int(re.search(r"^#define\s+SMM_CG_LANES\s+(\d+)", open(os.path.join(ROOT, "include", "smm_hip.h")).read(), re.M).group(1))
CONVERGED, LIMIT, BREAKDOWN = 0, 1, 2


def restate_dot(u, v, lanes=LANES):
    """dot(u, v) per column (u, v: n or n x k) in the specified order."""
    u2, v2 = np.asarray(u, np.float64), np.asarray(v, np.float64)
    u2, v2 = u2.reshape(u2.shape[0], -1), v2.reshape(v2.shape[0], -1)
    s = np.zeros((lanes, u2.shape[1]))
    for i0 in range(0, u2.shape[0], lanes):              # row i0 + t goes to partial t
        m = min(lanes, u2.shape[0] - i0)
        s[:m] = s[:m] + u2[i0:i0 + m] * v2[i0:i0 + m]
    h = lanes // 2
    while h >= 1:
        s = s[:h] + s[h:2 * h]
        h //= 2
    return s[0] if np.ndim(u) > 1 else s[0, 0]


def diag_csr(r):
    """The diagonal matrix of the vector r as a CSR that stores every entry (zeros included)."""
    n = len(r)
    return sp.csr_matrix((np.asarray(r, np.float64), np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32)), shape=(n, n))


def restate_apply(H, Q, R, P):
    """(S + R) P: three stored-order products, then one add per element."""
    W = restate_spmm(H, restate_spmm(Q, restate_spmm(H, P, True)))
    return W if R is None else W + restate_spmm(R, P)


def restate_cg(H, Q, R, D, tol=1e-8, maxiter=None):
    """(Z, info): info has iterations, status (int32), residual_sq, rhs_sq, one entry per column.  R: CSR or None."""
    D = np.asarray(D, np.float64)
    d2 = D.reshape(D.shape[0], -1)
    n, k = d2.shape
    maxiter = n if maxiter is None else maxiter
    x, r, p = np.zeros((n, k)), d2.copy(), d2.copy()
    iterations, status = np.zeros(k, np.int32), np.full(k, LIMIT, np.int32)
    with np.errstate(all="ignore"):
        rho = restate_dot(r, r)
        rhs_sq, res_sq = rho.copy(), rho.copy()
        thr = (tol * tol) * rhs_sq
        frozen = rho <= thr
        status[frozen] = CONVERGED
        for it in range(1, maxiter + 1):
            if frozen.all():
                break
            w = restate_apply(H, Q, R, p)
            pw = restate_dot(p, w)
            for j in range(k):                           # columns are independent: one at a time, as the contract reads
                if frozen[j]:
                    continue
                if not (pw[j] > 0):
                    status[j], iterations[j], frozen[j] = BREAKDOWN, it - 1, True
                    continue
                alpha = rho[j] / pw[j]
                x[:, j] = x[:, j] + alpha * p[:, j]
                r[:, j] = r[:, j] - alpha * w[:, j]
                rho_new = restate_dot(r[:, j], r[:, j])
                res_sq[j], iterations[j] = rho_new, it
                if rho_new <= thr[j]:
                    status[j], frozen[j] = CONVERGED, True
                    continue
                beta = rho_new / rho[j]
                p[:, j] = r[:, j] + beta * p[:, j]
                rho[j] = rho_new
    info = types.SimpleNamespace(iterations=iterations, status=status, residual_sq=res_sq, rhs_sq=rhs_sq)
    return x.reshape(D.shape), info


def true_residual(H, Q, R, Z, D):
    """||(S + R) z - d|| / ||d|| per column with scipy in float64 (0 for a zero column with a zero z)."""
    Z2, D2 = np.asarray(Z).reshape(Z.shape[0], -1), np.asarray(D).reshape(D.shape[0], -1)
    W = H @ (Q @ (H.T @ Z2))
    if R is not None:
        W = W + R @ Z2
    num, den = np.linalg.norm(W - D2, axis=0), np.linalg.norm(D2, axis=0)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), num)


def local_h(n, K, seed):
    """8 entries per row inside a window of 16 columns, values in (-1, 1), columns ascending."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(8, K - 8, size=n)
    off = np.argsort(rng.random((n, 16)), axis=1)[:, :8]
    cols = np.sort(centre[:, None] - 8 + off, axis=1).astype(np.int32)
    return sp.csr_matrix((rng.uniform(-1, 1, 8 * n), cols.ravel(), np.arange(0, 8 * n + 1, 8, dtype=np.int32)), shape=(n, K))


def gaussian_band(K, w):
    """Symmetric band of half-width w whose entries decay like a Gaussian of the offset (sigma = w / 3)."""
    offs = list(range(-w, w + 1))
    return sp.diags([np.full(K - abs(o), np.exp(-0.5 * (3.0 * o / w) ** 2)) for o in offs], offs, shape=(K, K), format="csr")


def random_band(K, w, seed):
    """Symmetric band of half-width w with entries in (-1, 1) (indefinite: a solve needs an R that dominates)."""
    rng = np.random.default_rng(seed)
    B = sp.diags([rng.uniform(-1, 1, K - abs(d)) for d in range(-w, w + 1)], list(range(-w, w + 1)), shape=(K, K), format="csr")
    return ((B + B.T) * 0.5).tocsr()


def dominant_diagonal(H, Q, seed):
    """r with r[i] = sum_j |S|[i, j] bound + U(0.5, 1.5): (|H| (|Q| (|H|^T 1)))[i] bounds row i of |H Q H^T|, so S + diag(r)
    is strictly diagonally dominant with a positive diagonal, hence positive definite (Gershgorin), whatever Q is."""
    g = abs(H) @ (abs(Q) @ (abs(H).T @ np.ones(H.shape[0])))
    return g + np.random.default_rng(seed).uniform(0.5, 1.5, H.shape[0])


CASES = {"small": (2000, 8000, 8, 0.5, 1.5), "wide": (5000, 20000, 32, 0.5, 1.5), "stiff": (3000, 6000, 8, 0.05, 0.15)}


@functools.lru_cache(maxsize=None)
def system(name):
    """(H, Q, r) of a named case: n x K, Q's half-width, R's diagonal r ~ U(lo, hi).  S + R is positive definite."""
    n, K, w, lo, hi = CASES[name]
    seed = sorted(CASES).index(name)
    return local_h(n, K, 100 + seed), gaussian_band(K, w), np.random.default_rng(200 + seed).uniform(lo, hi, n)


def rhs(n, k, seed, zero_column=None):
    """k right-hand sides; column zero_column is all zeros."""
    D = np.random.default_rng(seed).standard_normal((n, k))
    if zero_column is not None:
        D[:, zero_column] = 0.0
    return D
