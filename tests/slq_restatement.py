"""Stochastic Lanczos quadrature for log det(H Q H^T + R), restated in numpy: the probes of smm_probe_fill, the CG of
tests/cg_restatement.py with its coefficients recorded (the contract of smm_innovation_solve_coef, include/smm_hip.h) and the
tridiagonal quadrature of innovation_logdet.

restate_cg_coef is restate_cg's loop -- restate_dot and an apply in stored order, every update a rounded multiply followed
by an add -- so its X, info, alpha and beta are the SMM_EXACT result bit for bit.  The quadrature uses numpy.linalg.eigh
(LAPACK) and is compared by tolerance, never by bits."""
import functools
import types

import numpy as np

from cg_restatement import BREAKDOWN, CONVERGED, LIMIT, diag_csr, restate_apply, restate_dot, system

MASK = (1 << 64) - 1


def probe_bits(seed, i, c):
    """The mixed word z of entry (i, c) in Python integers: the contract as the header states it."""
    z = (seed + c * 0xD1B54A32D192ED03 + (i + 1) * 0x9E3779B97F4A7C15) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def restate_probes(n, k, seed):
    """n x k float64 of +-1.0: -1.0 iff bit 63 of z is set.  numpy uint64 arrays wrap around silently."""
    u = np.uint64
    i = np.arange(1, n + 1, dtype=u)[:, None]
    c = np.arange(k, dtype=u)[None, :]
    z = np.array([seed & MASK], dtype=u) + c * u(0xD1B54A32D192ED03) + i * u(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    return np.where((z >> u(63)) == u(1), -1.0, 1.0)


def restate_cg_coef(H, Q, R, D, tol=1e-8, maxiter=1000, apply=None):
    """(Z, info): restate_cg with info.alpha and info.beta, maxiter x k, row it - 1: alpha where the column does not break
    down in iteration it, beta where it does not converge in it, +0.0 elsewhere.  apply(P) is (S + R) P; the default is
    restate_apply(H, Q, R, P)."""
    if apply is None:
        apply = lambda P: restate_apply(H, Q, R, P)  # noqa: E731
    D = np.asarray(D, np.float64)
    d2 = D.reshape(D.shape[0], -1)
    n, k = d2.shape
    x, r, p = np.zeros((n, k)), d2.copy(), d2.copy()
    iterations, status = np.zeros(k, np.int32), np.full(k, LIMIT, np.int32)
    ha, hb = np.zeros((maxiter, k)), np.zeros((maxiter, k))
    with np.errstate(all="ignore"):
        rho = restate_dot(r, r)
        rhs_sq, res_sq = rho.copy(), rho.copy()
        thr = (tol * tol) * rhs_sq
        frozen = rho <= thr
        status[frozen] = CONVERGED
        for it in range(1, maxiter + 1):
            if frozen.all():
                break
            w = apply(p)
            pw = restate_dot(p, w)
            for j in range(k):
                if frozen[j]:
                    continue
                if not (pw[j] > 0):
                    status[j], iterations[j], frozen[j] = BREAKDOWN, it - 1, True
                    continue
                alpha = rho[j] / pw[j]
                ha[it - 1, j] = alpha
                x[:, j] = x[:, j] + alpha * p[:, j]
                r[:, j] = r[:, j] - alpha * w[:, j]
                rho_new = restate_dot(r[:, j], r[:, j])
                res_sq[j], iterations[j] = rho_new, it
                if rho_new <= thr[j]:
                    status[j], frozen[j] = CONVERGED, True
                    continue
                beta = rho_new / rho[j]
                hb[it - 1, j] = beta
                p[:, j] = r[:, j] + beta * p[:, j]
                rho[j] = rho_new
    info = types.SimpleNamespace(iterations=iterations, status=status, residual_sq=res_sq, rhs_sq=rhs_sq, alpha=ha, beta=hb)
    return x.reshape(D.shape), info


def tridiagonal(alpha, beta, m):
    """The m x m Lanczos tridiagonal of a column with m iterations."""
    a, b = np.asarray(alpha[:m], np.float64), np.asarray(beta[:m], np.float64)
    T = np.zeros((m, m))
    for j in range(m):
        T[j, j] = 1.0 / a[j] + (b[j - 1] / a[j - 1] if j else 0.0)
        if j + 1 < m:
            T[j, j + 1] = T[j + 1, j] = np.sqrt(b[j]) / a[j]
    return T


def quadrature(alpha, beta, m, n):
    """(n e_1^T ln(T) e_1, the Ritz values ascending)."""
    theta, V = np.linalg.eigh(tridiagonal(alpha, beta, m))
    return n * float(np.sum(V[0] ** 2 * np.log(theta))), theta


def slq(info, n):
    """(samples, logdet, stderr, ritz_min, ritz_max) of the columns of info."""
    k = len(info.iterations)
    out = [quadrature(info.alpha[:, c], info.beta[:, c], int(info.iterations[c]), n) for c in range(k)]
    samples = np.array([s for s, _ in out])
    stderr = float(np.std(samples, ddof=1) / np.sqrt(k)) if k > 1 else float("nan")
    return samples, float(samples.mean()), stderr, min(t[0] for _, t in out), max(t[-1] for _, t in out)


@functools.lru_cache(maxsize=None)
def dense_log(name):
    """(lam, V, slogdet) of the dense Psi = H Q H^T + diag(r) of a named system of cg_restatement."""
    H, Q, r = system(name)
    lam, V = np.linalg.eigh((H @ Q @ H.T).toarray() + np.diag(r))
    return lam, V, float(np.sum(np.log(lam)))


def exact_samples(name, Z):
    """z_c^T ln(Psi) z_c per column of Z from the dense eigen-decomposition."""
    lam, V, _ = dense_log(name)
    return np.sum((V.T @ Z) ** 2 * np.log(lam)[:, None], axis=0)


@functools.lru_cache(maxsize=None)
def restated_slq(name, probes, seed, tol=1e-8, maxiter=1000):
    """(Z, info) of the restated CG on the probes of a named system; shared by the tests, never modified."""
    H, Q, r = system(name)
    Z = restate_probes(H.shape[0], probes, seed)
    return Z, restate_cg_coef(H, Q, diag_csr(r), Z, tol, maxiter)[1]
