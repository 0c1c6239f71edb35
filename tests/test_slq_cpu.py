"""innovation_logdet without a device: the restated probes and the restated CG with recorded coefficients
(tests/slq_restatement.py) give the quadrature the contract promises, checked against a dense eigen-decomposition; the
public function serves Psi = R on the host and refuses bad arguments before any device work."""
import numpy as np
import pytest
import scipy.sparse as sp

from sparse_matrix_mult import innovation_logdet          # (the feature: this import fails without it)

from cg_restatement import CONVERGED, diag_csr, restate_cg, rhs, system
from slq_restatement import (MASK, dense_log, exact_samples, probe_bits, restate_cg_coef, restate_probes, restated_slq, slq,
                             tridiagonal)

SEED = 12345


def test_probe_statistics():
    Z = restate_probes(2000, 32, SEED)
    assert Z.dtype == np.float64 and Z.shape == (2000, 32) and np.all(np.abs(Z) == 1.0)
    # column c does not depend on k
    wide = restate_probes(2000, 40, SEED)
    assert np.array_equal(wide[:, :32], Z)
    for c in (0, 7, 39):
        assert np.array_equal(restate_probes(2000, c + 1, SEED)[:, c], wide[:, c])
    assert np.array_equal(restate_probes(2000, 1, SEED)[:, 0], wide[:, 0])
    # the vectorised hash is the header's recipe in Python integers, large seeds included
    for seed in (0, SEED, (1 << 63) + 5, MASK):
        got = restate_probes(7, 3, seed)
        want = [[-1.0 if probe_bits(seed, i, c) >> 63 else 1.0 for c in range(3)] for i in range(7)]
        assert np.array_equal(got, want), seed
    other = restate_probes(2000, 32, SEED + 1)
    assert not np.array_equal(other, Z) and np.abs((other * Z).mean()) < 0.1
    means = np.abs(Z.mean(axis=0))
    gram = Z.T @ Z / 2000
    off = np.abs(gram - np.diag(np.diag(gram)))
    print("largest |column mean|", means.max(), "largest off-diagonal of Z^T Z / n", off.max())
    assert means.max() <= 0.1 and off.max() <= 0.1
    assert np.all(np.diag(gram) == 1.0)


def test_package_probes_are_the_restatement():
    from sparse_matrix_mult_amd.matrix_ops import _probe_signs
    for n, k, seed in ((1, 1, 0), (5, 3, SEED), (2049, 2, (1 << 63) + 5), (100, 7, -1)):
        assert np.array_equal(_probe_signs(n, k, seed), restate_probes(n, k, seed & MASK))


def test_recorded_coefficients_follow_the_contract():
    """restate_cg_coef is restate_cg plus recording; a column with m iterations has m alphas, m - 1 betas when it
    converged and m when it hit the limit; a zero column has none."""
    H, Q, r = system("small")
    R = diag_csr(r)
    D = rhs(H.shape[0], 3, 11, zero_column=1)
    want = restate_cg(H, Q, R, D, 1e-8, 1000)
    Z, info = restate_cg_coef(H, Q, R, D, 1e-8, 1000)
    assert np.array_equal(Z, want[0])
    for f in ("iterations", "status", "residual_sq", "rhs_sq"):
        assert np.array_equal(getattr(info, f), getattr(want[1], f)), f
    assert np.all(info.status == CONVERGED) and info.iterations[1] == 0
    for j in range(3):
        m = info.iterations[j]
        assert np.count_nonzero(info.alpha[:, j]) == m and np.all(info.alpha[:m, j] > 0)
        assert np.count_nonzero(info.beta[:, j]) == max(m - 1, 0) and np.all(info.beta[:max(m - 1, 0), j] > 0)
    _, lim = restate_cg_coef(H, Q, R, D, 1e-8, 5)
    assert lim.iterations.tolist() == [5, 0, 5] and lim.alpha.shape == (5, 3)
    assert np.all(lim.alpha[:, [0, 2]] > 0) and np.all(lim.beta[:, [0, 2]] > 0) and not lim.alpha[:, 1].any() and not lim.beta[:, 1].any()
    assert np.array_equal(lim.alpha, info.alpha[:5]) and np.array_equal(lim.beta, info.beta[:5])


def test_quadrature_against_a_dense_eigendecomposition():
    Z, info = restated_slq("small", 8, SEED)
    n = Z.shape[0]
    lam, _, logdet = dense_log("small")
    samples, est, stderr, lo, hi = slq(info, n)
    want = exact_samples("small", Z)
    rel = np.abs(samples - want) / np.abs(want)
    print("iterations", info.iterations.tolist(), "largest relative error of a sample", rel.max())
    print("logdet", logdet, "estimate", est, "+-", stderr, "error in standard errors", (est - logdet) / stderr)
    assert np.all(info.status == CONVERGED)
    assert np.all(rel <= 1e-10)
    assert abs(est - logdet) <= 3 * stderr


def test_ritz_values_lie_in_the_spectrum():
    Z, info = restated_slq("small", 8, SEED)
    lam, _, _ = dense_log("small")
    tops = []
    for c in range(8):
        m = int(info.iterations[c])
        theta = np.linalg.eigvalsh(tridiagonal(info.alpha[:, c], info.beta[:, c], m))
        assert theta[0] >= lam[0] * (1 - 1e-8) and theta[-1] <= lam[-1] * (1 + 1e-8), (c, theta[0], theta[-1])
        tops.append(theta[-1])
    print("lambda_max", lam[-1], "largest Ritz value", max(tops), "smallest Ritz / lambda_min", lo_ratio(info, lam))
    assert abs(max(tops) - lam[-1]) <= 1e-8 * lam[-1]


def lo_ratio(info, lam):
    return min(np.linalg.eigvalsh(tridiagonal(info.alpha[:, c], info.beta[:, c], int(info.iterations[c])))[0]
               for c in range(len(info.iterations))) / lam[0]


def test_host_path_through_the_public_interface():
    """H without entries: Psi = R = diag(r) with three distinct values, so every probe is exact after 3 iterations
    (z_i^2 = 1: the probe weighs every eigenvalue by its multiplicity)."""
    from sparse_matrix_mult_amd import innovation_logdet as same
    assert innovation_logdet is same
    r = np.repeat([0.5, 2.0, 7.0], 100)
    H0, Q = sp.csr_matrix((300, 40)), sp.identity(40, format="csr")
    want = float(np.sum(np.log(r)))
    res = innovation_logdet(H0, Q, r, probes=8, seed=SEED)
    print(res)
    assert res.samples.shape == (8,) and np.all(np.abs(res.samples - want) <= 1e-12 * abs(want))
    assert abs(res.logdet - want) <= 1e-12 * abs(want) and res.stderr <= 1e-9
    assert res.info.iterations.tolist() == [3] * 8 and res.info.converged and res.positive_definite
    assert res.info.alpha.shape == (300, 8) and np.count_nonzero(res.info.alpha) == 24 and np.count_nonzero(res.info.beta) == 16
    assert abs(res.lambda_min - 0.5) <= 1e-12 and abs(res.lambda_max - 7.0) <= 1e-11
    assert res.Z is None and res.info_d is None and res.solutions is None
    # the recorded host iteration is the restatement's, bit for bit
    Zp = restate_probes(300, 8, SEED)
    _, winfo = restate_cg_coef(H0, Q, diag_csr(r), Zp, 1e-8, 300)
    assert np.array_equal(res.info.alpha, winfo.alpha) and np.array_equal(res.info.beta, winfo.beta)
    # right-hand sides in front of the probes, and the solutions
    D = rhs(300, 2, 5)
    res2 = innovation_logdet(H0, sp.csr_matrix((40, 40)), sp.diags(r).tocsr(), probes=8, seed=SEED, d=D, return_solutions=True)
    assert np.array_equal(res2.samples, res.samples)
    assert res2.Z.shape == (300, 2) and np.allclose(res2.Z, D / r[:, None], rtol=1e-8) and res2.info_d.iterations.shape == (2,)
    assert res2.solutions.shape == (300, 8) and np.allclose(res2.solutions, Zp / r[:, None], rtol=1e-8)
    z1 = innovation_logdet(H0, Q, r, probes=1, seed=SEED, d=D[:, 0])
    assert z1.Z.shape == (300,) and np.isnan(z1.stderr) and z1.logdet == res.samples[0]
    # an indefinite R: breakdown is reported, not raised
    bad = innovation_logdet(H0, Q, -r, probes=4)
    assert np.isnan(bad.logdet) and not bad.positive_definite and bad.info.status.tolist() == [2] * 4
    # a limit of two iterations: the two-point quadrature, and info says so
    lim = innovation_logdet(H0, Q, r, probes=4, maxiter=2)
    assert lim.info.status.tolist() == [1] * 4 and not lim.info.converged and np.all(np.isfinite(lim.samples))
    assert np.count_nonzero(lim.info.alpha) == 8 and np.count_nonzero(lim.info.beta) == 8
    # n = 0
    empty = innovation_logdet(sp.csr_matrix((0, 40)), Q, None, probes=3)
    assert empty.logdet == 0.0 and empty.samples.tolist() == [0.0] * 3


def test_argument_errors():
    H = sp.random(30, 50, density=0.2, format="csr", random_state=np.random.default_rng(1))
    Q = sp.identity(50, format="csr")
    r = np.ones(30)
    H0 = sp.csr_matrix((30, 50))
    bad = [
        (H, Q, r, {"probes": 0}), (H, Q, r, {"probes": -3}), (H, Q, r, {"probes": 2.5}), (H, Q, r, {"probes": "many"}),
        (H0, Q, None, {}),                                                         # Psi = 0: singular
        (H0, Q, sp.csr_matrix((30, 30)), {}),
        (H, sp.identity(49, format="csr"), r, {}),                                 # H, Q do not fit
        (H, sp.random(50, 40, density=0.1, format="csr"), r, {}),                  # Q not square
        (H, Q, np.ones(29), {}), (H, Q, sp.identity(31, format="csr"), {}),        # R of the wrong size
        (H, Q, r, {"d": np.ones((31, 2))}), (H, Q, r, {"d": np.ones((30, 2, 2))}),
        (H, Q, r, {"tol": 0.0}), (H, Q, r, {"tol": float("nan")}),
        (H, Q, r, {"maxiter": 0}), (H, Q, r, {"maxiter": 65537}), (H, Q, r, {"maxiter": 2.5}),
        (H, Q, r, {"seed": "x"}),
    ]
    for h, q, rr, kw in bad:
        with pytest.raises(ValueError):
            innovation_logdet(h, q, rr, **kw)
