"""innovation_solve without a device: the numpy restatement of its contract (tests/cg_restatement.py) solves the shared
systems, reports zero columns, breakdown and the iteration limit as specified, and sums dot products in the specified
order; the public function refuses bad arguments before any device work and serves S = 0 on the host."""
import functools
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from cg_restatement import (BREAKDOWN, CASES, CONVERGED, LANES, LIMIT, diag_csr, restate_cg, restate_dot, rhs, system,
                            true_residual)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _dense(name):
    """S + R as a dense matrix and its eigenvalues."""
    H, Q, r = system(name)
    dense = (H @ Q @ H.T + diag_csr(r)).toarray()
    return dense, np.linalg.eigvalsh(dense)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("tol", [1e-6, 1e-10])
def test_restatement_solves_the_shared_systems(name, tol):
    H, Q, r = system(name)
    R = diag_csr(r)
    n = H.shape[0]
    D = rhs(n, 5, 7, zero_column=2)
    Z, info = restate_cg(H, Q, R, D, tol=tol)
    print(name, tol, "iterations", info.iterations.tolist(), "status", info.status.tolist())
    assert np.all(info.status == CONVERGED), "no breakdown and no iteration limit on these operands"
    assert info.iterations[2] == 0 and np.all(Z[:, 2] == 0.0) and info.rhs_sq[2] == 0.0
    live = [0, 1, 3, 4]
    assert np.all(info.iterations[live] > 10)
    res = true_residual(H, Q, R, Z, D)
    print("true residual / tol", (res / tol).tolist())
    assert np.all(res <= tol)
    dense, lam = _dense(name)
    want = np.linalg.solve(dense, D)
    err = np.linalg.norm(Z - want, axis=0)
    print("eigenvalues", lam[0], lam[-1], "cond", lam[-1] / lam[0], "max abs error", np.max(np.abs(Z - want)))
    assert lam[0] > 0, "S + R is positive definite"
    # ||z - z*|| <= ||(S + R)^-1|| ||(S + R) z - d|| = true residual * ||d|| / lambda_min; 1e-12 ||z*|| for the dense solve itself
    assert np.all(err <= res * np.linalg.norm(D, axis=0) / lam[0] + 1e-12 * np.linalg.norm(want, axis=0))
    assert np.all(info.residual_sq <= tol * tol * info.rhs_sq)


def test_indefinite_system_reports_breakdown():
    H, Q, r = system("small")
    D = rhs(H.shape[0], 3, 8)
    Z, info = restate_cg(H, Q, diag_csr(np.full(H.shape[0], -10.0)), D, tol=1e-8, maxiter=200)
    assert BREAKDOWN in info.status.tolist()
    assert np.all(np.isfinite(Z))
    j = int(np.flatnonzero(info.status == BREAKDOWN)[0])
    assert info.iterations[j] < 200


def test_iteration_limit():
    H, Q, r = system("small")
    D = rhs(H.shape[0], 4, 9, zero_column=1)
    Z, info = restate_cg(H, Q, diag_csr(r), D, tol=1e-10, maxiter=3)
    assert info.status.tolist() == [LIMIT, CONVERGED, LIMIT, LIMIT]
    assert info.iterations.tolist() == [3, 0, 3, 3]
    Z0, info0 = restate_cg(H, Q, diag_csr(r), D, tol=1e-10, maxiter=0)
    assert info0.status.tolist() == [LIMIT, CONVERGED, LIMIT, LIMIT] and not Z0.any() and not info0.iterations.any()


def test_dot_restatement_against_fsum():
    rng = np.random.default_rng(3)
    for n in (1, 5, LANES - 1, LANES, LANES + 1, 3 * LANES + 17, 50000):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        want = math.fsum((u * v).tolist())
        scale = math.fsum(np.abs(u * v).tolist())
        assert abs(restate_dot(u, v) - want) <= 1e-12 * scale
        U, V = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
        got = restate_dot(U, V)
        for j in range(3):
            assert got[j] == restate_dot(U[:, j], V[:, j])


def test_dot_order_is_the_specified_one():
    """Hand-built vectors on which the specified order and a plain sequential sum differ (e = 2^-53; 1 + e rounds to 1)."""
    def sequential(u):
        s = 0.0
        for t in u:
            s = s + t
        return s
    e = 2.0 ** -53
    # the tree: partials 0 .. 3 hold 1, e, e, 2e.  h = 2: s[0] = 1 + e = 1, s[1] = e + 2e; h = 1: 1 + 3e = 1 + 2^-51.
    # Sequentially: 1 + e = 1, + e = 1, + 2e = 1 + 2^-52.
    u = np.zeros(LANES)
    u[:4] = 1.0, e, e, 2 * e
    ones = np.ones_like(u)
    assert sequential(u) == 1.0 + 2.0 ** -52
    assert restate_dot(u, ones) == (1.0 + e) + (e + 2 * e) == 1.0 + 2.0 ** -51
    # the lanes: rows 0 and LANES share partial 0 (e + 1 = 1), row 1 is partial 1 (e), and 1 + e = 1.
    # Sequentially: e + e = 2e, + 1 = 1 + 2^-52.
    u = np.zeros(LANES + 1)
    u[0], u[1], u[LANES] = e, e, 1.0
    assert sequential(u) == 1.0 + 2.0 ** -52
    assert restate_dot(u, np.ones_like(u)) == 1.0


def test_header_and_package_agree_on_the_lanes():
    text = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    assert int(re.search(r"#define\s+SMM_CG_LANES\s+(\d+)", text).group(1)) == LANES == 2048
    from sparse_matrix_mult_amd import matrix_ops
    assert matrix_ops.CG_LANES == LANES
    assert np.array_equal(matrix_ops._cg_dot(np.arange(5000.0)[:, None], np.ones((5000, 1))), [restate_dot(np.arange(5000.0), np.ones(5000))])


def test_value_errors_fire_without_a_device():
    from sparse_matrix_mult import innovation_solve
    from sparse_matrix_mult_amd import innovation_solve as same
    assert innovation_solve is same
    H = sp.random(30, 50, density=0.2, format="csr", random_state=np.random.default_rng(1))
    Q = sp.identity(50, format="csr")
    r = np.ones(30)
    D = np.ones((30, 2))
    bad = [
        (H, sp.random(50, 40, density=0.1, format="csr"), r, D, {}),               # Q not square
        (H, sp.identity(49, format="csr"), r, D, {}),                              # H, Q do not fit
        (H, Q, np.ones(29), D, {}),                                                # diagonal of the wrong length
        (H, Q, sp.identity(31, format="csr"), D, {}),                              # R of the wrong shape
        (H, Q, np.ones((30, 29)), D, {}),
        (H, Q, r, np.ones((31, 2)), {}),                                           # D of the wrong height
        (H, Q, r, np.ones((30, 2, 2)), {}),
        (H, Q, r, D, {"tol": 0.0}), (H, Q, r, D, {"tol": -1e-8}), (H, Q, r, D, {"tol": float("nan")}),
        (H, Q, r, D, {"tol": float("inf")}), (H, Q, r, D, {"tol": "tight"}),
        (H, Q, r, D, {"maxiter": -1}), (H, Q, r, D, {"maxiter": 2.5}),
    ]
    for h, q, rr, d, kw in bad:
        with pytest.raises(ValueError):
            innovation_solve(h, q, rr, d, **kw)


def test_degenerate_systems_are_served_on_the_host():
    from sparse_matrix_mult_amd import innovation_solve
    H = sp.random(40, 60, density=0.2, format="csr", random_state=np.random.default_rng(2))
    Q = sp.identity(60, format="csr")
    r = np.random.default_rng(3).uniform(0.5, 1.5, 40)
    Z, info = innovation_solve(H, Q, r, np.zeros((40, 0)))
    assert Z.shape == (40, 0) and info.iterations.shape == (0,) and info.status.shape == (0,)
    Z, info = innovation_solve(sp.csr_matrix((0, 60)), Q, None, np.zeros((0, 3)))
    assert Z.shape == (0, 3) and info.status.tolist() == [0, 0, 0]
    # S = 0 (H without entries): R z = d, by the same iteration
    H0 = sp.csr_matrix((40, 60))
    D = rhs(40, 3, 4, zero_column=1)
    Z, info = innovation_solve(H0, Q, r, D, tol=1e-12)
    want, winfo = restate_cg(H0, Q, diag_csr(r), D, tol=1e-12)
    assert np.array_equal(Z.view(np.int64), want.view(np.int64))
    for f in ("iterations", "status", "residual_sq", "rhs_sq"):
        assert np.array_equal(getattr(info, f), getattr(winfo, f)), f
    assert info.status.tolist() == [0, 0, 0] and np.allclose(Z, D / r[:, None], rtol=1e-10)
    z1, info1 = innovation_solve(H0, Q, sp.diags(r).tocsr(), D[:, 0], tol=1e-12)
    assert z1.shape == (40,) and np.array_equal(z1, Z[:, 0]) and info1.iterations.tolist() == [info.iterations[0]]
    # nothing at all on the left: breakdown at the first step, z = 0
    Z, info = innovation_solve(H0, Q, None, D)
    assert info.status.tolist() == [BREAKDOWN, CONVERGED, BREAKDOWN] and not Z.any() and not info.iterations.any()
