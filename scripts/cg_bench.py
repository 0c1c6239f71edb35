"""The device CG solve (innovation_solve) against the loop a user writes without it.  One JSON line.

    python scripts/cg_bench.py --parent DIR [--reps R] [--exact] [--widths 1,16,64]
    python scripts/cg_bench.py --only solve --widths 16 --reps 1        (what a profiler wraps)

Workload: scripts/triple_sparse_bench.py's H (200 000 x 1 000 000, 8 per row) and Q (random band, half-width 32), R the
diagonal that makes S + R strictly diagonally dominant (|H| |Q| |H|^T 1 + U(0.5, 1.5)), k right-hand sides, tol = 1e-8.
Operands pinned, D and Z in HBM.
(a) solve: innovation_solve through Context.innovation_solve_into -- wall time per solve and per iteration, and the
    HIP-event sum of every launch of one more solve (timing adds events to every launch, so it is a run of its own).
(b) baseline: the same recurrence as a torch loop over triple_product_apply, sparse_dense_multiply, torch reductions and
    axpys, run in a child process that imports the package from DIR -- a checkout of the commit before the solver, with
    its library built -- so the code under test never times itself.  The loop reads one flag per iteration, as the
    solver does, and does not freeze columns one by one (which favours it).
Every figure is the median of R repetitions with the spread (min, max)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-8


def operands(root):
    """The workload, built by the helpers of `root`'s own scripts/ (importing them imports the package from `root`)."""
    sys.path.insert(0, os.path.join(root, "scripts"))
    from triple_sparse_bench import banded_q, local_h
    import sparse_matrix_mult_amd
    assert os.path.abspath(sparse_matrix_mult_amd.__file__).startswith(os.path.abspath(root) + os.sep), sparse_matrix_mult_amd.__file__
    n, K = 200000, 1000000
    H, Q = local_h(n, K, 1), banded_q(K, 32, 2)
    g = abs(H) @ (abs(Q) @ (abs(H).T @ np.ones(n)))
    r = g + np.random.default_rng(3).uniform(0.5, 1.5, n)
    return H, Q, sp.diags(r).tocsr()


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "spread": [round(float(min(ms)), 3), round(float(max(ms)), 3)]}


def per_iteration(ms, iters):
    return stats([m / max(iters, 1) for m in ms])


def run_solve(root, widths, reps, exact):
    import torch
    H, Q, R = operands(root)
    from sparse_matrix_mult_amd.engine import default_context
    from triple_sparse_bench import kernel_names
    ctx = default_context()
    dev = torch.device("cuda", ctx.device)
    h, q, r = (ctx.csr_from_scipy(M) for M in (H, Q, R))
    names = kernel_names()
    out = {}
    for k in widths:
        D = torch.from_numpy(np.random.default_rng(4).standard_normal((H.shape[0], k))).to(dev)
        Z = torch.empty_like(D)
        call = lambda: ctx.innovation_solve_into(h, q, r, D, k, k, Z, k, TOL, exact=exact)  # noqa: E731
        info = call()                                # (builds H^T on the first width; warm-up)
        iters = int(info.iterations.max())
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.timing(True); ctx.timing_reset()
        call()
        split = {}
        for nm in names:
            ms, calls = ctx.kernel_time(nm)
            if calls:
                split[nm] = {"ms": round(ms, 3), "launches": int(calls)}
        ctx.timing(False)
        kern = sum(v["ms"] for v in split.values())
        out[f"k{k}"] = {"iterations": iters, "all_converged": bool(info.converged), "ms_solve": stats(wall),
                        "ms_per_iteration": per_iteration(wall, iters), "ms_kernels_solve": round(kern, 3),
                        "ms_kernels_per_iteration": round(kern / max(iters, 1), 4), "split": split}
        del D, Z
    for hd in (h, q, r):
        hd.close()
    return out


def run_baseline(root, widths, reps, exact):
    import torch
    H, Q, R = operands(root)
    from sparse_matrix_mult_amd import pin_operand, set_exact, set_result_device, sparse_dense_multiply, triple_product_apply
    from sparse_matrix_mult_amd.engine import default_context
    set_exact(exact)
    set_result_device(True)
    dev = torch.device("cuda", default_context().device)
    ph, pq, pr = pin_operand(H), pin_operand(Q), pin_operand(R)

    def solve(D):
        x, r = torch.zeros_like(D), D.clone()
        p = r.clone()
        rho = (r * r).sum(0)
        thr = (TOL * TOL) * rho
        it = 0
        for it in range(1, D.shape[0] + 1):
            w = triple_product_apply(ph, pq, p) + sparse_dense_multiply(pr, p)
            alpha = rho / (p * w).sum(0)
            x += alpha * p
            r -= alpha * w
            rho_new = (r * r).sum(0)
            if bool((rho_new <= thr).all()):
                break
            p = r + (rho_new / rho) * p
            rho = rho_new
        return x, it

    out = {}
    for k in widths:
        D = torch.from_numpy(np.random.default_rng(4).standard_normal((H.shape[0], k))).to(dev)
        _, iters = solve(D)
        torch.cuda.synchronize()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            solve(D)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out[f"k{k}"] = {"iterations": iters, "ms_solve": stats(wall), "ms_per_iteration": per_iteration(wall, iters)}
        del D
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the commit before the solver, library built: the baseline imports from it")
    ap.add_argument("--only", choices=["solve", "baseline"])
    ap.add_argument("--root", default=os.path.dirname(HERE), help="tree the package is imported from (child processes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--widths", default="1,16,64")
    ap.add_argument("--exact", action="store_true")
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]
    if args.only:
        root = os.path.abspath(args.root)
        sys.path.insert(0, root)
        res = (run_solve if args.only == "solve" else run_baseline)(root, widths, args.reps, args.exact)
        print(json.dumps(res))
        return
    if not args.parent:
        ap.error("--parent is required: the baseline must not be the tree under test")

    def child(role, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", role, "--root", root, "--reps", str(args.reps), "--widths", args.widths]
        p = subprocess.run(cmd + (["--exact"] if args.exact else []), capture_output=True, text=True, timeout=200)
        if p.returncode != 0:
            raise SystemExit(f"{role} failed ({p.returncode}):\n{p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])

    line = {"workload": "CG on (H Q H^T + R) Z = D: H 200000 x 1000000 (8 per row), Q banded half-width 32, R diagonal, tol 1e-8",
            "mode": "SMM_EXACT" if args.exact else "default", "reps": args.reps,
            "solve": child("solve", os.path.dirname(HERE)), "baseline_torch_loop_on_parent": child("baseline", os.path.abspath(args.parent))}
    verdict = {}
    for key, a in line["solve"].items():
        b = line["baseline_torch_loop_on_parent"][key]
        verdict[key] = {"speedup_per_iteration": round(b["ms_per_iteration"]["median"] / a["ms_per_iteration"]["median"], 2),
                        "solve_below_baseline_beyond_spread": a["ms_per_iteration"]["spread"][1] < b["ms_per_iteration"]["spread"][0]}
    line["per_iteration_a_vs_b"] = verdict
    print(json.dumps(line))


if __name__ == "__main__":
    main()
