"""log det(H Q H^T + R) by stochastic Lanczos quadrature (innovation_logdet) and the recording solve under it, against the
plain solve of the parent commit.  One JSON line, appended to $OUT/logdet_bench.jsonl (default profiles/).

    python scripts/logdet_bench.py --parent DIR [--reps R] [--probes 16,32] [--workloads cg,kron]
    python scripts/logdet_bench.py --only new --workloads cg --probes 16 --reps 1          (what a profiler wraps)

Workloads (one MI355X; operands pinned, probes and solutions in HBM; tol = 1e-8, maxiter = 1000):
  cg    scripts/cg_bench.py's system: H 200 000 x 1 000 000 (8 per row), Q banded half-width 32, R the dominant diagonal.
  kron  scripts/kron_bench.py's system with the banded D: Q = D (x) E applied through its factors.
The right-hand sides are the +-1 probes of smm_probe_fill, seed 12345: filled on the device in this tree, by the same hash
in numpy and uploaded in the parent's child -- the same columns on both sides.
  new     the tree this script lives in: (coef) Context.innovation_solve_coef[_kron]_into, the recording solve -- wall per
          solve and per iteration, and the HIP-event sum of every launch of one more solve; (solve) this tree's
          Context.innovation_solve[_kron]_into on the same columns; (logdet) innovation_logdet end to end and the host
          quadrature (matrix_ops._slq_result) on its own.
  parent  a child process that imports the package from DIR -- a checkout of the parent commit with its own library, so the
          code under test never times itself: Context.innovation_solve[_kron]_into on the same columns.
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
TOL, MAXITER, SEED = 1e-8, 1000, 12345


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "spread": [round(float(min(ms)), 3), round(float(max(ms)), 3)]}


def per_iteration(ms, iters):
    return {"median": round(float(np.median(ms)) / max(iters, 1), 4),
            "spread": [round(float(min(ms)) / max(iters, 1), 4), round(float(max(ms)) / max(iters, 1), 4)]}


def probes_numpy(n, k, seed):
    """The hash of include/smm_hip.h (smm_probe_fill) in numpy uint64, for the tree that has no smm_probe_fill."""
    u = np.uint64
    i = np.arange(1, n + 1, dtype=u)[:, None]
    c = np.arange(k, dtype=u)[None, :]
    z = np.array([seed % (1 << 64)], dtype=u) + c * u(0xD1B54A32D192ED03) + i * u(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    return np.where((z >> u(63)) == u(1), -1.0, 1.0)


def system(root, workload):
    """(operands, kron): scipy (H, Q, R) or (H, D, E, R), built by the helpers of `root`'s own scripts/."""
    sys.path.insert(0, os.path.join(root, "scripts"))
    import sparse_matrix_mult_amd
    assert os.path.abspath(sparse_matrix_mult_amd.__file__).startswith(os.path.abspath(root) + os.sep), sparse_matrix_mult_amd.__file__
    if workload == "cg":
        import cg_bench
        return cg_bench.operands(root), False
    import kron_bench
    H, E = kron_bench.workload(root)
    D = kron_bench.d_factor("banded")
    return (H, D, E, sp.diags(kron_bench.dominant_r(H, D, E)).tocsr()), True


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def solve_figures(call, reps):
    info = call()                                    # warm-up (and H^T, built on first use)
    iters = int(info.iterations.max())
    ms = wall(call, reps)
    return info, {"iterations": iters, "all_converged": bool(info.converged), "ms_solve": stats(ms), "ms_per_iteration": per_iteration(ms, iters)}


def run_new(root, workloads, probes, reps):
    import torch
    import sparse_matrix_mult_amd as smm
    from sparse_matrix_mult_amd import matrix_ops
    from sparse_matrix_mult_amd.engine import default_context
    sys.path.insert(0, os.path.join(root, "scripts"))
    from triple_sparse_bench import kernel_names
    ctx = default_context()
    dev = torch.device("cuda", ctx.device)
    names = kernel_names()
    out = {}
    for workload in workloads:
        ops, kron = system(root, workload)
        n = ops[0].shape[0]
        pins = [smm.pin_operand(M) for M in ops]
        hs = [p._handle for p in pins]
        q_public = smm.KroneckerOperand(pins[1], pins[2]) if kron else pins[1]
        res = {}
        for k in probes:
            B = torch.empty((n, k), dtype=torch.float64, device=dev)
            ctx.probe_fill_into(B, k, n, k, SEED)
            assert np.array_equal(B[:4096].cpu().numpy(), probes_numpy(4096, k, SEED)), "the device probes are not the numpy hash"
            Z = torch.empty_like(B)
            if kron:
                coef = lambda: ctx.innovation_solve_coef_kron_into(*hs, B, k, k, Z, k, TOL, MAXITER)  # noqa: E731
                plain = lambda: ctx.innovation_solve_kron_into(*hs, B, k, k, Z, k, TOL, MAXITER)  # noqa: E731
            else:
                coef = lambda: ctx.innovation_solve_coef_into(*hs, B, k, k, Z, k, TOL, MAXITER)  # noqa: E731
                plain = lambda: ctx.innovation_solve_into(*hs, B, k, k, Z, k, TOL, MAXITER)  # noqa: E731
            info, fig = solve_figures(coef, reps)
            ctx.timing(True); ctx.timing_reset()
            coef()
            split = {}
            for nm in names:
                ms, calls = ctx.kernel_time(nm)
                if calls:
                    split[nm] = {"ms": round(ms, 3), "launches": int(calls)}
            ctx.timing(False)
            kern = sum(v["ms"] for v in split.values())
            fig.update({"ms_kernels_solve": round(kern, 3), "ms_kernels_per_iteration": round(kern / max(fig["iterations"], 1), 4),
                        "split": split})
            _, fig_plain = solve_figures(plain, reps)
            fill = wall(lambda: ctx.probe_fill_into(B, k, n, k, SEED), reps)
            logdet = lambda: smm.innovation_logdet(pins[0], q_public, pins[-1], probes=k, seed=SEED, tol=TOL, maxiter=MAXITER)  # noqa: E731
            r = logdet()
            e2e = wall(logdet, reps)
            quad = wall(lambda: matrix_ops._slq_result(matrix_ops.LogdetResult(), info, n), reps)
            res[f"probes{k}"] = {"coef": fig, "solve": fig_plain, "ms_probe_fill_call": stats(fill),
                                 "logdet": {"ms_end_to_end": stats(e2e), "ms_host_quadrature": stats(quad), "logdet": r.logdet,
                                            "stderr": r.stderr, "lambda_min": r.lambda_min, "lambda_max": r.lambda_max}}
            del B, Z
        out[workload] = res
        for p in pins:
            p.unpin()
    return out


def run_parent(root, workloads, probes, reps):
    import torch
    from sparse_matrix_mult_amd.engine import default_context
    ctx = default_context()
    dev = torch.device("cuda", ctx.device)
    out = {}
    for workload in workloads:
        ops, kron = system(root, workload)
        n = ops[0].shape[0]
        hs = [ctx.csr_from_scipy(M) for M in ops]
        res = {}
        for k in probes:
            B = torch.from_numpy(probes_numpy(n, k, SEED)).to(dev)
            Z = torch.empty_like(B)
            if kron:
                plain = lambda: ctx.innovation_solve_kron_into(*hs, B, k, k, Z, k, TOL, MAXITER)  # noqa: E731
            else:
                plain = lambda: ctx.innovation_solve_into(*hs, B, k, k, Z, k, TOL, MAXITER)  # noqa: E731
            res[f"probes{k}"] = {"solve": solve_figures(plain, reps)[1]}
            del B, Z
        out[workload] = res
        for hd in hs:
            hd.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit, library built: the baseline imports from it")
    ap.add_argument("--only", choices=["new", "parent"])
    ap.add_argument("--root", default=os.path.dirname(HERE), help="tree the package is imported from (child processes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--probes", default="16,32")
    ap.add_argument("--workloads", default="cg,kron")
    ap.add_argument("--timeout", type=int, default=500)
    args = ap.parse_args()
    probes, workloads = [int(w) for w in args.probes.split(",")], args.workloads.split(",")
    if args.only:
        root = os.path.abspath(args.root)
        sys.path.insert(0, root)
        print(json.dumps((run_new if args.only == "new" else run_parent)(root, workloads, probes, args.reps)))
        return
    if not args.parent:
        ap.error("--parent is required: the baseline must not be the tree under test")

    def child(role, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", role, "--root", root, "--reps", str(args.reps), "--probes", args.probes,
               "--workloads", args.workloads]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if p.returncode != 0:
            raise SystemExit(f"{role} failed ({p.returncode}):\n{p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])

    line = {"workloads": {"cg": "H 200000 x 1000000 (8 per row), Q banded half-width 32, R diagonal",
                          "kron": "Q = D (x) E: E 158 x 158 grid tapered at 4.5 steps, D banded half-width 2, p = 40, H 200000 x K"},
            "tol": TOL, "maxiter": MAXITER, "seed": SEED, "mode": "default", "reps": args.reps,
            "new": child("new", os.path.dirname(HERE)), "parent": child("parent", os.path.abspath(args.parent))}
    verdict = {}
    for w in workloads:
        for k in probes:
            new, par = line["new"][w][f"probes{k}"], line["parent"][w][f"probes{k}"]["solve"]["ms_per_iteration"]
            a, b = new["coef"]["ms_per_iteration"], new["solve"]["ms_per_iteration"]
            verdict[f"{w}_probes{k}"] = {
                "a_coef_over_parent": round(a["median"] / par["median"], 4), "a_coef_inside_parent_spread": a["median"] <= par["spread"][1],
                "b_solve_over_parent": round(b["median"] / par["median"], 4), "b_solve_inside_parent_spread": b["median"] <= par["spread"][1],
                "c_quadrature_share_of_logdet": round(new["logdet"]["ms_host_quadrature"]["median"] / new["logdet"]["ms_end_to_end"]["median"], 4)}
    line["verdict"] = verdict
    out_dir = os.environ.get("OUT", os.path.join(os.path.dirname(HERE), "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "logdet_bench.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
