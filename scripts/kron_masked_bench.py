"""Entries of H (D (x) E) H^T and of H (D (x) E) on a given pattern, Q never formed, against what a user had without it.
One JSON line, appended to $OUT/kron_masked_bench.jsonl (default bench_out/).

    python scripts/kron_masked_bench.py --parent DIR [--reps R] [--kinds banded,dense] [--exact]
    python scripts/kron_masked_bench.py --only new --kinds dense --reps 1          (what a profiler wraps)

Workload (one MI355X): that of scripts/kron_bench.py -- E a 158 x 158-point grid tapered to 69 entries per interior row,
p = 40 periods (K = 998 560), D banded with half-width 2 or dense, H 200 000 x K with 8 entries per row.  Patterns: for the
triple product the identity (diag(S)) and a band of half-width 16; for H Q the pattern of H and a random mask of density
1e-5.  Operands and masks pinned, results left in HBM (set_result_device(True)).
  new       the tree this script lives in: sparse_triple_product(H, KroneckerOperand(D, E), mask=L) and
            masked_matrix_multiply(H, KroneckerOperand(D, E), M).  Wall time per call, and the HIP-event sum of every launch
            of one more call.
  baseline  a child process that imports the package from DIR -- a checkout of the parent commit with its own library --:
            the explicit Q = kronecker_product(D, E, pin=True) (its build is timed: 3.9 GB for the banded D), then the same
            two calls on it.  The dense D gives 2.7e9 entries, more than an operand holds: "cannot be built".
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
sys.path.insert(0, HERE)
from kron_bench import N_OBS, d_factor, stats, workload  # noqa: E402


def masks(H):
    n, K = H.shape
    band = sp.diags([np.ones(n - abs(o)) for o in range(-16, 17)], list(range(-16, 17)), shape=(n, n), format="csr")
    rng = np.random.default_rng(7)
    cnt = int(n * K * 1e-5)
    R = sp.csr_matrix((np.ones(cnt), (rng.integers(0, n, cnt), rng.integers(0, K, cnt))), shape=(n, K))
    R.sum_duplicates()
    R.sort_indices()
    pat = H.copy()
    pat.sum_duplicates()
    pat.sort_indices()
    return {"identity": sp.identity(n, format="csr"), "band16": band}, {"pattern_of_h": pat, "random_1e-5": R}


def measure(ctx, torch, names, call, reps):
    """Wall time of call() (median of reps, after a warm-up) and the HIP-event sum of the launches of one more call."""
    call(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.timing(True); ctx.timing_reset()
    call()
    torch.cuda.synchronize()
    split = {nm: round(ctx.kernel_time(nm)[0], 3) for nm in names if ctx.kernel_time(nm)[1]}
    ctx.timing(False)
    return {"ms_call": stats(ms), "ms_kernels": round(sum(split.values()), 3), "split": split}


def run(root, kinds, reps, exact, explicit):
    import torch
    H, E = workload(root)
    import sparse_matrix_mult_amd as smm
    # workload() imported the package from `root` and put root/scripts first on the path: triple_sparse_bench below is that
    # tree's module, and its kernel_names() reads that tree's smm_api.hip -- the names the library under test reports
    assert os.path.abspath(smm.__file__).startswith(os.path.abspath(root) + os.sep), smm.__file__
    from sparse_matrix_mult_amd.engine import default_context
    import triple_sparse_bench
    assert os.path.abspath(triple_sparse_bench.__file__).startswith(os.path.abspath(root) + os.sep), triple_sparse_bench.__file__
    kernel_names = triple_sparse_bench.kernel_names
    ctx = default_context()
    names = kernel_names()
    smm.set_exact(exact)
    smm.set_result_device(True)
    ph, pe = smm.pin_operand(H), smm.pin_operand(E)
    tri, aq = masks(H)
    pins = {k: smm.pin_operand(v) for k, v in {**tri, **aq}.items()}
    out = {"nnz_e": int(E.nnz), "K": int(H.shape[1]), "positions": {k: int(sp.triu(v).nnz if k in tri else v.nnz) for k, v in {**tri, **aq}.items()}}
    for kind in kinds:
        D = d_factor(kind)
        pd = smm.pin_operand(D)
        res = {"nnz_q": int(D.nnz) * int(E.nnz)}
        q = None
        if not explicit:
            q = smm.KroneckerOperand(pd, pe)
        elif res["nnz_q"] > 2 ** 31 - 2:
            res["cannot_be_built"] = f"nnz(Q) = {res['nnz_q']} > 2^31 - 2: more than an operand holds"
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q = smm.kronecker_product(pd, pe, pin=True)
            torch.cuda.synchronize()
            res["ms_build_q"] = round((time.perf_counter() - t0) * 1e3, 1)
            res["q_bytes"] = 12 * res["nnz_q"] + 4 * (H.shape[1] + 1)
        if q is not None:
            for k in tri:
                res[f"triple_{k}"] = measure(ctx, torch, names, lambda: smm.sparse_triple_product(ph, q, mask=pins[k]), reps)
            for k in aq:
                res[f"hq_{k}"] = measure(ctx, torch, names, lambda: smm.masked_matrix_multiply(ph, q, pins[k]), reps)
            if explicit:
                q.unpin()
        out[kind] = res
        pd.unpin()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit, library built: the baseline imports from it")
    ap.add_argument("--only", choices=["new", "baseline"])
    ap.add_argument("--root", default=os.path.dirname(HERE), help="tree the package is imported from (child processes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kinds", default="banded,dense")
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--timeout", type=int, default=900)
    args = ap.parse_args()
    kinds = args.kinds.split(",")
    if args.only:
        root = os.path.abspath(args.root)
        sys.path.insert(0, root)
        print(json.dumps(run(root, kinds, args.reps, args.exact, explicit=args.only == "baseline")))
        return
    if not args.parent:
        ap.error("--parent is required: the baseline must not be the tree under test")

    def child(role, root):
        assert os.path.exists(os.path.join(root, "scripts", "kron_bench.py")), f"{root} is not a checkout of this project"
        cmd = [sys.executable, os.path.abspath(__file__), "--only", role, "--root", root, "--reps", str(args.reps), "--kinds", args.kinds]
        p = subprocess.run(cmd + (["--exact"] if args.exact else []), capture_output=True, text=True, timeout=args.timeout)
        if p.returncode != 0:
            raise SystemExit(f"{role} failed ({p.returncode}):\n{p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])

    line = {"workload": f"H {N_OBS} x K (8 per row), Q = D (x) E of scripts/kron_bench.py; masks: identity, band 16, pattern of H, random 1e-5",
            "mode": "SMM_EXACT" if args.exact else "default", "reps": args.reps,
            "new": child("new", os.path.dirname(HERE)), "baseline_on_parent": child("baseline", os.path.abspath(args.parent))}
    verdict = {}
    for kind in kinds:
        base = line["baseline_on_parent"][kind]
        for key, new in line["new"][kind].items():
            if not isinstance(new, dict):
                continue
            if key in base:
                b, a = base[key]["ms_call"], new["ms_call"]
                verdict[f"{kind}_{key}"] = {"call_speedup_over_explicit_q": round(b["median"] / a["median"], 2),
                                            "faster_beyond_spread": a["spread"][1] < b["spread"][0],
                                            "slower_beyond_spread": a["spread"][0] > b["spread"][1]}
            else:
                verdict[f"{kind}_{key}"] = {"explicit_q": "cannot be built"}
    line["verdict"] = verdict
    out_dir = os.environ.get("OUT", "bench_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kron_masked_bench.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
