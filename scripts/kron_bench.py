"""The Kronecker operand Q = D (x) E -- device build, matrix-free apply, triple apply and CG solve -- against what a user
has without it.  One JSON line, appended to $OUT/kron_bench.jsonl (default bench_out/).

    python scripts/kron_bench.py --parent DIR [--reps R] [--widths 1,16,64] [--kinds banded,dense] [--exact]
    python scripts/kron_bench.py --only new --kinds dense --widths 16 --reps 1          (what a profiler wraps)

Workload (one MI355X): E is a 158 x 158-point grid tapered by localization_taper to 69 entries per interior row (cutoff
4.5 grid steps, Gaspari-Cohn), r = 24 964; p = 40 periods, so K = p r = 998 560 states -- the K = 1 000 000 case of
scripts/triple_sparse_bench.py, whose H (200 000 x K, 8 per row) is used.  D is banded with half-width 2 or dense
(exp(-|t - t'| / 8)).  R is the diagonal that makes S + R strictly diagonally dominant.  Operands pinned, X and Y in HBM.
  new       the tree this script lives in: kronecker_product(pin=True) (banded D only; the refusal is recorded for the dense
            one), KroneckerOperand through sparse_dense_multiply, triple_product_apply and innovation_solve (8 iterations).
            Wall time per call, and the HIP-event sum of every launch of one more call of Context.kron_apply_into with its
            bytes against the floor nnz(E) 12 + 3 K k 8.
  baseline  a child process that imports the package from DIR -- a checkout of the parent commit with its own library -- so
            the code under test never times itself:
            (a) explicit Q from scipy.sparse.kron on the host, pinned (banded D only: the dense Q has 2.7e9 entries, more
                than an operand holds), through the same three calls;
            (b) the two-step recipe from public calls: p calls of sparse_dense_multiply(E, .) and one
                sparse_dense_multiply(D, U.reshape(p, r k)).
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
PEAK_BW = 8e12
GRID, P, N_OBS, CUTOFF, CG_ITERS = 158, 40, 200000, 4.5, 8


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "spread": [round(float(min(ms)), 3), round(float(max(ms)), 3)]}


def d_factor(kind):
    t = np.arange(P)
    dense = np.exp(-np.abs(t[:, None] - t[None, :]) / 8.0)
    if kind == "banded":
        dense = np.where(np.abs(t[:, None] - t[None, :]) <= 2, dense, 0.0)
    return sp.csr_matrix(dense)


def workload(root):
    """(H, E, coords): E comes from `root`'s own localization_taper."""
    sys.path.insert(0, os.path.join(root, "scripts"))
    from triple_sparse_bench import local_h
    import sparse_matrix_mult_amd
    assert os.path.abspath(sparse_matrix_mult_amd.__file__).startswith(os.path.abspath(root) + os.sep), sparse_matrix_mult_amd.__file__
    g = np.arange(GRID, dtype=np.float64)
    coords = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    E = sparse_matrix_mult_amd.localization_taper(coords, CUTOFF)
    return local_h(N_OBS, P * GRID * GRID, 1), E


def dominant_r(H, D, E):
    """|H| (|D| (x) |E|) |H|^T 1 + U(0.5, 1.5), the Kronecker factor applied through its factors."""
    v = np.asarray(abs(H).T @ np.ones(H.shape[0])).reshape(P, -1)
    w = np.asarray(abs(D) @ np.asarray(abs(E) @ v.T).T).ravel()
    return np.asarray(abs(H) @ w).ravel() + np.random.default_rng(3).uniform(0.5, 1.5, H.shape[0])


def wall(fn, reps, sync):
    fn(); sync()                                     # warm-up (and H^T, built on first use)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def three_calls(smm, torch, dev, ph, q, pr, K, widths, reps):
    """sparse_dense_multiply, triple_product_apply and CG_ITERS iterations of innovation_solve with q as Q."""
    out = {}
    for k in widths:
        rng = np.random.default_rng(4)
        X = torch.from_numpy(rng.standard_normal((K, k))).to(dev)
        W = torch.from_numpy(rng.standard_normal((N_OBS, k))).to(dev)
        out[f"k{k}"] = {
            "ms_apply": wall(lambda: smm.sparse_dense_multiply(q, X), reps, torch.cuda.synchronize),
            "ms_triple_apply": wall(lambda: smm.triple_product_apply(ph, q, W), reps, torch.cuda.synchronize),
            f"ms_solve_{CG_ITERS}_iterations": wall(lambda: smm.innovation_solve(ph, q, pr, W, tol=1e-30, maxiter=CG_ITERS), reps,
                                                    torch.cuda.synchronize)}
        del X, W
    return out


def run_new(root, kinds, widths, reps, exact):
    import torch
    H, E = workload(root)
    import sparse_matrix_mult_amd as smm
    from sparse_matrix_mult_amd.engine import default_context
    from triple_sparse_bench import kernel_names
    ctx = default_context()
    dev = torch.device("cuda", ctx.device)
    smm.set_exact(exact)
    names = kernel_names()
    K = H.shape[1]
    ph, pe = smm.pin_operand(H), smm.pin_operand(E)
    out = {"nnz_e": int(E.nnz), "r": int(E.shape[0]), "K": int(K)}
    for kind in kinds:
        D = d_factor(kind)
        pd, pr = smm.pin_operand(D), smm.pin_operand(sp.diags(dominant_r(H, D, E)).tocsr())
        res = {"nnz_d": int(D.nnz), "nnz_q": int(D.nnz) * int(E.nnz)}
        try:                                         # the explicit operand, built where it is used
            ms_call, ms_fill = [], []
            for rep in range(reps + 1):              # (the first one is the warm-up)
                ctx.timing(True); ctx.timing_reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                built = smm.kronecker_product(pd, pe, pin=True)
                ctx.synchronize()
                if rep:
                    ms_call.append((time.perf_counter() - t0) * 1e3)
                    ms_fill.append(ctx.kernel_time("smm_kron_fill")[0])
                ctx.timing(False)
                built.unpin()
            nbytes = 12 * res["nnz_q"] + 4 * (K + 1)
            res["build"] = {"ms_call": stats(ms_call), "ms_fill_kernel": stats(ms_fill), "bytes": nbytes,
                            "fraction_of_8TBps": round(nbytes / (float(np.median(ms_fill)) * 1e-3) / PEAK_BW, 4)}
        except ValueError as e:
            res["build"] = {"refused": str(e)[:160]}
        q = smm.KroneckerOperand(pd, pe)
        res.update(three_calls(smm, torch, dev, ph, q, pr, K, widths, reps))
        for k in widths:                             # the launches of one apply, and their bytes against the floor
            X = torch.from_numpy(np.random.default_rng(4).standard_normal((K, k))).to(dev)
            Y = torch.empty((K, k), dtype=torch.float64, device=dev)
            call = lambda: ctx.kron_apply_into(pd._handle, pe._handle, X, k, k, Y, k, exact=exact)  # noqa: E731
            call()
            ctx.timing(True); ctx.timing_reset()
            call()
            split = {nm: round(ctx.kernel_time(nm)[0], 3) for nm in names if ctx.kernel_time(nm)[1]}
            ctx.timing(False)
            kern, floor = sum(split.values()), 12 * int(E.nnz) + 3 * K * k * 8
            moved = 12 * int(E.nnz) + 8 * K * k * (2 + 1 + int(D.nnz) / P)          # X in, U out, U in nnz(D)/p times, Y out
            res[f"k{k}"].update({"ms_apply_kernels": round(kern, 3), "split": split, "bytes_floor": floor, "bytes_moved": int(moved),
                                 "floor_fraction_of_8TBps": round(floor / (kern * 1e-3) / PEAK_BW, 4),
                                 "moved_fraction_of_8TBps": round(moved / (kern * 1e-3) / PEAK_BW, 4)})
            del X, Y
        out[kind] = res
        pd.unpin(); pr.unpin()
    return out


def run_baseline(root, kinds, widths, reps, exact):
    import torch
    H, E = workload(root)
    import sparse_matrix_mult_amd as smm
    from sparse_matrix_mult_amd.engine import default_context
    dev = torch.device("cuda", default_context().device)
    smm.set_exact(exact)
    K, r = H.shape[1], E.shape[0]
    ph, pe = smm.pin_operand(H), smm.pin_operand(E)
    out = {}
    for kind in kinds:
        D = d_factor(kind)
        pd, pr = smm.pin_operand(D), smm.pin_operand(sp.diags(dominant_r(H, D, E)).tocsr())
        res = {}
        # (b) the two-step recipe from public calls
        two = {}
        for k in widths:
            X = torch.from_numpy(np.random.default_rng(4).standard_normal((K, k))).to(dev)

            def recipe():
                U = torch.empty((P, r, k), dtype=torch.float64, device=dev)
                for t in range(P):
                    U[t] = smm.sparse_dense_multiply(pe, X[t * r:(t + 1) * r])
                return smm.sparse_dense_multiply(pd, U.reshape(P, r * k)).reshape(K, k)
            two[f"k{k}"] = {"ms_apply": wall(recipe, reps, torch.cuda.synchronize)}
            del X
        res["b_two_step_recipe"] = two
        # (a) the explicit Q, where an operand can hold it
        nnz_q = int(D.nnz) * int(E.nnz)
        if nnz_q > 2 ** 31 - 2:
            res["a_explicit_q"] = {"cannot_be_built": f"nnz(Q) = {nnz_q} > 2^31 - 2: more than an operand holds"}
        else:
            t0 = time.perf_counter()
            Q = sp.kron(D, E, format="csr")
            t1 = time.perf_counter()
            pq = smm.pin_operand(Q)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res["a_explicit_q"] = {"ms_host_kron": round((t1 - t0) * 1e3, 1), "ms_pin_upload": round((t2 - t1) * 1e3, 1), "nnz_q": int(Q.nnz)}
            del Q
            res["a_explicit_q"].update(three_calls(smm, torch, dev, ph, pq, pr, K, widths, reps))
            pq.unpin()
        out[kind] = res
        pd.unpin(); pr.unpin()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit, library built: the baselines import from it")
    ap.add_argument("--only", choices=["new", "baseline"])
    ap.add_argument("--root", default=os.path.dirname(HERE), help="tree the package is imported from (child processes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--widths", default="1,16,64")
    ap.add_argument("--kinds", default="banded,dense")
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--timeout", type=int, default=900)
    args = ap.parse_args()
    widths, kinds = [int(w) for w in args.widths.split(",")], args.kinds.split(",")
    if args.only:
        root = os.path.abspath(args.root)
        sys.path.insert(0, root)
        print(json.dumps((run_new if args.only == "new" else run_baseline)(root, kinds, widths, args.reps, args.exact)))
        return
    if not args.parent:
        ap.error("--parent is required: the baselines must not be the tree under test")

    def child(role, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", role, "--root", root, "--reps", str(args.reps), "--widths", args.widths,
               "--kinds", args.kinds]
        p = subprocess.run(cmd + (["--exact"] if args.exact else []), capture_output=True, text=True, timeout=args.timeout)
        if p.returncode != 0:
            raise SystemExit(f"{role} failed ({p.returncode}):\n{p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])

    line = {"workload": f"Q = D (x) E: E {GRID} x {GRID} grid tapered at {CUTOFF} steps, p = {P}, H {N_OBS} x K (8 per row)",
            "mode": "SMM_EXACT" if args.exact else "default", "reps": args.reps,
            "new": child("new", os.path.dirname(HERE)), "baseline_on_parent": child("baseline", os.path.abspath(args.parent))}
    verdict = {}
    for kind in kinds:
        for k in widths:
            a = line["new"][kind][f"k{k}"]["ms_apply"]
            b = line["baseline_on_parent"][kind]["b_two_step_recipe"][f"k{k}"]["ms_apply"]
            v = {"apply_speedup_over_b": round(b["median"] / a["median"], 2), "below_b_beyond_spread": a["spread"][1] < b["spread"][0]}
            ex = line["baseline_on_parent"][kind]["a_explicit_q"]
            if f"k{k}" in ex:
                for key in ("ms_apply", "ms_triple_apply", f"ms_solve_{CG_ITERS}_iterations"):
                    v[key.replace("ms_", "") + "_speedup_over_a"] = round(ex[f"k{k}"][key]["median"] / line["new"][kind][f"k{k}"][key]["median"], 2)
            verdict[f"{kind}_k{k}"] = v
    line["verdict"] = verdict
    out_dir = os.environ.get("OUT", "bench_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kron_bench.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
