"""The observation operator built on the device (smm_interp_build) against the host route that exists without it.  One
JSON line per workload, appended to --out (default profiles/interp_bench.jsonl).

    python scripts/interp_bench.py [--steps N] [--warmup W] [--reps R] [--cases grid2d,grid3d,spacetime] [--baseline-reps R]
                                   [--no-baseline] [--scale S] [--ab-stage]

Three workloads, multilinear weights, points uniform inside the grid (--scale S divides the point count: a quick look):
  grid2d     1e6 points on a 1000 x 1000 grid (4 entries per row)
  grid3d     2e5 points on 100^3 (8 per row)
  spacetime  2e5 points on 40 x 158 x 158, time slowest: the columns of kron_bench.py's Q = D (x) E (8 per row)
and, only when named in --cases, grid2d_x10: 1e7 points on the 1000 x 1000 grid -- 520 MB written, where the fill's fixed
costs no longer show.
Device: interpolation_operator(points on the device, axes, pin=True) -- HIP-event sums of every launch of a call
(ms_kernels, with the per-kernel split) and host wall time around the call (ms_call), median over R repetitions of N calls,
with the spread.  Bytes the fill must write: 12 per entry plus the row pointer, as a fraction of 8 TB/s at the fill
kernel's own time (the points it reads, 8 dim bytes per row, are counted separately).
--ab-stage: the fill with the axes searched in LDS against the axes read where they are (SMM_INTERP_STAGE=0), on two
contexts, alternating, through Context.interp_into.
Baseline, on the same points: cell and fraction by np.searchsorted, the 2^dim weights and columns in numpy,
scipy.sparse.csr_matrix and pin_operand (the upload), each step timed; wall time, median over --baseline-reps runs with
the spread.  The script checks that both routes give the same columns and values."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from masked_bench import timed  # noqa: E402
from scipy.sparse import csr_matrix  # noqa: E402
from sparse_matrix_mult_amd import interpolation_operator, pin_operand  # noqa: E402
from sparse_matrix_mult_amd.engine import Context, default_context  # noqa: E402
from triple_sparse_bench import PEAK_BW, kernel_names  # noqa: E402

GRIDS = {"grid2d": ((1000, 1000), 1000000), "grid3d": ((100, 100, 100), 200000), "spacetime": ((40, 158, 158), 200000),
         "grid2d_x10": ((1000, 1000), 10000000)}


def workload(name, scale):
    shape, n = GRIDS[name]
    axes = [np.arange(m, dtype=np.float64) for m in shape]
    rng = np.random.default_rng(sorted(GRIDS).index(name))
    pts = np.stack([rng.random(n // scale) * (m - 1) for m in shape], axis=1)
    return axes, pts


def host_weights(pts, axes):
    """(indptr, indices, data) in the contract's order (include/smm_hip.h), vectorised over the points."""
    n, dim = pts.shape
    stride = [int(np.prod([a.size for a in axes[t + 1:]], dtype=np.int64)) for t in range(dim)]
    c, f = [], []
    for t, a in enumerate(axes):
        ct = np.clip(np.searchsorted(a, pts[:, t], side="right") - 1, 0, a.size - 2)
        c.append(ct)
        f.append((pts[:, t] - a[ct]) / (a[ct + 1] - a[ct]))
    cols = np.empty((n, 1 << dim), dtype=np.int32)
    vals = np.empty((n, 1 << dim))
    for e in range(1 << dim):
        col, w = 0, None
        for t in range(dim):
            up = (e >> (dim - 1 - t)) & 1
            col = col + (c[t] + up) * stride[t]
            wt = f[t] if up else 1.0 - f[t]
            w = wt if w is None else w * wt
        cols[:, e], vals[:, e] = col, w
    return np.arange(n + 1, dtype=np.int32) * (1 << dim), cols.ravel(), vals.ravel()


def host_route(pts, axes, K):
    """The parent's way to an H in HBM; returns (steps in seconds, the scipy matrix)."""
    steps = {}
    t0 = time.perf_counter()
    ptr, idx, val = host_weights(pts, axes)
    steps["numpy_weights_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    H = csr_matrix((val, idx, ptr), shape=(pts.shape[0], K))
    steps["csr_matrix_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    P = pin_operand(H)
    default_context().synchronize()
    steps["pin_operand_s"] = time.perf_counter() - t0
    P.unpin()
    steps["total_s"] = sum(steps.values())
    return steps, H


def ab_stage(t, axes, steps, reps):
    """Median fill kernel ms per call, axes in LDS against axes through L2, alternating."""
    ms = {"lds": [], "l2": []}
    ctxs = {"lds": default_context()}
    os.environ["SMM_INTERP_STAGE"] = "0"
    ctxs["l2"] = Context(default_context().device)
    del os.environ["SMM_INTERP_STAGE"]
    n, dim = t.shape
    try:
        for rep in range(reps + 1):
            for name, c in ctxs.items():
                c.timing(True); c.timing_reset()
                for _ in range(steps):
                    c.interp_into(t, dim, n, dim, axes).close()
                c.synchronize()
                if rep:                                              # (the first round warms up)
                    ms[name].append(c.kernel_time("smm_interp_fill")[0] / steps)
                c.timing(False)
    finally:
        ctxs["l2"].close()
    return {k: {"ms_fill": round(float(np.median(v)), 4), "spread": [round(min(v), 4), round(max(v), 4)]} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--cases", default="grid2d,grid3d,spacetime")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--ab-stage", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_bench.jsonl"))
    args = ap.parse_args()
    import torch
    ctx = default_context()
    dev = torch.device("cuda", ctx.device)
    names = kernel_names()
    for case in args.cases.split(","):
        axes, pts = workload(case, args.scale)
        n, dim = pts.shape
        K = int(np.prod([a.size for a in axes]))
        t = torch.from_numpy(pts).to(dev)

        def build():
            P = interpolation_operator(t, axes, pin=True)
            nnz = P.nnz
            P.unpin()
            return nnz

        nnz = build()
        r = timed(ctx, build, args.steps, args.warmup, args.reps, names)
        out_bytes = 12 * nnz + 4 * (n + 1)
        fill_ms = r["split"].get("smm_interp_fill", float("nan"))
        r.update({"bytes_written": out_bytes, "bytes_points_read": 8 * dim * n,
                  "written_fraction_of_8TBps": round(out_bytes / (fill_ms * 1e-3) / PEAK_BW, 4)})
        line = {"case": case, "points": n, "grid": [a.size for a in axes], "nnz": int(nnz), "device": r}
        if args.ab_stage:
            line["axes_lds_vs_l2"] = ab_stage(t, axes, args.steps, args.reps)
        print(json.dumps(line), flush=True)
        if not args.no_baseline:
            runs = []
            for i in range(args.baseline_reps):
                steps, H = host_route(pts, axes, K)
                runs.append(steps)
                print(f"# {case}: host route run {i + 1}: {steps['total_s']:.3f} s", flush=True)
            got = interpolation_operator(t, axes)
            assert np.array_equal(got.indptr, H.indptr) and np.array_equal(got.indices, H.indices), f"{case}: patterns differ"
            assert np.array_equal(got.data.view(np.int64), H.data.view(np.int64)), f"{case}: values differ"
            totals = sorted(s["total_s"] for s in runs)
            med = runs[[s["total_s"] for s in runs].index(totals[len(totals) // 2])]
            line["host_route"] = {k: round(v, 4) for k, v in med.items()}
            line["host_route"]["total_s_spread"] = [round(totals[0], 4), round(totals[-1], 4)]
            line["speedup_call"] = round(med["total_s"] * 1e3 / r["ms_call"], 1)
        del t
        torch.cuda.empty_cache()
        ctx.release_pool()
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
