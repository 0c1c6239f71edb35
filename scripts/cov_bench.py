"""Parametric covariances on a taper's pattern (smm_cov_eval) against the two routes that exist without it.  One JSON line
per workload, appended to --out (default profiles/cov_bench.jsonl).

    python scripts/cov_bench.py [--steps N] [--warmup W] [--reps R] [--cases line,grid2d,grid3d] [--host-reps R]
                                [--no-host] [--scale S]

The three workloads of taper_bench.py (1e6 points, about 65 neighbours per row; --scale S divides the point count), the
pattern from localization_taper(coords on the device, cutoff, pin=True), correlation length = cutoff / 3, variance 2.5.
Variants: each of the five models, value only and value plus d/dlength, with and without scaling by the pattern.
Device: Context.cov_into on the pinned pattern into preallocated tensors -- the HIP-event time of the launch (ms_kernels) and
host wall time around the call (ms_call), median over R repetitions of N calls, with the spread.  Bytes the call must
move: 4 per entry for the column, 8 per output written and 8 more when scaled, as a fraction of 8 TB/s at the measured
kernel time (the coordinates, 8 dim per point, are read once from HBM and are not counted).  public_call: the same through
covariance_on_pattern(..., pin=True), which also copies the pattern for each result and pins them.
Baseline (a), `torch`: the same arrays from torch element-wise operations on the device over the pattern's tensors, rows
by repeat_interleave (timed with it and, rows_cached, without); it uses nothing of smm_cov_eval.  The fused result is
compared with it at full size (largest relative difference, recorded).
Baseline (b), `host_route`: the pattern downloaded (PinnedOperand.to_scipy), the exponential model's value and derivative in
numpy, scaled, and pin_operand of both -- each step timed, wall time, median over --host-reps runs with the spread."""
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
from sparse_matrix_mult_amd import covariance_on_pattern, localization_taper, pin_operand  # noqa: E402
from sparse_matrix_mult_amd.engine import COV_MODELS, default_context  # noqa: E402
from taper_bench import workload  # noqa: E402
from triple_sparse_bench import PEAK_BW  # noqa: E402

SQRT3, SQRT5 = 1.7320508075688772, 2.23606797749979
VARIANCE = 2.5


def correlation(xp, model, h2, h):
    """(c, g) of include/smm_hip.h with the array module xp (torch or numpy)."""
    if model == "spherical":
        inside = h < 1.0
        zero = xp.zeros_like(h)
        return xp.where(inside, ((0.5 * h) * h - 1.5) * h + 1.0, zero), xp.where(inside, 1.5 - 1.5 * (h * h), zero)
    if model == "exponential":
        e = xp.exp(-h)
        return e, e
    if model == "gaussian":
        e = xp.exp(-h2)
        return e, (2.0 * h) * e
    if model == "matern32":
        s = SQRT3 * h
        e = xp.exp(-s)
        return (1.0 + s) * e, (3.0 * h) * e
    s = SQRT5 * h
    e = xp.exp(-s)
    return ((1.0 + s) + (5.0 / 3.0) * h2) * e, (((5.0 / 3.0) * h) * (1.0 + s)) * e


def elementwise(xp, pts, rows, cols, w, model, length, deriv, scale):
    """(val, dval) from element-wise array operations over the entries (rows, cols): the baseline, in torch or numpy.
    Coordinate by coordinate, from contiguous columns: gathers of 8-byte elements.  (The row gather pts[rows] of a
    two-column tensor with 6.9e7 indices came back with wrong rows from torch on the MI355X: this script's check against
    the fused result showed it, and the fused result equalled the restatement.)"""
    h2 = None
    for t in range(pts.shape[1]):
        x = pts[:, t].contiguous() if xp is not np else np.ascontiguousarray(pts[:, t])
        u = (x[rows] - x[cols]) / length
        h2 = u * u if h2 is None else h2 + u * u
    h = xp.sqrt(h2)
    c, g = correlation(xp, model, h2, h)
    val = VARIANCE * c
    dval = None
    if deriv:
        dval = xp.where(h == 0.0, xp.zeros_like(h), ((VARIANCE * g) * h) / length)
    if scale:
        val = val * w
        dval = dval * w if deriv else None
    return val, dval


def wall(fn, sync, reps):
    """(median ms, [min, max]) of fn() followed by sync()."""
    ms = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]


def host_route(L, coords, length):
    """The parent's way to (Q, dQ) in HBM from a pinned taper; returns the steps in seconds."""
    steps = {}
    t0 = time.perf_counter()
    S = L.to_scipy()
    steps["download_pattern_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    val, dval = elementwise(np, coords, rows, S.indices, S.data, "exponential", length, True, True)
    Q, dQ = S.copy(), S.copy()
    Q.data, dQ.data = val, dval
    steps["numpy_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    P = [pin_operand(Q), pin_operand(dQ)]
    default_context().synchronize()
    steps["pin_operand_s"] = time.perf_counter() - t0
    for p in P:
        p.unpin()
    steps["total_s"] = sum(steps.values())
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cases", default="line,grid2d,grid3d")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_bench.jsonl"))
    args = ap.parse_args()
    import torch
    ctx = default_context()
    dev = torch.device("cuda", ctx.device)

    def sync():
        torch.cuda.synchronize()
        ctx.synchronize()

    for case in args.cases.split(","):
        coords, cutoff = workload(case, args.scale)
        n, dim = coords.shape
        length = cutoff / 3.0
        t = torch.from_numpy(coords).to(dev)
        L = localization_taper(t, cutoff, pin=True)
        h, nnz = L._handle, L.nnz
        out = [torch.empty(nnz, dtype=torch.float64, device=dev) for _ in range(2)]
        indptr, indices = h.pattern_torch()
        w = torch.empty(nnz, dtype=torch.float64, device=dev)
        h.values_into(w)
        counts = (indptr[1:] - indptr[:-1]).to(torch.int64)
        cols = indices.to(torch.int64)
        ids = torch.arange(n, device=dev)
        rows_cached = torch.repeat_interleave(ids, counts)
        line = {"case": case, "points": n, "dim": dim, "cutoff": cutoff, "length": length, "nnz": int(nnz),
                "neighbours_per_row": round(nnz / n, 2), "variants": []}
        line["repeat_interleave_ms"], _ = wall(lambda: torch.repeat_interleave(ids, counts), sync, args.reps)
        for model in COV_MODELS:
            for deriv in (False, True):
                for scale in (False, True):
                    wrt = "length" if deriv else None

                    def fused():
                        ctx.cov_into(h, t, dim, t, dim, dim, model, length, VARIANCE, out[0], out[1] if deriv else None, wrt=wrt, scale=scale)

                    r = timed(ctx, fused, args.steps, args.warmup, args.reps, ["smm_cov_eval"])
                    nbytes = nnz * (4 + 8 * (1 + deriv) + 8 * scale)
                    r.pop("split")
                    r.update({"model": model, "derivative": deriv, "scaled": scale, "bytes": nbytes,
                              "fraction_of_8TBps": round(nbytes / (r["ms_kernels"] * 1e-3) / PEAK_BW, 4)})

                    def base(rows=None):
                        rr = torch.repeat_interleave(ids, counts) if rows is None else rows
                        return elementwise(torch, t, rr, cols, w, model, length, deriv, scale)

                    ref = base()
                    diff = 0.0
                    for got, want in zip(out, ref):
                        if want is not None:
                            scale_ = torch.clamp(want.abs(), min=1e-300)
                            diff = max(diff, float(((got - want).abs() / scale_).max().item()))
                    del ref
                    r["largest_relative_difference_from_torch"] = diff
                    r["ms_torch"], r["ms_torch_spread"] = wall(base, sync, args.reps)
                    r["ms_torch_rows_cached"], r["ms_torch_rows_cached_spread"] = wall(lambda: base(rows_cached), sync, args.reps)
                    r["torch_fastest_over_fused_call_slowest"] = round(r["ms_torch_rows_cached_spread"][0] / r["ms_call_spread"][1], 2)
                    line["variants"].append(r)
                    print(json.dumps(r), flush=True)

        def public():
            Q, dQ = covariance_on_pattern(L, t, "exponential", length, VARIANCE, scale_by_pattern=True, derivative="length", pin=True)
            Q.unpin(); dQ.unpin()

        public()
        line["public_call_ms"], line["public_call_ms_spread"] = wall(public, sync, args.reps)
        if not args.no_host:
            runs = [host_route(L, coords, length) for _ in range(args.host_reps)]
            totals = sorted(s["total_s"] for s in runs)
            med = runs[[s["total_s"] for s in runs].index(totals[len(totals) // 2])]
            line["host_route"] = {k: round(v, 3) for k, v in med.items()}
            line["host_route"]["total_s_spread"] = [round(totals[0], 3), round(totals[-1], 3)]
        L.unpin()
        del t, out, w, indptr, indices, cols, counts, rows_cached
        torch.cuda.empty_cache()
        ctx.release_pool()
        print(json.dumps({k: v for k, v in line.items() if k != "variants"}), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
