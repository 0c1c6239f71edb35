"""The empirical variogram on a taper's pattern (smm_variogram) against the two routes that exist without it.  One JSON line
per workload, appended to --out (default profiles/variogram_bench.jsonl).

    python scripts/variogram_bench.py [--steps N] [--warmup W] [--reps R] [--cases line,grid2d,grid3d] [--host-reps R]
                                      [--no-host] [--scale S]

The three workloads of taper_bench.py as cov_bench.py builds them (1e6 points, about 65 neighbours per row; --scale S divides
the point count), the pattern from localization_taper(coords on the device, cutoff, pin=True), values k = 1 and 16 columns of
standard normals in HBM, nb = 15 and 32 equal bins from 0 to the cutoff, each pair once (upper=True).  Run one case per
process, each under its own time limit.
Device: Context.variogram_device on the pinned pattern -- the HIP-event times of the two launches (ms_kernels, with the split)
and host wall time around the call, which includes the three small downloads (ms_call), median over R repetitions of N calls,
with the spread.  public_call: the same through empirical_variogram.
Baseline (a), `torch`: the same three arrays from torch operations on the device over the pattern's tensors -- gathers
coordinate by coordinate and column by column (see cov_bench.py on row gathers), bucketize, bincount with weights; rows by
repeat_interleave (timed with it and, rows_cached, without).  It uses nothing of smm_variogram.  The fused result is compared
with it at full size: counts must be equal, the largest relative difference of the sums is recorded.
Baseline (b), `host_route`: the pattern downloaded (PinnedOperand.to_scipy) and the same in numpy (searchsorted, bincount),
k = 1 and nb = 15 only -- each step timed, wall time, median over --host-reps runs with the spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cov_bench import timed, wall, workload  # noqa: E402
from sparse_matrix_mult_amd import empirical_variogram, localization_taper  # noqa: E402
from sparse_matrix_mult_amd.engine import default_context  # noqa: E402

KERNELS = ["smm_variogram_bins", "smm_variogram_finish"]


def torch_route(torch, pts, vals, rows, cols, edges):
    """(count, sum_h, sum_sq) over the entries with cols > rows, by torch alone."""
    nb = edges.numel() - 1
    h2 = None
    for t in range(pts.shape[1]):
        x = pts[:, t].contiguous()
        d = x[rows] - x[cols]
        h2 = d * d if h2 is None else h2 + d * d
    h = torch.sqrt(h2)
    s = torch.zeros_like(h)
    for c in range(vals.shape[1]):
        y = vals[:, c].contiguous()
        d = y[rows] - y[cols]
        s = s + d * d
    b = torch.bucketize(h, edges, right=True) - 1
    b = torch.where((cols > rows) & (b >= 0) & (b < nb), b, torch.full_like(b, nb))
    return (torch.bincount(b, minlength=nb + 1)[:nb], torch.bincount(b, weights=h, minlength=nb + 1)[:nb],
            torch.bincount(b, weights=s, minlength=nb + 1)[:nb])


def host_route(L, coords, vals, edges):
    """The parent's way to the same arrays from a pinned taper; returns the steps in seconds."""
    steps = {}
    t0 = time.perf_counter()
    S = L.to_scipy()
    steps["download_pattern_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    nb = edges.size - 1
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    cols = S.indices
    h2 = np.zeros(cols.size)
    for t in range(coords.shape[1]):
        x = np.ascontiguousarray(coords[:, t])
        d = x[rows] - x[cols]
        h2 += d * d
    h = np.sqrt(h2)
    s = np.zeros(cols.size)
    for c in range(vals.shape[1]):
        y = np.ascontiguousarray(vals[:, c])
        d = y[rows] - y[cols]
        s += d * d
    b = np.searchsorted(edges, h, side="right") - 1
    b = np.where((cols > rows) & (b >= 0) & (b < nb), b, nb)
    out = (np.bincount(b, minlength=nb + 1)[:nb], np.bincount(b, weights=h, minlength=nb + 1)[:nb], np.bincount(b, weights=s, minlength=nb + 1)[:nb])
    steps["numpy_s"] = time.perf_counter() - t0
    steps["total_s"] = sum(steps.values())
    return steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cases", default="line,grid2d,grid3d")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variogram_bench.jsonl"))
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
        values = np.random.default_rng(5).standard_normal((n, 16))
        t = torch.from_numpy(coords).to(dev)
        L = localization_taper(t, cutoff, pin=True)
        h, nnz = L._handle, L.nnz
        indptr, indices = h.pattern_torch()
        counts = (indptr[1:] - indptr[:-1]).to(torch.int64)
        cols = indices.to(torch.int64)
        ids = torch.arange(n, device=dev)
        rows_cached = torch.repeat_interleave(ids, counts)
        line = {"case": case, "points": n, "dim": dim, "cutoff": cutoff, "nnz": int(nnz), "neighbours_per_row": round(nnz / n, 2), "variants": []}
        line["repeat_interleave_ms"], _ = wall(lambda: torch.repeat_interleave(ids, counts), sync, args.reps)
        for k in (1, 16):
            v = torch.from_numpy(np.ascontiguousarray(values[:, :k])).to(dev)
            for nb in (15, 32):
                edges = np.linspace(0.0, cutoff, nb + 1)
                edges_t = torch.from_numpy(edges).to(dev)
                got = []

                def fused():
                    got[:] = ctx.variogram_device(h, t, dim, dim, v, k, k, edges, True)

                r = timed(ctx, fused, args.steps, args.warmup, args.reps, KERNELS)
                r.update({"k": k, "nb": nb, "pairs": int(got[0].sum())})

                def base(rows=None):
                    rr = torch.repeat_interleave(ids, counts) if rows is None else rows
                    return torch_route(torch, t, v, rr, cols, edges_t)

                ref = [x.cpu().numpy() for x in base()]
                r["counts_equal_torch"] = bool(np.array_equal(got[0], ref[0]))
                r["largest_relative_difference_from_torch"] = max(
                    float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))) for g, w in zip(got[1:], ref[1:]))
                r["ms_torch"], r["ms_torch_spread"] = wall(base, sync, args.reps)
                r["ms_torch_rows_cached"], r["ms_torch_rows_cached_spread"] = wall(lambda: base(rows_cached), sync, args.reps)
                r["torch_fastest_over_fused_call_slowest"] = round(r["ms_torch_rows_cached_spread"][0] / r["ms_call_spread"][1], 2)
                if k == 1 and nb == 15:
                    def public():
                        empirical_variogram(L, t, v, edges)

                    public()
                    r["public_call_ms"], r["public_call_ms_spread"] = wall(public, sync, args.reps)
                    if not args.no_host:
                        runs = [host_route(L, coords, values[:, :1], edges) for _ in range(args.host_reps)]
                        r["counts_equal_host"] = bool(np.array_equal(got[0], runs[0][1][0]))
                        totals = sorted(s["total_s"] for s, _ in runs)
                        med = [s for s, _ in runs if s["total_s"] == totals[len(totals) // 2]][0]
                        line["host_route"] = {key: round(val, 3) for key, val in med.items()}
                        line["host_route"]["total_s_spread"] = [round(totals[0], 3), round(totals[-1], 3)]
                        del runs
                line["variants"].append(r)
                print(json.dumps(r), flush=True)
            del v
        L.unpin()
        del t, indptr, indices, cols, counts, rows_cached
        torch.cuda.empty_cache()
        ctx.release_pool()
        print(json.dumps({key: val for key, val in line.items() if key != "variants"}), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
