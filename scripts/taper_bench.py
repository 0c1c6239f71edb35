"""The localisation taper built on the device (smm_taper_build) against the host route that exists without it.  One JSON
line per workload, appended to --out (default profiles/taper_bench.jsonl).

    python scripts/taper_bench.py [--steps N] [--warmup W] [--reps R] [--cases line,grid2d,grid3d] [--baseline-reps R]
                                  [--no-baseline] [--scale S]

Three workloads of about 65 neighbours per row and 6.5e7 entries (--scale S divides the point count: a quick look):
  line    1e6 points on a line, spacing 1, cutoff 32.5 (the pattern of triple_sparse_bench.py's Q)
  grid2d  1000 x 1000 grid, cutoff 4.6
  grid3d  100^3 grid, cutoff 2.5
Device: localization_taper(coords on the device, cutoff, pin=True) -- HIP-event sums of every launch of a call (ms_kernels,
with the per-kernel split) and host wall time around the call (ms_call), median over R repetitions of N calls, with the
spread.  Bytes the call must move: 12 per entry out plus the row pointer, and the column array once more through the
sort and the value pass (4 read + 4 written + 4 read), as a fraction of 8 TB/s at the measured kernel time.
Baseline, on the same coordinates: scipy.spatial.cKDTree.sparse_distance_matrix (COO output, the faster of its forms),
conversion to CSR, the Gaspari-Cohn weights in numpy and pin_operand (the upload), each step timed; wall time, median over
--baseline-reps runs with the spread.  The two patterns agree (the baseline's <= against the contract's < makes no
difference on these grids: no pair lies at exactly the cutoff); the script checks nnz."""
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
from sparse_matrix_mult_amd import localization_taper, pin_operand  # noqa: E402
from sparse_matrix_mult_amd.engine import default_context  # noqa: E402
from triple_sparse_bench import PEAK_BW, kernel_names  # noqa: E402


def workload(name, scale):
    if name == "line":
        return np.arange(1000000 // scale, dtype=np.float64).reshape(-1, 1), 32.5
    if name == "grid2d":
        side = int(round((1000000 / scale) ** 0.5))
        g = np.arange(side, dtype=np.float64)
        return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), 4.6
    if name == "grid3d":
        side = int(round((1000000 / scale) ** (1.0 / 3.0)))
        g = np.arange(side, dtype=np.float64)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3), 2.5
    raise KeyError(name)


def gaspari_cohn(d, cutoff):
    z = d / (0.5 * cutoff)
    with np.errstate(divide="ignore", invalid="ignore"):
        near = (((-0.25 * z + 0.5) * z + 0.625) * z - 5.0 / 3.0) * z * z + 1.0
        far = ((((1.0 / 12.0) * z - 0.5) * z + 0.625) * z + 5.0 / 3.0) * z
        far = (far - 5.0) * z + 4.0 - 2.0 / (3.0 * z)
    return np.maximum(np.where(z <= 1.0, near, far), 0.0)


def host_route(coords, cutoff):
    """The parent's way to an L in HBM; returns (steps in seconds, nnz)."""
    from scipy.spatial import cKDTree
    steps = {}
    t0 = time.perf_counter()
    tree = cKDTree(coords)
    D = tree.sparse_distance_matrix(tree, cutoff, output_type="coo_matrix")
    steps["kdtree_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    L = D.tocsr()
    L.sort_indices()
    steps["to_csr_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    L.data = gaspari_cohn(L.data, cutoff)
    L.indices = L.indices.astype(np.int32, copy=False)
    L.indptr = L.indptr.astype(np.int32, copy=False)
    steps["numpy_taper_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    P = pin_operand(L)
    default_context().synchronize()
    steps["pin_operand_s"] = time.perf_counter() - t0
    nnz = P.nnz
    P.unpin()
    steps["total_s"] = sum(steps.values())
    return steps, nnz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--cases", default="line,grid2d,grid3d")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taper_bench.jsonl"))
    args = ap.parse_args()
    import torch
    ctx = default_context()
    dev = torch.device("cuda", ctx.device)
    names = kernel_names()
    for case in args.cases.split(","):
        coords, cutoff = workload(case, args.scale)
        t = torch.from_numpy(coords).to(dev)
        held = []

        def build():
            held[:] = [localization_taper(t, cutoff, pin=True)]
            nnz = held[0].nnz
            held[0].unpin()
            return nnz

        nnz = build()
        r = timed(ctx, build, args.steps, args.warmup, args.reps, names)
        n = len(coords)
        out_bytes, col_bytes = 12 * nnz + 4 * (n + 1), 12 * nnz
        r.update({"bytes_out": out_bytes, "bytes_columns_through_sort_and_values": col_bytes,
                  "fraction_of_8TBps": round((out_bytes + col_bytes) / (r["ms_kernels"] * 1e-3) / PEAK_BW, 4)})
        line = {"case": case, "points": n, "dim": int(coords.shape[1]), "cutoff": cutoff, "nnz": int(nnz),
                "neighbours_per_row": round(nnz / n, 2), "device": r}
        print(json.dumps(line), flush=True)
        if not args.no_baseline:
            runs = []
            for i in range(args.baseline_reps):
                steps, host_nnz = host_route(coords, cutoff)
                assert host_nnz == nnz, f"{case}: the host route stores {host_nnz} entries, the device {nnz}"
                runs.append(steps)
                print(f"# {case}: host route run {i + 1}: {steps['total_s']:.2f} s", flush=True)
            totals = sorted(s["total_s"] for s in runs)
            med = runs[[s["total_s"] for s in runs].index(totals[len(totals) // 2])]
            line["host_route"] = {k: round(v, 3) for k, v in med.items()}
            line["host_route"]["total_s_spread"] = [round(totals[0], 3), round(totals[-1], 3)]
            line["speedup_call"] = round(med["total_s"] * 1e3 / r["ms_call"], 1)
            line["device_slowest_over_host_fastest"] = round(r["ms_call_spread"][1] / (totals[0] * 1e3), 5)
        del t
        torch.cuda.empty_cache()
        ctx.release_pool()
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
