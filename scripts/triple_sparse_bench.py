"""Sparse-output triple product S = H Q H^T (smm_triple_product_sparse) on the covariance workload of the issue that
added it, plus a reduced BASELINE configs[3]-like shape against the dense triple product.  One JSON line.

    python scripts/triple_sparse_bench.py [--steps N] [--warmup W] [--n 200000] [--K 1000000] [--band 32] [--no-scipy]

Workload: K states, Q symmetric banded with half-width `band`; H n x K, 8 nonzeros per row inside a 16-column window
around a random centre.  Reported: ms per product (kernels, summed HIP-event times of every launch of the call, and end
to end through sparse_triple_product with a scipy result), the per-kernel split, nnz(S), the algorithmic bytes of the
stage-2 numeric kernel and their fraction of 8 TB/s, scipy's triu(H @ Q @ H.T) on the same operands, and why the dense
triple product cannot run this size."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_matrix_mult_amd import set_exact, sparse_triple_product  # noqa: E402
from sparse_matrix_mult_amd.engine import default_context  # noqa: E402

HBM_BYTES = 288e9
PEAK_BW = 8e12


def kernel_names():
    names = set()
    for line in open(os.path.join(ROOT, "sparse_matrix_mult_amd", "csrc", "smm_api.hip")):
        if "LAUNCH" in line or "LaunchTimer" in line:
            names.update(re.findall(r'"(smm_\w+)"', line))
    return sorted(names)


def local_h(n, K, seed):
    rng = np.random.default_rng(seed)
    centre = rng.integers(8, K - 8, size=n)
    off = np.argsort(rng.random((n, 16)), axis=1)[:, :8]
    cols = np.sort(centre[:, None] - 8 + off, axis=1).astype(np.int32)
    return sp.csr_matrix((rng.uniform(-1, 1, 8 * n), cols.ravel(), np.arange(0, 8 * n + 1, 8, dtype=np.int32)), shape=(n, K))


def banded_q(K, w, seed):
    rng = np.random.default_rng(seed)
    B = sp.diags([rng.uniform(-1, 1, K - abs(d)) for d in range(-w, w + 1)], list(range(-w, w + 1)), shape=(K, K), format="csr")
    return ((B + B.T) * 0.5).tocsr()


def timed(ctx, fn, steps, warmup, names):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    ctx.timing(True); ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    split = {}
    for k in names:
        ms, calls = ctx.kernel_time(k)
        if calls:
            split[k] = round(ms / steps, 3)
    ctx.timing(False)
    return out, wall, split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--K", type=int, default=1000000)
    ap.add_argument("--band", type=int, default=32)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    ctx = default_context()
    names = kernel_names()
    set_exact(args.exact)
    n, K = args.n, args.K
    H, Q = local_h(n, K, 1), banded_q(K, args.band, 2)
    h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
    (ptr, idx, _), dev_ms, split = timed(ctx, lambda: ctx.triple_sparse_torch(h, q, exact=args.exact), args.steps, args.warmup, names)
    kernel_ms = round(sum(split.values()), 3)
    nnz_s = int(idx.numel())
    ptr, idx = ptr.cpu().numpy(), idx.cpu().numpy()
    # stage-2 numeric kernel, algorithmic bytes: T rows once (12 B per entry), S indices in and values out (12 B per entry),
    # per entry of S its row of H (row pointer 8 B + 12 B per entry)
    t0 = time.perf_counter()
    T = (H @ Q).tocsr()
    nnz_t = int(T.nnz)
    h_len = np.diff(H.indptr).astype(np.int64)
    s2_bytes = 12 * nnz_t + 12 * nnz_s + int(8 * nnz_s + 12 * h_len[idx].sum())
    s2_ms = split.get("smm_triple_sparse_s2", 0.0)
    e2e = []
    for _ in range(args.warmup + args.steps):
        t1 = time.perf_counter()
        sparse_triple_product(H, Q)
        e2e.append((time.perf_counter() - t1) * 1e3)
    line = {
        "workload": f"S = H Q H^T, H {n} x {K} (8 per row in a 16-column window), Q banded half-width {args.band}, "
                    f"{'SMM_EXACT' if args.exact else 'default'} mode",
        "ms_kernels": kernel_ms, "ms_device_call": round(dev_ms, 3),
        "ms_end_to_end_api": round(float(np.median(e2e[args.warmup:])), 3),
        "kernel_split_ms": split, "nnz_s": nnz_s, "nnz_t": nnz_t, "nnz_h": int(H.nnz), "nnz_q": int(Q.nnz),
        "stage2_numeric": {"ms": s2_ms, "bytes": s2_bytes,
                           "fraction_of_8TBps": round(s2_bytes / (s2_ms * 1e-3) / PEAK_BW, 4) if s2_ms else None},
        "dense_triple": {"bytes_needed": 8 * n * n, "hbm_bytes": HBM_BYTES, "fits": 8 * n * n < HBM_BYTES,
                         "note": "n x n float64 result alone (plus T, n x K, in stage 1); arithmetic, not attempted"},
    }
    h.close(); q.close()
    if not args.no_scipy:
        t1 = time.perf_counter()
        W = sp.triu((T @ H.T).tocsr())
        line["scipy_triu_ms"] = round((time.perf_counter() - t1 + (t1 - t0)) * 1e3, 1)
        line["scipy_nnz"] = int(W.nnz)
    # reduced configs[3]-like shape: where the dense triple product wins
    Hs = sp.random(5000, 20000, density=0.02, format="csr", random_state=np.random.default_rng(3))
    S = sp.random(20000, 20000, density=0.01, format="csr", random_state=np.random.default_rng(4))
    Qs = (S + S.T).tocsr()
    hs, qs = ctx.csr_from_scipy(Hs), ctx.csr_from_scipy(Qs)
    (_, ci, _), sm, _ = timed(ctx, lambda: ctx.triple_sparse_torch(hs, qs, exact=args.exact), 3, 1, names)
    import torch
    out = torch.empty((5000, 5000), dtype=torch.float64, device=torch.device("cuda", ctx.device))
    _, dm, _ = timed(ctx, lambda: ctx.triple_into(hs, qs, out.data_ptr(), exact=args.exact), 3, 1, names)
    line["c3_reduced"] = {"shape": "H 5000 x 20000 d=0.02, Q 20000 x 20000 symmetric d=0.02", "nnz_s": int(ci.numel()),
                          "fill_of_upper": round(int(ci.numel()) / (5000 * 5001 / 2), 4),
                          "ms_sparse": round(sm, 3), "ms_dense": round(dm, 3)}
    hs.close(); qs.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
