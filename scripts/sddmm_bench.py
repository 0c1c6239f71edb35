"""The sampled dense product (smm_sddmm) against the routes that exist without it.  One JSON line per case, appended to
--out (default profiles/sddmm_bench.jsonl).

    python scripts/sddmm_bench.py [--steps N] [--warmup W] [--reps R] [--exact] [--cases band1m,c1] [--k 16,64,256]
                                  [--no-baseline] [--classes 0,1,2]

1. band1m: the scripts/triple_sparse_bench.py Q pattern -- K = 1 000 000 state variables, band half-width 32 (6.5e7
   entries) -- with an ensemble E (K x k) in HBM, Q = L o (E E^T), k in {16, 64, 256}.
2. c1: the BASELINE configs[1] shape, 50 000 rows, k = 64: the identity mask (diag(X Y^T)), a band of half-width 64 and a
   random mask of density 1e-4.
Baselines per case: masked_matrix_multiply's device call on csr(X), csr(Y^T) and the mask (the only route without this
kernel; the CSR copies of the dense operands are made on the device and are not timed, the first call -- which builds and
caches B^T -- is reported on its own, the steady state counts kernels only), and torch.sparse.sampled_addmm where it runs
(where it raises, the message is recorded instead).
Times: HIP-event sums of every launch of a call (ms_kernels) and host wall time around the call (ms_call), median over R
repetitions of N calls, with the spread.  Bytes per case: algorithmic (mask, X, Y and the output read or written once) and
gathered (one row segment of X and one of Y per entry), each as a fraction of 8 TB/s at the measured kernel time."""
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
from sparse_matrix_mult_amd.engine import default_context  # noqa: E402
from triple_sparse_bench import PEAK_BW, kernel_names  # noqa: E402


def band_pattern(n, w):
    """(indptr, indices) of the n x n band of half-width w, int32."""
    i = np.arange(n, dtype=np.int64)
    lo, hi = np.maximum(i - w, 0), np.minimum(i + w, n - 1)
    lens = hi - lo + 1
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.arange(int(indptr[-1]), dtype=np.int64) - np.repeat(indptr[:-1] - lo, lens)
    return indptr.astype(np.int32), indices.astype(np.int32)


def random_pattern(m, n, density, seed):
    rng = np.random.default_rng(seed)
    flat = np.unique(rng.integers(0, m * n, int(m * n * density)))
    rows, cols = flat // n, flat % n
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
    return indptr.astype(np.int32), cols.astype(np.int32)


def roofline(ms, nnz, m, n, k, same, scale):
    alg = 4 * (m + 1) + (12 if scale else 4) * nnz + 8 * (m if same else m + n) * k + 8 * nnz
    gat = 16 * nnz * k
    out = {"bytes_algorithmic": int(alg), "bytes_gathered": int(gat)}
    if ms:
        s = ms * 1e-3
        out["fraction_of_8TBps_algorithmic"] = round(alg / s / PEAK_BW, 4)
        out["fraction_of_8TBps_gathered"] = round(gat / s / PEAK_BW, 4)
    return out


def dense_as_csr(torch, ctx, T):
    """A dense rows x cols tensor as a CSR operand on the device (every element stored), borrowing T's values."""
    rows, cols = T.shape
    indptr = torch.arange(rows + 1, dtype=torch.int64, device=T.device).mul_(cols).to(torch.int32)
    indices = torch.arange(cols, dtype=torch.int32, device=T.device).repeat(rows)
    return ctx.csr_from_torch(rows, cols, indptr, indices, T.reshape(-1))


def run_case(torch, ctx, args, names, label, m, n, pattern, k, same, out):
    dev = torch.device("cuda", ctx.device)
    S, W, R = args.steps, args.warmup, args.reps
    indptr, indices = pattern
    nnz = int(indptr[-1])
    gen = torch.Generator(device=dev).manual_seed(7)
    X = torch.rand((m, k), dtype=torch.float64, device=dev, generator=gen) * 2 - 1
    Y = X if same else torch.rand((n, k), dtype=torch.float64, device=dev, generator=gen) * 2 - 1
    t_ptr, t_idx = torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev)
    t_w = torch.rand(nnz, dtype=torch.float64, device=dev, generator=gen)
    mask = ctx.csr_from_torch(m, n, t_ptr, t_idx, t_w)
    C = torch.empty(nnz, dtype=torch.float64, device=dev)
    line = {"case": label, "m": m, "n": n, "k": k, "nnz_mask": nnz, "y_is_x": same, "mode": "SMM_EXACT" if args.exact else "default",
            "scale_by_mask": True}
    for cls in args.classes:
        ctx.tune_sddmm(cls)
        r = timed(ctx, lambda: ctx.sddmm_into(mask, X, k, Y, k, k, C, scale=True, exact=args.exact), S, W, R, names)
        r.update(roofline(r["ms_kernels"], nnz, m, n, k, same, True))
        line[f"sddmm_class{cls}"] = r
    ctx.tune_sddmm(0)
    if not args.no_baseline:
        try:
            a = dense_as_csr(torch, ctx, X)
            Yt = Y.t().contiguous()
            b = dense_as_csr(torch, ctx, Yt)
            ctx.timing(True); ctx.timing_reset()
            t0 = time.perf_counter()
            ctx.spgemm_masked_into(a, b, mask, C.data_ptr(), exact=args.exact)
            ctx.synchronize()
            split = {nm: round(ctx.kernel_time(nm)[0], 3) for nm in names if ctx.kernel_time(nm)[1]}
            ctx.timing(False)
            line["masked_spgemm_first_call_with_bt_build"] = {"ms_call": round((time.perf_counter() - t0) * 1e3, 3), "split": split}
            line["masked_spgemm"] = timed(ctx, lambda: ctx.spgemm_masked_into(a, b, mask, C.data_ptr(), exact=args.exact), S, W, R, names)
            line["masked_spgemm"]["operand_bytes_csr_x_and_yt"] = int(12 * (m + n) * k)
            a.close(); b.close()
            del Yt
        except Exception as e:                      # (recorded, not hidden)
            line["masked_spgemm"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
        try:
            Mt = torch.sparse_csr_tensor(t_ptr.to(torch.int64), t_idx.to(torch.int64), torch.zeros(nnz, dtype=torch.float64, device=dev),
                                         size=(m, n))
            Ytt = Y.t()
            fn = lambda: torch.sparse.sampled_addmm(Mt, X, Ytt, beta=0.0)  # noqa: E731
            fn(); torch.cuda.synchronize()
            ts = []
            for _ in range(R):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(S):
                    fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / S)
            line["torch_sampled_addmm"] = {"ms_call": round(float(np.median(ts)), 3), "spread": [round(min(ts), 3), round(max(ts), 3)]}
            del Mt
        except Exception as e:
            line["torch_sampled_addmm"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
    mask.close()
    del X, Y, C, t_ptr, t_idx, t_w
    torch.cuda.empty_cache()
    ctx.release_pool()
    print(json.dumps(line), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--cases", default="band1m,c1")
    ap.add_argument("--k", default="16,64,256")
    ap.add_argument("--classes", default="0")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm_bench.jsonl"))
    args = ap.parse_args()
    args.classes = [int(c) for c in args.classes.split(",")]
    import torch
    ctx = default_context()
    names = kernel_names()
    cases = args.cases.split(",")
    if "band1m" in cases:
        K = 1000000
        pat = band_pattern(K, 32)
        for k in (int(v) for v in args.k.split(",")):
            run_case(torch, ctx, args, names, "band1m: K 1e6, half-width 32, Q = L o (E E^T)", K, K, pat, k, True, args.out)
    if "c1" in cases:
        n, k = 50000, 64
        i32 = np.arange(n + 1, dtype=np.int32)
        run_case(torch, ctx, args, names, "c1: identity mask, diag(X Y^T)", n, n, (i32, i32[:-1].copy()), k, False, args.out)
        run_case(torch, ctx, args, names, "c1: band half-width 64", n, n, band_pattern(n, 64), k, False, args.out)
        run_case(torch, ctx, args, names, "c1: random mask d=1e-4", n, n, random_pattern(n, n, 1e-4, 3), k, False, args.out)


if __name__ == "__main__":
    main()
