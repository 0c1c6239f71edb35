"""Sparse x dense products (smm_spmm, smm_triple_apply) against what users have today.  One JSON line.

    python scripts/spmm_bench.py [--steps N] [--warmup W] [--reps R] [--exact] [--no-scipy] [--no-triple]

1. BASELINE configs[1] A (50 000 x 50 000, d = 0.01, generated on the device), Y = A X and Y = A^T X for k in
   {1, 8, 64, 256}; X and Y in HBM.  The first transposed call on a fresh handle builds A^T (reported on its own); every
   later call finds it cached.  Baselines: the device SpGEMM with a dense result on X as a CSR
   (sparse_matrix_multiply(A, csr_matrix(X), output_format='dense'), timed as its device call with X already
   uploaded), torch.sparse_csr_tensor(...) @ X on the same device (or why it did not run), and scipy on the host.
2. The scripts/triple_sparse_bench.py workload (H 200 000 x 1 000 000, Q banded half-width 32): S X = H (Q (H^T X))
   for k in {1, 16, 64}, against scipy's H @ (Q @ (H.T @ X)).
Times: HIP-event sums of every launch of a call (ms_kernels) and host wall time around the call (ms_call), median over
R repetitions of N calls, with the spread.  Bytes per case: algorithmic (A, X and Y read or written once) and gathered
(nnz(A) * k * 8, one row segment of X per nonzero), each as a fraction of 8 TB/s at the measured kernel time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from masked_bench import timed  # noqa: E402
from sparse_matrix_mult_amd.engine import default_context  # noqa: E402
from triple_sparse_bench import PEAK_BW, banded_q, kernel_names, local_h  # noqa: E402


def roofline(ms, nnz, rows, cols_x, k):
    """Bytes of Y = op(A) X (op(A): rows x cols_x with nnz entries) and their fractions of 8 TB/s at `ms`."""
    alg = 12 * nnz + 4 * (rows + 1) + 8 * cols_x * k + 8 * rows * k
    gat = 8 * nnz * k
    s = ms * 1e-3
    out = {"bytes_algorithmic": int(alg), "bytes_gathered": int(gat)}
    if ms:
        out["fraction_of_8TBps_algorithmic"] = round(alg / s / PEAK_BW, 4)
        out["fraction_of_8TBps_gathered"] = round(gat / s / PEAK_BW, 4)
        out["bound"] = "gathered" if gat > alg else "algorithmic"
    return out


def wall(fn, reps=1):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-triple", action="store_true")
    args = ap.parse_args()
    import torch

    from sparse_matrix_mult_amd.synthetic import gen_csr_device
    ctx = default_context()
    names = kernel_names()
    dev = torch.device("cuda", ctx.device)
    S, W, R, ex = args.steps, args.warmup, args.reps, args.exact
    n = 50000
    a_t = gen_csr_device(torch, n, n, 0.01, 1, dev)
    A = ctx.csr_from_torch(n, n, *a_t)
    nnz = A.nnz
    Ah = sp.csr_matrix((a_t[2].cpu().numpy(), a_t[1].cpu().numpy(), a_t[0].cpu().numpy()), shape=(n, n))
    line = {"workload": f"configs[1] A 50000 x 50000 d=0.01 (nnz {nnz}); {'SMM_EXACT' if ex else 'default'} mode", "c1": {}}
    rng = np.random.default_rng(5)
    first = True
    for k in (1, 8, 64, 256):
        Xh = rng.uniform(-1, 1, (n, k))
        X = torch.from_numpy(Xh).to(dev)
        Y = torch.empty((n, k), dtype=torch.float64, device=dev)
        res = {}
        for tr in (False, True):
            call = lambda: ctx.spmm_into(A, X, k, k, Y, k, transpose=tr, exact=ex)  # noqa: E731
            if tr and first:                    # the first transposed call on A's handle builds A^T
                ctx.timing(True); ctx.timing_reset()
                t0 = time.perf_counter()
                call()
                split = {nm: round(ctx.kernel_time(nm)[0], 3) for nm in names if ctx.kernel_time(nm)[1]}
                ctx.timing(False)
                line["c1"]["first_transposed_call_with_at_build"] = {
                    "k": k, "ms_call": round((time.perf_counter() - t0) * 1e3, 3),
                    "ms_transpose_kernels": round(sum(v for nm, v in split.items() if "transpose" in nm or "seg_sort" in nm or "scan" in nm), 3),
                    "split": split}
                first = False
            r = timed(ctx, call, S, W, R, names)
            r.update(roofline(r["ms_kernels"], nnz, n, n, k))
            res["AtX" if tr else "AX"] = r
        # baseline on the device today: A times X as a CSR, dense result (X uploaded once, outside the timing)
        xc = ctx.csr_from_scipy(sp.csr_matrix(Xh))
        res["spgemm_dense_baseline"] = timed(ctx, lambda: ctx.dense_into(A, xc, Y.data_ptr(), exact=ex), S, W, R, names)
        xc.close()
        # torch's sparse CSR x dense on the same device
        try:
            At = torch.sparse_csr_tensor(a_t[0].to(torch.int64), a_t[1].to(torch.int64), a_t[2], size=(n, n))
            fn = lambda: torch.matmul(At, X)  # noqa: E731
            fn(); torch.cuda.synchronize()
            ts = []
            for _ in range(R):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(S):
                    fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / S)
            res["torch_sparse_csr"] = {"ms_call": round(float(np.median(ts)), 3), "spread": [round(min(ts), 3), round(max(ts), 3)]}
            del At
        except Exception as e:                  # (recorded, not hidden)
            res["torch_sparse_csr"] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
        if not args.no_scipy:
            res["scipy_host_AX_ms"] = wall(lambda: Ah @ Xh)
            res["scipy_host_AtX_ms"] = wall(lambda: Ah.T @ Xh)
            from sparse_matrix_mult_amd import set_exact, sparse_dense_multiply
            old = set_exact(ex)
            sparse_dense_multiply(Ah, Xh)       # (operand upload and hash, once)
            res["end_to_end_numpy_AX_ms"] = wall(lambda: sparse_dense_multiply(Ah, Xh), 3)
            set_exact(old)
        line["c1"][f"k{k}"] = res
        del X, Y
        torch.cuda.empty_cache()
    A.close()
    del a_t
    torch.cuda.empty_cache()
    if not args.no_triple:
        nt, K = 200000, 1000000
        H, Q = local_h(nt, K, 1), banded_q(K, 32, 2)
        h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
        tr = {"workload": f"S X = H (Q (H^T X)), H {nt} x {K} (8 per row), Q banded half-width 32 (nnz {Q.nnz})"}
        for k in (1, 16, 64):
            Xh = rng.uniform(-1, 1, (nt, k))
            X = torch.from_numpy(Xh).to(dev)
            Y = torch.empty((nt, k), dtype=torch.float64, device=dev)
            r = timed(ctx, lambda: ctx.triple_apply_into(h, q, X, k, k, Y, k, exact=ex), S, W, R, names)
            # three products: H^T X (K x k out), Q Z1, H Z2
            alg = sum(roofline(0, z, rows, cx, k)["bytes_algorithmic"] for z, rows, cx in
                      ((H.nnz, K, nt), (Q.nnz, K, K), (H.nnz, nt, K)))
            gat = 8 * k * (2 * H.nnz + Q.nnz)
            s = r["ms_kernels"] * 1e-3
            r.update({"bytes_algorithmic": alg, "bytes_gathered": gat, "fraction_of_8TBps_algorithmic": round(alg / s / PEAK_BW, 4),
                      "fraction_of_8TBps_gathered": round(gat / s / PEAK_BW, 4), "bound": "gathered" if gat > alg else "algorithmic"})
            if not args.no_scipy and k <= 16:
                r["scipy_host_ms"] = wall(lambda: H @ (Q @ (H.T @ Xh)))
            tr[f"k{k}"] = r
            del X, Y
        h.close(); q.close()
        line["triple"] = tr
    print(json.dumps(line))


if __name__ == "__main__":
    main()
