"""Masked products (smm_spgemm_masked, smm_triple_product_sparse_masked) against the unmasked products a user has
today.  One JSON line.

    python scripts/masked_bench.py [--steps N] [--warmup W] [--reps R] [--exact] [--no-triple]

1. BASELINE configs[1] operands (A, B 50 000 x 50 000, d = 0.01, generated on the device).  Masks: identity, band of
   half-width 64, random with density 1e-4.  Each is timed with the path forced (dot, row) and chosen per row (auto).
   The baseline is the unmasked device product (symbolic + numeric, 2.48e9 entries) on the same operands.  The first
   masked call on a fresh handle of B also builds B^T (reported on its own); every later call finds it cached.
2. Masked triple product on the scripts/triple_sparse_bench.py workload (H 200 000 x 1 000 000, Q banded half-width
   32): the diagonal and a band mask against the unmasked sparse_triple_product.
Times are HIP-event sums of every launch of a call (ms_kernels) and host wall time around the call (ms_call), median
over R repetitions of N steps each, with the spread (min, max) of the repetitions."""
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
from sparse_matrix_mult_amd.engine import default_context  # noqa: E402
from triple_sparse_bench import banded_q, kernel_names, local_h  # noqa: E402


def timed(ctx, fn, steps, warmup, reps, names):
    """(median kernel ms, [min, max], median call ms, [min, max], kernel split of the last repetition)."""
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    kms, wms, split = [], [], {}
    for _ in range(reps):
        ctx.timing(True); ctx.timing_reset()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        ctx.synchronize()
        wms.append((time.perf_counter() - t0) * 1e3 / steps)
        split = {}
        for k in names:
            ms, calls = ctx.kernel_time(k)
            if calls:
                split[k] = round(ms / steps, 3)
        kms.append(sum(split.values()))
        ctx.timing(False)
    r = lambda v: round(float(v), 3)  # noqa: E731
    return {"ms_kernels": r(np.median(kms)), "ms_kernels_spread": [r(min(kms)), r(max(kms))],
            "ms_call": r(np.median(wms)), "ms_call_spread": [r(min(wms)), r(max(wms))], "split": split}


def band(n, w):
    return sp.diags([np.ones(n)] * (2 * w + 1), list(range(-w, w + 1)), shape=(n, n), format="csr")


def random_mask(n, density, seed):
    rng = np.random.default_rng(seed)
    k = int(n * n * density)
    key = np.unique(rng.integers(0, n, k).astype(np.int64) * n + rng.integers(0, n, k))
    return sp.csr_matrix((np.ones(key.size), (key // n, key % n)), shape=(n, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--no-triple", action="store_true")
    args = ap.parse_args()
    import torch

    from sparse_matrix_mult_amd.synthetic import gen_csr_device
    ctx = default_context()
    names = kernel_names()
    dev = torch.device("cuda", ctx.device)
    S, W, R, ex = args.steps, args.warmup, args.reps, args.exact
    m = n = 50000
    a_t = gen_csr_device(torch, m, n, 0.01, 1, dev)
    b_t = gen_csr_device(torch, n, n, 0.01, 2, dev)
    A, B = ctx.csr_from_torch(m, n, *a_t), ctx.csr_from_torch(n, n, *b_t)
    line = {"workload": f"configs[1] A, B 50000 x 50000 d=0.01; {'SMM_EXACT' if ex else 'default'} mode", "c1": {}}
    # baseline: the unmasked device product
    plan = ctx.spgemm_plan(A, B, exact=ex)
    nnz = plan.nnz
    plan.close()
    indptr = torch.empty(m + 1, dtype=torch.int64, device=dev)
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    data = torch.empty(nnz, dtype=torch.float64, device=dev)

    def unmasked():
        p = ctx.spgemm_plan(A, B, exact=ex)
        p.numeric_into(indptr.data_ptr(), indices.data_ptr(), data.data_ptr())
        p.close()
    base = timed(ctx, unmasked, S, W, R, names)
    line["c1"]["unmasked"] = dict(base, nnz=int(nnz))
    del indices, data
    torch.cuda.empty_cache()
    masks = {"identity": sp.identity(n, format="csr"), "band64": band(n, 64), "random1e-4": random_mask(n, 1e-4, 3)}
    first = True
    for name, M in masks.items():
        mk = ctx.csr_from_scipy(M)
        out = torch.empty(M.nnz, dtype=torch.float64, device=dev)
        res = {"nnz_mask": int(M.nnz)}
        for mode, label in ((0, "auto"), (1, "dot"), (2, "row")):
            ctx.tune_masked(mode)
            call = lambda: ctx.spgemm_masked_into(A, B, mk, out.data_ptr(), exact=ex)  # noqa: E731
            if first:                     # the first call on B's handle builds B^T
                ctx.timing(True); ctx.timing_reset()
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                split = {k: round(ctx.kernel_time(k)[0], 3) for k in names if ctx.kernel_time(k)[1]}
                ctx.timing(False)
                line["c1"]["first_call_with_bt_build"] = {"mask": name, "mode": label, "ms_call": round((time.perf_counter() - t0) * 1e3, 3),
                                                          "ms_kernels": round(sum(split.values()), 3), "split": split}
                first = False
            res[label] = timed(ctx, call, S, W, R, names)
        ctx.tune_masked(0)
        line["c1"][name] = res
        mk.close()
        del out
    line["c1"]["auto_never_slower_than_unmasked"] = all(
        line["c1"][k]["auto"]["ms_kernels"] <= base["ms_kernels"] for k in masks)
    A.close(); B.close()
    del a_t, b_t
    torch.cuda.empty_cache()
    if not args.no_triple:
        nt, K = 200000, 1000000
        H, Q = local_h(nt, K, 1), banded_q(K, 32, 2)
        h, q = ctx.csr_from_scipy(H), ctx.csr_from_scipy(Q)
        tr = {"workload": f"S = H Q H^T, H {nt} x {K}, Q banded half-width 32"}
        tr["unmasked"] = timed(ctx, lambda: ctx.triple_sparse_torch(h, q, exact=ex), S, W, R, names)
        for name, L in (("diag", sp.identity(nt, format="csr")), ("band16", band(nt, 16))):
            mk = ctx.csr_from_scipy(L)
            tr[name] = timed(ctx, lambda: ctx.triple_sparse_torch(h, q, exact=ex, mask=mk), S, W, R, names)
            tr[name]["nnz_mask_upper"] = int(sp.triu(L).nnz)
            mk.close()
        h.close(); q.close()
        line["triple"] = tr
    print(json.dumps(line))


if __name__ == "__main__":
    main()
