"""bench.py's host-side pieces, without a GPU: what --dump-outputs writes and the argument checks."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_is_float64_seeded_and_bounded(tmp_path):
    big = bench.DUMP_MAX_ELEMS * 3
    arrays = [("indptr", torch.arange(1001, dtype=torch.int64) * 7),
              ("indices", torch.arange(big, dtype=torch.int32).flip(0)),
              ("data", torch.rand(big, dtype=torch.float64, generator=torch.Generator().manual_seed(1))),
              ("dense", torch.rand(2000, 2000, dtype=torch.float64, generator=torch.Generator().manual_seed(2)))]
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(torch, arrays, str(a))
    bench.dump_outputs(torch, arrays, str(b))
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b))
    assert "indptr_positions.npy" not in files                      # small arrays are written whole
    assert np.array_equal(np.load(a / "indptr.npy"), np.arange(1001) * 7.0)
    total = 0
    for f in files:
        x = np.load(a / f)
        assert x.dtype == np.float64 and np.array_equal(x, np.load(b / f))   # same positions, same values
        total += os.path.getsize(a / f)
    assert total <= 64 << 20
    for name, t in arrays[1:]:
        pos = np.load(a / f"{name}_positions.npy").astype(np.int64)
        assert 0 < len(pos) <= bench.DUMP_MAX_ELEMS and np.all(np.diff(pos) > 0) and pos[-1] < t.numel()
        assert np.array_equal(np.load(a / f"{name}.npy"), t.reshape(-1).numpy()[pos].astype(np.float64))


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr
