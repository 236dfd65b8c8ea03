"""bench.py --dump-outputs, host side: the writer keeps float64, stores everything else as float32, and past the 64 MB
budget cuts an array to a fixed sample of its elements with the flat indices beside it.  No GPU: only the writer runs."""
import os

import numpy as np
import torch

import bench


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    x = torch.randn(2, 80, 96)
    bench.dump_outputs(str(tmp_path), {"x_prev": x, "loss": torch.tensor(0.5, dtype=torch.float64),
                                       "count": torch.tensor([3, 4])})
    assert sorted(os.listdir(tmp_path)) == ["count.npy", "loss.npy", "x_prev.npy"]
    a = np.load(tmp_path / "x_prev.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.numpy())
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == () and float(loss) == 0.5
    assert np.load(tmp_path / "count.npy").dtype == np.float32


def test_large_outputs_are_a_fixed_sample_within_budget(tmp_path):
    x = torch.randn(24, 80, 10000)                       # 76.8 MB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x_prev": x})
        assert _sizes(tmp_path / d) <= bench.DUMP_BYTES
    idx = np.load(tmp_path / "a" / "x_prev_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "x_prev_index.npy"))
    assert np.all(np.diff(idx) > 0) and idx[-1] < x.numel() and len(idx) > 1_000_000
    vals = np.load(tmp_path / "a" / "x_prev.npy")
    assert vals.dtype == np.float32 and np.array_equal(vals, x.numpy().reshape(-1)[idx.astype(np.int64)])
