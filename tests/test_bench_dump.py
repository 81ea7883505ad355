"""bench.py --dump-outputs: file names, dtypes, the per-array cap and the seeded sample (runs without a GPU)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_dtypes_cap_and_fixed_sample(tmp_path):
    big = torch.arange(bench.DUMP_CAP + 1000, dtype=torch.float32)
    arrays = [("loss", torch.tensor(3.5)), ("half", torch.ones(4, dtype=torch.bfloat16)), ("dbl", torch.ones(3, dtype=torch.float64)), ("big", big)]
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "dbl.npy", "half.npy", "loss.npy"]
    loss, half, dbl = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("loss", "half", "dbl"))
    assert loss.dtype == np.float32 and loss.tolist() == [3.5]
    assert half.dtype == np.float32 and half.tolist() == [1.0] * 4
    assert dbl.dtype == np.float64
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (bench.DUMP_CAP,) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)                          # the same positions every run
    assert np.all(np.diff(a) >= 0) and a.max() <= big.numel() - 1   # sorted flat positions of the source array
