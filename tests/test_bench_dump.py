"""bench.py --dump-outputs: what the timed path computed is written as float32 .npy files, at most 64 MB in all; a larger
output is reduced to a fixed, seeded sample so that two builds' dumps compare element for element."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_small_output_is_written_whole_as_float32(tmp_path):
    y = torch.linspace(-1, 1, 3 * 64 * 48).reshape(1, 3, 64, 48)
    bench.dump_outputs(str(tmp_path), {"output": y})
    got = np.load(tmp_path / "output.npy")
    assert got.dtype == np.float32 and got.shape == (1, 3, 64, 48)
    np.testing.assert_array_equal(got, y.numpy())


def test_uint8_frame_is_written_exactly(tmp_path):
    frame = np.random.default_rng(3).integers(0, 256, size=(40, 30, 3), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), {"output": frame})
    got = np.load(tmp_path / "output.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, frame.astype(np.float32))


def test_large_output_is_a_fixed_sample_under_the_limit(tmp_path):
    n = bench.DUMP_LIMIT_BYTES // 4 + 1                      # one element over the limit as float32
    y = torch.arange(n, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"output": y})
    a, b = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "b" / "output.npy")
    assert a.dtype == np.float32 and a.ndim == 1
    assert 0 < a.nbytes <= bench.DUMP_LIMIT_BYTES and a.size <= bench.DUMP_SAMPLE
    np.testing.assert_array_equal(a, b)                      # the same elements on every run
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and int(a[-1]) < n   # distinct indices, in order, all in range
