"""bench.py --dump-outputs: the sample of a large output is bounded, the same from run to run, and made of whole rows of what was
computed (both ends of a row kept when one row alone is too large).  Checked on CPU tensors; the GPU path is
tests/test_gpu_bench_contract.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_output_is_dumped_whole():
    t = torch.arange(6 * 10, dtype=torch.float32).reshape(6, 10)
    assert np.array_equal(bench.dump_sample(t, 1 << 20), t.numpy())


def test_large_output_is_a_fixed_sample_of_whole_rows():
    t = torch.arange(1000 * 64, dtype=torch.float64).reshape(1000, 64)
    share = 40 * 64 * 8
    a = bench.dump_sample(t, share)
    assert a.dtype == np.float64 and a.nbytes <= share and a.shape == (40, 64)
    rows = a[:, 0] / 64
    assert np.array_equal(rows, np.round(rows)) and np.all(np.diff(rows) > 0)
    assert np.array_equal(a, t.numpy()[rows.astype(int)])
    assert np.array_equal(a, bench.dump_sample(t, share))


def test_rows_longer_than_the_share_keep_both_ends():
    t = torch.arange(3 * 1000, dtype=torch.float32).reshape(3, 1000)
    a = bench.dump_sample(t, 100 * 4)
    assert a.shape == (1, 100) and a.nbytes <= 400
    r = int(a[0, 0]) // 1000
    assert np.array_equal(a[0], np.concatenate([t.numpy()[r, :50], t.numpy()[r, 950:]]))


def test_dump_writes_npy_files(tmp_path):
    bench.dump_outputs(str(tmp_path / "out"), {"y": np.ones((2, 3), np.float32), "z": np.zeros(4)})
    assert sorted(os.listdir(tmp_path / "out")) == ["y.npy", "z.npy"]
    assert np.load(tmp_path / "out" / "y.npy").dtype == np.float32 and np.load(tmp_path / "out" / "z.npy").dtype == np.float64
