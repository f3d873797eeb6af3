"""bench.py --dump-outputs on the host: an output larger than the byte cap is written as a fixed seeded sample of whole hops."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_output_samples_whole_hops_the_same_way_every_time(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    H, hops = bench.HOP, 1000
    y = torch.arange(hops * H, dtype=torch.float32).reshape(1, hops * H)
    bench.dump_output(str(tmp_path / "a"), "y", y, 100 * H * 4)
    bench.dump_output(str(tmp_path / "b"), "y", y, 100 * H * 4 + 7)
    bench.dump_output(str(tmp_path / "c"), "y", y, hops * H * 4)
    a, b, c = (np.load(tmp_path / d / "y.npy") for d in "abc")
    assert a.dtype == np.float32 and a.shape == (100, H) and a.nbytes <= 100 * H * 4
    first = a[:, 0].astype(np.int64) // H                    # which hop each row is
    assert np.array_equal(a, (first[:, None] * H + np.arange(H)).astype(np.float32))
    assert (np.diff(first) > 0).all() and first[-1] - first[0] > hops // 2   # distinct, in stream order, spread over the output
    assert np.array_equal(a, b)                              # the pick depends only on the output's size
    assert np.array_equal(c, y.numpy())                      # what fits is written whole, in its own shape
