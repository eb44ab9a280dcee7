"""bench.py's host-side pieces that need no GPU: the options of a plain run and --dump-outputs' writer."""
import os

import numpy as np

import bench


def test_plain_run_options():
    a = bench.parse_args(["--gpus", "1", "--steps", "9", "--warmup", "2"])
    assert a.steps == 9 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_float32_and_seeded_sample_within_budget(tmp_path):
    """Outputs that fit are written whole, as float32; outputs over the budget keep one fixed, seeded sample of anchors, the same in
    every array and from call to call, and stay within the budget."""
    n = 1000
    idx = np.arange(n, dtype=np.float64)[None, :, None]
    arrays = {"regression": np.broadcast_to(idx, (2, n, 4)) + np.zeros((2, 1, 4)),
              "hand": np.broadcast_to(idx, (2, n, 63)) + np.arange(2.0)[:, None, None]}
    assert bench.dump_outputs(str(tmp_path / "whole"), arrays) == n
    for k, a in arrays.items():
        got = np.load(tmp_path / "whole" / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    budget = 100_000
    keep = bench.dump_outputs(str(tmp_path / "s1"), arrays, budget=budget)
    assert 0 < keep < n and bench.dump_outputs(str(tmp_path / "s2"), arrays, budget=budget) == keep
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= budget
    picked = None
    for k in arrays:
        got = np.load(tmp_path / "s1" / (k + ".npy"))
        assert got.dtype == np.float32 and got.shape[:2] == (2, keep)
        assert (tmp_path / "s1" / (k + ".npy")).read_bytes() == (tmp_path / "s2" / (k + ".npy")).read_bytes()
        anchors = got[0, :, 0]
        assert np.all(np.diff(anchors) > 0) and (picked is None or np.array_equal(anchors, picked))
        picked = anchors
