"""bench.py's command line on the CPU: --full is off by default, --dump-outputs writes float32 /
float64 .npy files within its byte budget, and the cut of an oversized array is the same in every
call."""
import os
import sys

import numpy as np
import torch


def _parse(monkeypatch, argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = _parse(monkeypatch, ["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_dtypes_and_values(tmp_path):
    import bench

    t = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    d64 = np.linspace(0, 1, 5)
    bench.dump_outputs(str(tmp_path / "o"), {"samples": t, "lp": d64})
    s = np.load(tmp_path / "o" / "samples.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, t.float().numpy())
    lp = np.load(tmp_path / "o" / "lp.npy")
    assert lp.dtype == np.float64 and np.array_equal(lp, d64)


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * 8192)
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    small = torch.ones(4, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "other": big.double()})
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 3 * 8192
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < 5000
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)        # same elements, in the array's order
    assert np.load(tmp_path / "a" / "small.npy").shape == (4, 2)  # within its share: written whole
    o = np.load(tmp_path / "a" / "other.npy")
    assert o.dtype == np.float64 and 0 < o.size < a.size           # the same share holds fewer doubles
