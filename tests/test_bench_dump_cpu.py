"""bench.py --dump-outputs / --full plumbing on the CPU: arrays land as float32 .npy, a large array is written as the
same seeded sample every time, and --full is off unless asked for."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("rvcx_bench", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    b = _bench()
    x = torch.arange(1000, dtype=torch.float64).reshape(10, 100) / 7.0
    args = argparse.Namespace(dump_outputs=str(tmp_path / "a"))
    b.dump_outputs(args, 0, 1, {"audio": x})
    a = np.load(tmp_path / "a" / "audio.npy")
    assert a.dtype == np.float32 and a.shape == (10, 100)
    np.testing.assert_array_equal(a, x.float().numpy())

    # two arrays share a cap of 800 bytes: 100 float32 elements each, the same elements on every run
    monkeypatch.setattr(b, "DUMP_CAP_BYTES", 800)
    for d in ("b", "c"):
        b.dump_outputs(argparse.Namespace(dump_outputs=str(tmp_path / d)), 1, 2, {"audio": x, "vol": x[0, :50]})
    s1, s2 = np.load(tmp_path / "b" / "audio_rank1.npy"), np.load(tmp_path / "c" / "audio_rank1.npy")
    assert s1.shape == (100,) and s1.dtype == np.float32
    np.testing.assert_array_equal(s1, s2)
    flat = x.float().numpy().reshape(-1)
    assert np.all(np.diff(np.searchsorted(flat, s1)) > 0) and np.all(np.isin(s1, flat))
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "vol_rank1.npy"), flat[:50])
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= 800 + 2 * 128  # payload within the cap (+ the .npy headers)


def test_dump_outputs_off_writes_nothing(tmp_path):
    b = _bench()
    b.dump_outputs(argparse.Namespace(dump_outputs=None), 0, 1, {"audio": torch.zeros(4)})
    assert os.listdir(tmp_path) == []


def test_full_is_off_by_default(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = b.parse()
    assert a.full and a.dump_outputs == "d"
