"""bench.py's command line and its output dump (no GPU): --full is off by default, and --dump-outputs
writes every 32-bit CRC exactly (float64, read as unsigned)."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("ambry_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"


def test_dump_outputs_is_exact(tmp_path):
    import torch

    bench = _bench()
    crc = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xCBF43926, 0xFFFFFFFF], dtype=np.uint32)
    flags = np.array([0, 1, 0, 1, 1, 0], dtype=np.uint8)
    out = tmp_path / "dump" / "nested"
    bench.dump_outputs(str(out), {"crc32": torch.from_numpy(crc.view(np.int32)), "mismatch": torch.from_numpy(flags)})
    got = np.load(out / "crc32.npy")
    assert got.dtype == np.float64 and np.array_equal(got, crc.astype(np.float64))
    got = np.load(out / "mismatch.npy")
    assert got.dtype == np.float64 and np.array_equal(got, flags.astype(np.float64))
    assert sorted(os.listdir(out)) == ["crc32.npy", "mismatch.npy"]
