"""CPU: bench.py's option surface and its --dump-outputs writer (the GPU run itself: tests/test_gpu_boundary.py)."""
import sys

import numpy as np
import torch

import bench


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_writes_every_output_as_float32(tmp_path):
    out = {"mel": torch.randn(2, 5, 3), "tgt_mask": torch.tensor([[False, True]]), "duration_rounded": torch.tensor([[3, 4]], dtype=torch.int32),
           "variances_pitch": {"reconstructed_signal": torch.ones(2, 5), "mean": torch.zeros(2)}}
    bench.dump_outputs(out, str(tmp_path / "d"))
    got = {p.name for p in (tmp_path / "d").iterdir()}
    assert got == {"mel.npy", "tgt_mask.npy", "duration_rounded.npy", "variances_pitch.reconstructed_signal.npy", "variances_pitch.mean.npy"}
    mel = np.load(tmp_path / "d" / "mel.npy")
    assert mel.dtype == np.float32 and np.array_equal(mel, out["mel"].numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "tgt_mask.npy"), np.array([[0.0, 1.0]], np.float32))
    assert np.array_equal(np.load(tmp_path / "d" / "duration_rounded.npy"), np.array([[3.0, 4.0]], np.float32))


def test_dump_over_the_limit_is_a_fixed_sample_within_it(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    out = {"mel": big, "small": torch.ones(4)}
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d))
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= 4096 + 4 * 128   # + the .npy headers
    idx = np.load(tmp_path / "a" / "mel.index.npy")
    vals = np.load(tmp_path / "a" / "mel.npy")
    assert vals.dtype == np.float32 and len(vals) == len(idx) > 0 and np.all(np.diff(idx) > 0)
    assert np.array_equal(vals, big.numpy().reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), np.ones(4, np.float32))
    for p in (tmp_path / "a").iterdir():
        assert np.array_equal(np.load(p), np.load(tmp_path / "b" / p.name)), p.name

