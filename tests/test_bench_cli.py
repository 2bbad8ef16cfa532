"""bench.py's command line (no GPU): what a plain run leaves out, what --full
brings back, and the files --dump-outputs writes."""
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_times_the_steps_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_probe and a.no_cpu_baseline and not a.read_loss
    assert a.vq_reps == 0 and a.fp32_steps == 0


def test_full_run_keeps_every_leg_and_its_switch(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not a.no_probe and not a.no_cpu_baseline and a.read_loss
    assert a.vq_reps > 0 and a.fp32_steps > 0 and a.cpu_steps > 0
    a = _parse(monkeypatch, "--full", "--no-probe", "--vq-reps", "0", "--no-read-loss")
    assert a.no_probe and a.vq_reps == 0 and not a.read_loss and a.fp32_steps > 0


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float_arrays_with_a_fixed_sample(tmp_path):
    n = bench.DUMP_PARAM_SAMPLE + 12345
    flat = torch.arange(n, dtype=torch.float32)
    emb = torch.randn(8, 4)
    tr = SimpleNamespace(model=SimpleNamespace(quantizer=SimpleNamespace(embeddings=emb)),
                         engine=SimpleNamespace(flat_p=flat))
    det = {"Total": 1.5, "VQ loss": 0.25}
    bench.dump_outputs(str(tmp_path / "a"), tr, det)
    bench.dump_outputs(str(tmp_path / "b"), tr, det)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["codebook.npy", "loss_Total.npy", "loss_VQ_loss.npy", "params.npy"]
    total = 0
    for name in names:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 << 20
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.shape == (bench.DUMP_PARAM_SAMPLE,) and (np.diff(p) >= 0).all() and p.max() < n
    assert np.load(tmp_path / "a" / "loss_VQ_loss.npy").tolist() == [0.25]
    assert np.array_equal(np.load(tmp_path / "a" / "codebook.npy"), emb.numpy())
    # a parameter vector below the sample size is written whole
    tr.engine.flat_p = flat[:1000]
    bench.dump_outputs(str(tmp_path / "c"), tr, det)
    assert np.array_equal(np.load(tmp_path / "c" / "params.npy"), flat[:1000].numpy())
