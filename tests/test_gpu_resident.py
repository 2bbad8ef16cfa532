"""The device-resident corpus on the GPU (-m gpu): vqx_crop_batch against
numpy slicing bit for bit, `resident.loader` against the DataLoader it
replaces (batches and random streams), its private streams under a
ShardSampler, and bin/train.py trained through either loader."""
import hashlib
import random
import types

import numpy as np
import pytest
import torch
import yaml
from torch.utils.data import DataLoader

from tests.helpers import cfg_of
from tests.resident_data import CFG, CROP, make_data_dir
from vae_npvc_amd.trainer.basic import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_X, GUARD_Y = 12345.0, -7


def _lens_for(T):
    """len = T, 1, 0, T - 1 and a value inside a 32-frame tile (where T allows them)."""
    straddle = {1: [], 4: [2], 5: [3]}.get(T, [33, T - 20])
    out = []
    for v in [T, 1, 0, T - 1] + straddle:
        if 0 <= v <= T and v not in out:
            out.append(v)
    return out


def _run_crop(B, mel, T, lens, seed):
    """One ops.crop_batch call checked against numpy: every element of x and y
    written (they start as NaN / -1), nothing around them touched."""
    from vae_npvc_amd import ops
    rng = np.random.default_rng(seed)
    n_rows, n_utts = 3 * T + 7, 37
    corpus = rng.standard_normal((n_rows, mel)).astype(np.float32)
    table = rng.integers(-2 ** 40, 2 ** 40, n_utts, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int32)
    assert lens.shape == (B,)
    row0 = np.array([rng.integers(0, n_rows - l + 1) for l in lens], dtype=np.int64)
    row0[0] = 0                          # the first row of the corpus
    if B > 1 or seed % 2:
        row0[-1] = n_rows - lens[-1]     # ... and its last: row0 + len == n_rows exactly
    if B > 1:
        row0[1] = n_rows - lens[1]
    utt = rng.integers(0, n_utts, B).astype(np.int32)
    utt[0], utt[-1] = n_utts - 1, 0
    g = 2 * mel * T + 64                 # guard elements each side
    xbuf = torch.full((g + B * mel * T + g,), GUARD_X, device=DEV)
    ybuf = torch.full((16 + B + 16,), GUARD_Y, dtype=torch.int64, device=DEV)
    x = xbuf[g:g + B * mel * T].view(B, mel, T)
    y = ybuf[16:16 + B].view(B, 1)
    x.fill_(float("nan"))
    y.fill_(-1)
    ops.crop_batch(torch.from_numpy(corpus).to(DEV), torch.from_numpy(table).to(DEV), torch.from_numpy(row0),
                   torch.from_numpy(lens), torch.from_numpy(utt), x, y)
    want = np.zeros((B, mel, T), dtype=np.float32)
    for b in range(B):
        want[b, :, :lens[b]] = corpus[row0[b]:row0[b] + lens[b]].T
    got = x.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # bit for bit, the sign of a zero included
    assert np.array_equal(y.cpu().numpy().reshape(-1), table[utt])
    xb, yb = xbuf.cpu(), ybuf.cpu()
    assert bool((xb[:g] == GUARD_X).all()) and bool((xb[g + B * mel * T:] == GUARD_X).all())
    assert bool((yb[:16] == GUARD_Y).all()) and bool((yb[16 + B:] == GUARD_Y).all())


@pytest.mark.parametrize("B,mel,T", [(1, 1, 1), (3, 7, 5), (5, 24, 70), (2, 80, 256), (2, 33, 65)])
def test_crop_batch_equals_numpy_slicing(B, mel, T):
    lens = _lens_for(T)
    # every listed length in every item position, B at a time
    for k in range(len(lens)):
        _run_crop(B, mel, T, [lens[(k + j) % len(lens)] for j in range(B)], seed=100 * T + k)
    if B == 5:  # mixed item lengths
        _run_crop(B, mel, T, [70, 13, 64, 0, 47], seed=1)
        _run_crop(B, mel, T, [32, 31, 33, 69, 1], seed=2)


def test_crop_batch_more_items_than_one_launch_holds():
    lens = [(4, 1, 0, 3, 2)[j % 5] for j in range(300)]
    _run_crop(300, 8, 4, lens, seed=3)
    _run_crop(193, 8, 4, lens[:193], seed=4)   # one item past a full argument block
    _run_crop(192, 8, 4, lens[:192], seed=5)   # exactly one block


def test_crop_batch_refuses_a_bad_item_and_writes_nothing():
    from vae_npvc_amd import _lib as L, ops
    corpus = torch.zeros(10, 4, device=DEV)
    table = torch.zeros(3, dtype=torch.int64, device=DEV)
    x = torch.full((2, 4, 8), 5.0, device=DEV)
    y = torch.full((2, 1), 5, dtype=torch.int64, device=DEV)
    with pytest.raises(L.VqxError, match="item 1: rows"):
        ops.crop_batch(corpus, table, torch.tensor([0, 3]), torch.tensor([8, 8], dtype=torch.int32),
                       torch.tensor([0, 1], dtype=torch.int32), x, y)
    assert bool((x == 5.0).all()) and bool((y == 5).all())


def _epochs(loader, n):
    return [(x, y) for _ in range(n) for x, y in loader]


@pytest.mark.parametrize("valid,shuffle,drop_last", [(False, True, True), (True, False, False)])
def test_loader_equals_the_dataloader_it_replaces(tmp_path, valid, shuffle, drop_last):
    """Same seeds: 2 epochs of batches bit-identical to DataLoader(num_workers=0)
    over the file-reading parent, and both global random streams left in the
    same state.  The validation form ends on a ragged batch (12 = 5 + 5 + 2)."""
    from vae_npvc_amd.dataset import resident, utt2mel_spk
    make_data_dir(tmp_path)
    par = utt2mel_spk.Dataset(tmp_path, CFG, valid=valid)
    res = resident.Dataset(tmp_path, CFG, valid=valid)
    torch.manual_seed(3)
    random.seed(4)
    dl = DataLoader(par, num_workers=0, shuffle=shuffle, batch_size=5, drop_last=drop_last)
    want = _epochs(dl, 2)
    state = (torch.get_rng_state(), random.getstate())
    torch.manual_seed(3)
    random.seed(4)
    ld = resident.loader(res, batch_size=5, shuffle=shuffle, drop_last=drop_last)
    assert res._device == {}  # nothing uploaded before the first iteration
    got = _epochs(ld, 2)
    assert torch.equal(torch.get_rng_state(), state[0]) and random.getstate() == state[1]
    assert len(ld) == len(dl) and len(got) == len(want) == 2 * len(dl)
    assert [tuple(x.shape) for x, _ in got] == [tuple(x.shape) for x, _ in want]
    if not drop_last:
        assert got[-1][0].shape[0] == 2
    for (x, y), (xr, yr) in zip(got, want):
        assert x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.int64
        assert x.is_contiguous() and y.shape == yr.shape
        assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
    assert len(res._device) == 1  # one upload, shared by both epochs


def test_loader_with_a_shard_sampler_keeps_to_private_streams(tmp_path):
    from vae_npvc_amd.dataset import resident
    from vae_npvc_amd.dataset.sampler import ShardSampler
    make_data_dir(tmp_path)
    res = resident.Dataset(tmp_path, CFG)
    torch.manual_seed(11)
    random.seed(12)
    state = (torch.get_rng_state(), random.getstate())
    seen = []
    for rank in range(2):
        def make():
            s = ShardSampler(res, 2, rank, shuffle=True, seed=9, drop_last=True)
            return s, resident.loader(res, batch_size=4, shuffle=False, drop_last=False, sampler=s,
                                      generator=torch.Generator().manual_seed(5 + rank))
        (s1, l1), (s2, l2) = make(), make()
        for epoch in range(2):
            s1.set_epoch(epoch)
            s2.set_epoch(epoch)
            order = list(s1)
            b1, b2 = list(l1), list(l2)
            assert len(b1) == len(l1) == 2 and [len(y) for _, y in b1] == [4, 2]
            for (x, y), (x2, y2) in zip(b1, b2):  # equal seeds: equal batches
                assert torch.equal(x, x2) and torch.equal(y, y2)
            xs, ys = torch.cat([x for x, _ in b1]).cpu(), torch.cat([y for _, y in b1]).cpu()
            for pos, i in enumerate(order):  # every item is a crop of the utterance the sampler named
                assert int(ys[pos]) == int(res.speakers[i])
                o, n = int(res.offsets[i]), res.lengths[i]
                if n <= CROP:
                    want = torch.zeros(res.frames.shape[1], CROP)
                    want[:, :n] = res.frames[o:o + n].t()
                    assert torch.equal(xs[pos], want)
                else:
                    assert any(torch.equal(xs[pos], res.frames[o + s:o + s + CROP].t()) for s in range(n - CROP + 1))
            seen.append(order)
    assert not set(seen[0]) & set(seen[2]) and seen[0] != seen[1]  # disjoint ranks, a new order per epoch
    assert torch.equal(torch.get_rng_state(), state[0]) and random.getstate() == state[1]


class RecTrainer(Trainer):
    """The Trainer, keeping every step's loss dict."""

    def train_step(self, input, iteration=None):
        iteration, loss_detail = super().train_step(input, iteration=iteration)
        self.__dict__.setdefault("steps", []).append(dict(loss_detail))
        return iteration, loss_detail


def test_train_entry_trains_the_same_through_either_loader(tmp_path):
    """bin/train.py for 7 iterations (epochs of 2 batches, two checkpoints with
    a validation each) with `dataset_type: vae_npvc_amd.dataset.resident` and with the
    default dataset on DataLoader(num_workers=0): the same loss dict at every
    step, the same validation losses, the same parameters at the end."""
    from vae_npvc_amd.bin import train as entry
    lengths = [40, 200, 64, 63, 65, 128, 90, 70]
    for d in ("train", "valid"):
        (tmp_path / d).mkdir()
    make_data_dir(tmp_path / "train", lengths=lengths, mel=80)
    make_data_dir(tmp_path / "valid", lengths=[64, 30, 100], mel=80, seed=6)
    runs = {}
    for name, dataset_type in (("resident", "vae_npvc_amd.dataset.resident"), ("default", None)):
        cfg = cfg_of("vcc20", compute_dtype="fp32", batch_size=3, max_iter=6, iters_per_log=2, iters_per_checkpoint=3,
                     crop_length=64, num_jobs=0, trainer_type="tests.test_gpu_resident:RecTrainer")
        if dataset_type is None:
            assert cfg["dataset_type"] == "vae_npvc_amd.dataset.utt2mel_spk"
        else:
            cfg["dataset_type"] = dataset_type
        path = tmp_path / f"{name}.yaml"
        yaml.safe_dump(cfg, open(path, "w"))
        args = types.SimpleNamespace(config=str(path), output_dir=str(tmp_path / name), checkpoint=None,
                                     train_dir=str(tmp_path / "train"), valid_dir=str(tmp_path / "valid"),
                                     backend=None)
        random.seed(21)  # the crop starts: Python's global generator, which the entry does not seed
        tr = entry.train(args)
        assert tr.iteration == 7
        ck = torch.load(tmp_path / name / "iter.6", map_location="cpu", weights_only=True)
        h = hashlib.sha256()
        for k in sorted(ck["model"]):
            h.update(k.encode() + ck["model"][k].contiguous().numpy().tobytes())
        log = (tmp_path / name / "train.log").read_text()
        runs[name] = dict(steps=tr.steps, hash=h.hexdigest(), final=(torch.get_rng_state(), random.getstate()),
                          lines=[l.split(" ", 2)[2] for l in log.splitlines() if " Iter " in l or " Valid " in l])
    a, b = runs["resident"], runs["default"]
    assert len(a["steps"]) == len(b["steps"]) == 7 and set(a["steps"][0]) >= {"Total", "X like", "VQ loss"}
    assert a["steps"] == b["steps"]
    assert len(a["lines"]) == 5 and a["lines"] == b["lines"]  # Iter 2, 4, 6 and Valid 3, 6
    assert a["hash"] == b["hash"]
    assert torch.equal(a["final"][0], b["final"][0]) and a["final"][1] == b["final"][1]
    assert "Resident corpus" in (tmp_path / "resident" / "train.log").read_text()
