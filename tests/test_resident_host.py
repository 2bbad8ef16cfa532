"""The resident corpus without a GPU: `resident.Dataset` items equal the
file-reading parent's bit for bit with the same random draws, its offsets and
frame count are right and its size cap is enforced; vqx_crop_batch refuses
every bad argument on the host before any launch; bin/train.py builds its
loaders through a dataset module's `loader` when there is one."""
import ctypes
import random
import sys
import types

import numpy as np
import pytest
import torch
import yaml

from tests.resident_data import CFG, CROP, LENGTHS, MEL, make_data_dir
from vae_npvc_amd.dataset import kaldi_io as K


@pytest.mark.parametrize("valid", [False, True])
@pytest.mark.parametrize("compression", [None, K.K_SPEECH_FEATURE])
def test_items_equal_the_parents_bit_for_bit(tmp_path, valid, compression):
    from vae_npvc_amd.dataset import resident, utt2mel_spk
    make_data_dir(tmp_path, compression=compression)
    par = utt2mel_spk.Dataset(tmp_path, CFG, valid=valid)
    res = resident.Dataset(tmp_path, CFG, valid=valid)
    assert isinstance(res, utt2mel_spk.Dataset) and len(res) == len(par) == len(LENGTHS)
    for rep in range(3):
        order = list(range(len(par))) if rep == 0 else random.Random(rep).sample(range(len(par)), len(par))
        random.seed(40 + rep)
        want = [par[i] for i in order]
        state_par = random.getstate()
        random.seed(40 + rep)
        got = [res[i] for i in order]
        assert random.getstate() == state_par  # the same draws, so the same stream afterwards
        for (x, y), (xr, yr) in zip(got, want):
            assert x.shape == xr.shape == (MEL, CROP) and x.dtype == xr.dtype == torch.float32
            assert torch.equal(x, xr)
            assert y.shape == yr.shape == (1,) and y.dtype == torch.int64 and torch.equal(y, yr)
    x, _ = res[0]
    x.fill_(7.0)  # an item is a copy: writing to it leaves the corpus alone
    assert torch.equal(res[0][0], par[0][0])


def test_offsets_frames_and_speakers(tmp_path):
    from vae_npvc_amd.dataset import resident
    mats = make_data_dir(tmp_path)
    res = resident.Dataset(tmp_path, CFG)
    assert res.offsets.dtype == torch.int64 and res.offsets.tolist() == [0] + np.cumsum(LENGTHS).tolist()
    assert res.frames.shape == (sum(LENGTHS), MEL) and res.frames.dtype == torch.float32
    assert res.frames.is_contiguous() and not res.frames.is_cuda
    assert np.array_equal(res.frames.numpy(), np.concatenate(mats))
    assert res.speakers.dtype == torch.int64
    assert res.speakers.tolist() == [(i * 7) % 5 + 11 for i in range(len(LENGTHS))]
    assert str(sum(LENGTHS)) in res.load_info and str(len(LENGTHS)) in res.load_info
    assert res._device == {}  # nothing on a device before loader() is iterated


def test_size_cap_raises_with_the_size_needed(tmp_path):
    from vae_npvc_amd.dataset import resident
    make_data_dir(tmp_path)
    need = sum(LENGTHS) * MEL * 4
    with pytest.raises(ValueError, match="GiB"):
        resident.Dataset(tmp_path, dict(CFG, resident_max_gib=(need - 1) / 2 ** 30))
    resident.Dataset(tmp_path, dict(CFG, resident_max_gib=need / 2 ** 30))  # exactly enough


def test_pickled_dataset_carries_no_device_handle(tmp_path):
    import pickle
    from vae_npvc_amd.dataset import resident
    make_data_dir(tmp_path)
    res = resident.Dataset(tmp_path, CFG, valid=True)
    res._device["sentinel"] = object()
    back = pickle.loads(pickle.dumps(res))
    assert back._device == {} and torch.equal(back[1][0], res[1][0])


def _crop_args(**over):
    """A valid vqx_crop_batch call on fake device pointers (n_rows 100, mel 8,
    n_utts 4, B 3, T 16) with `over` replacing arguments; the host arrays are real."""
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    a = dict(corpus=fake, n_rows=100, mel=8, spk=fake, n_utts=4, row0=[0, 50, 84], len=[16, 1, 16], utt=[0, 3, 1],
             B=3, T=16, x=fake, y=fake)
    a.update(over)
    row0 = (ctypes.c_int64 * len(a["row0"]))(*a["row0"])
    ln = (ctypes.c_int32 * len(a["len"]))(*a["len"])
    utt = (ctypes.c_int32 * len(a["utt"]))(*a["utt"])
    keep = (row0, ln, utt)
    return keep, (a["corpus"], a["n_rows"], a["mel"], a["spk"], a["n_utts"], ctypes.addressof(row0),
                  ctypes.addressof(ln), ctypes.addressof(utt), a["B"], a["T"], a["x"], a["y"], None)


@pytest.mark.parametrize("over,match", [
    (dict(len=[16, 17, 16]), r"item 1: len 17"),
    (dict(len=[16, 1, -1]), r"item 2: len -1"),
    (dict(row0=[-1, 50, 84]), r"item 0: rows"),
    (dict(row0=[0, 50, 85]), r"item 2: rows"),        # 85 + 16 = 101 > 100
    (dict(row0=[0, 100, 84]), r"item 1: rows"),       # 100 + 1 > 100
    (dict(row0=[0, 2 ** 62, 84]), r"item 1: rows"),
    (dict(utt=[0, 4, 1]), r"item 1: utt 4"),
    (dict(utt=[0, 3, -1]), r"item 2: utt -1"),
    (dict(mel=0), r"bad sizes"),
    (dict(T=0, len=[0, 0, 0]), r"bad sizes"),
    (dict(B=0), r"bad sizes"),
    (dict(x=None), r"null"),
    (dict(spk=None), r"null"),
])
def test_crop_batch_refuses_bad_arguments_before_any_launch(over, match):
    from vae_npvc_amd import _lib as L
    keep, args = _crop_args(**over)
    with pytest.raises(L.VqxError, match=match):
        L.call("vqx_crop_batch", *args)
    del keep


def test_crop_batch_is_declared_exported_and_bound():
    import re
    from tests.helpers import ROOT
    from vae_npvc_amd import _lib as L, ops
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vqx.h").read_text(), flags=re.S)
    assert re.search(r"^\s*int\s+vqx_crop_batch\s*\(", header, flags=re.M)
    assert "vqx_crop_batch" in L._SIGS and hasattr(lib, "vqx_crop_batch") and "vqx_crop_batch" in L.EXPORTS
    assert len(L._SIGS["vqx_crop_batch"]) == 13 and callable(ops.crop_batch)
    t = torch.zeros(2, 3)  # host tensors are refused: there is no CPU path
    with pytest.raises(L.VqxError, match="device tensors"):
        ops.crop_batch(t, t, t, t, t, t, t)


def _train_args(tmp_path, cfg):
    path = tmp_path / "conf.yaml"
    yaml.safe_dump(cfg, open(path, "w"))
    return types.SimpleNamespace(config=str(path), output_dir=str(tmp_path / "exp"), checkpoint=None,
                                 train_dir="train", valid_dir="valid", backend=None)


@pytest.mark.parametrize("with_loader", [True, False])
def test_train_entry_uses_a_dataset_modules_loader(tmp_path, monkeypatch, with_loader):
    """A dataset module with a `loader` attribute supplies both loaders (with
    the values bin/train.py gives DataLoader); one without it gets DataLoader."""
    from torch.utils.data import DataLoader

    from tests import ddp_stubs
    from vae_npvc_amd.bin import train as entry
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    calls = {"loader": [], "DataLoader": []}

    def loader(dataset, **kw):
        calls["loader"].append((len(dataset), kw))
        return DataLoader(dataset, num_workers=0, **kw)

    def data_loader(dataset, **kw):
        calls["DataLoader"].append((len(dataset), kw))
        return DataLoader(dataset, **kw)

    mod = types.ModuleType("resident_stub")
    mod.Dataset = ddp_stubs.Utts
    if with_loader:
        mod.loader = loader
    monkeypatch.setitem(sys.modules, "resident_stub", mod)
    monkeypatch.setattr(entry, "DataLoader", data_loader)
    cfg = dict(trainer_type="tests.ddp_stubs:Trainer", dataset_type="resident_stub", n_utts=9, n_valid=5,
               batch_size=2, max_iter=5, iters_per_log=2, iters_per_checkpoint=4, num_jobs=0, seed=777)
    tr = entry.train(_train_args(tmp_path, cfg))
    assert [it for it, _ in tr.seen] == [1, 2, 3, 4, 5, 6] and tr.valids == 1
    if with_loader:
        assert calls["DataLoader"] == []
        (n_train, kw_train), (n_valid, kw_valid) = calls["loader"]
        assert n_train == 9 and kw_train == dict(batch_size=2, shuffle=True, drop_last=True)
        assert n_valid == 5 and kw_valid == dict(batch_size=2, shuffle=False, drop_last=False)
    else:
        assert calls["loader"] == []
        (n_train, kw_train), (n_valid, kw_valid) = calls["DataLoader"]
        assert n_train == 9 and kw_train == dict(num_workers=0, shuffle=True, batch_size=2, pin_memory=True,
                                                 drop_last=True, collate_fn=None)
        assert n_valid == 5 and kw_valid["shuffle"] is False and kw_valid["num_workers"] == 0
    # the two paths feed the trainer the same batches: same seeds, same draws
    ref = types.ModuleType("resident_stub")
    ref.Dataset = ddp_stubs.Utts
    monkeypatch.setitem(sys.modules, "resident_stub", ref)
    monkeypatch.setattr(entry, "DataLoader", DataLoader)
    tr_ref = entry.train(_train_args(tmp_path, cfg))
    assert tr_ref.seen == tr.seen
