"""The training corpus held in memory, and batches cut from it on the device.

`dataset_type: vae_npvc_amd.dataset.resident` selects this module.  Its
`Dataset` is `utt2mel_spk.Dataset` (same files, same `crop_window`, same item
contract) that reads every utterance once at construction into one host fp32
tensor [total_frames, mel], the utterances back to back.  `__getitem__` then
slices that tensor: no file access per item, and the crop is bit-identical to
the parent's (a whole-matrix read sliced [s:e] is the inclusive range read
[s:e-1] the parent asks kaldi_io for).  Any DataLoader over it, with or
without workers, keeps working and gets the cheaper item.

`loader()` goes further: the corpus and the speaker ids are uploaded to the
current device once, at the first iteration, and every batch is cut there by
one `ops.crop_batch` call (vqx_crop_batch: crop, transpose, zero-pad and the
speaker lookup in one launch) on the current stream.  Per batch the host only
takes the indices from the sampler, draws the crop starts and fills three
small arrays that travel in the kernel arguments; nothing is copied on the
stream and nothing synchronises.  bin/train.py uses `loader` when the dataset
module defines it.

Random streams.  With `generator=None` the loader consumes the global torch
generator and Python's `random` exactly as `DataLoader(dataset, num_workers=0,
shuffle=..., batch_size=..., drop_last=..., sampler=...)` does: one int64
draw per `iter()` (the DataLoader iterator's base seed), torch's own
RandomSampler / BatchSampler, and `crop_window` once per item in item order.
The batches are then bit-identical to that DataLoader's.  With a `generator`
(the data-parallel entry passes one per rank beside its `ShardSampler`) the
per-`iter()` draw comes from that generator and seeds a private
`random.Random` for the crop starts, so neither global stream is consumed.
Those per-rank crops differ from the ones DataLoader workers would draw (each
worker seeds its own `random` from the base seed plus its worker id, which is
not reproducible across worker counts either).

The GPU is not touched before `loader()` is first iterated; a forked
DataLoader worker that only calls `__getitem__` never initialises it.
"""
import logging
import random
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler

from . import utt2mel_spk
from .kaldi_io import load_mat

GIB = 1 << 30


class Dataset(utt2mel_spk.Dataset):
    """utt2mel_spk.Dataset with every utterance decoded once into host memory.

    frames   f32 [total_frames, mel]; item i owns rows offsets[i]:offsets[i+1]
    offsets  int64 [n + 1]
    speakers int64 [n]
    `resident_max_gib` (config, default 16) caps the fp32 corpus size."""

    def __init__(self, data_dir, config, valid=False):
        super().__init__(data_dir, config, valid=valid)
        t0 = time.perf_counter()
        max_gib = float(config.get("resident_max_gib", 16))
        lengths = [int(self.utt2num_frames[utt]) for utt, _ in self.utt2spks]
        self.offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.tensor(lengths, dtype=torch.int64).cumsum(0) if lengths else 0
        self.speakers = torch.tensor([int(spk) for _, spk in self.utt2spks], dtype=torch.int64)
        total = int(self.offsets[-1])
        self.frames = None
        for i, (utt, _) in enumerate(self.utt2spks):
            mat = torch.from_numpy(np.array(load_mat(self.feats_scp[utt]))).float()  # (T, mel), the parent's conversion
            if self.frames is None:
                need = total * mat.shape[1] * 4
                if need > max_gib * GIB:
                    raise ValueError(f"resident corpus needs {need / GIB:.3f} GiB ({total} frames x {mat.shape[1]} "
                                     f"x fp32), resident_max_gib is {max_gib:g}")
                self.frames = torch.empty((total, mat.shape[1]), dtype=torch.float32)
            if mat.dim() != 2 or mat.shape[0] < lengths[i] or mat.shape[1] != self.frames.shape[1]:
                raise ValueError(f"{utt}: matrix {tuple(mat.shape)} does not hold utt2num_frames' {lengths[i]} "
                                 f"frames of {self.frames.shape[1]}")
            self.frames[int(self.offsets[i]):int(self.offsets[i + 1])] = mat[:lengths[i]]
        if self.frames is None:
            self.frames = torch.empty((0, 0), dtype=torch.float32)
        self.lengths = lengths
        self._device = {}  # torch.device -> (corpus, speaker table), filled by loader()
        self.load_info = "Resident corpus {}: {} utterances, {} frames, {} bytes, loaded in {:.2f} s".format(
            data_dir, self.num_data, total, self.frames.numel() * 4, time.perf_counter() - t0)
        logging.getLogger("logger").info(self.load_info)  # bin/train.py repeats it once its log file is open

    def __getstate__(self):  # spawned workers get the host corpus, never a device handle
        return dict(self.__dict__, _device={})

    def crop_window(self, feat_length, rng=random):
        """The parent's window with the start drawn from `rng` (Python's global
        generator by default, as the parent draws it)."""
        if rng is random or feat_length <= self.crop_length or self.valid:
            return super().crop_window(feat_length)
        start = rng.randint(0, feat_length - self.crop_length)
        return start, start + self.crop_length

    def __getitem__(self, index):
        feat_length = self.lengths[index]
        start, end = self.crop_window(feat_length)
        o = int(self.offsets[index])
        feat = self.frames[o + start:o + end].t().contiguous()  # (mel, T), a copy: items never alias the corpus
        if feat_length < self.crop_length:
            feat = F.pad(feat, (0, self.crop_length - feat_length)).data
        return feat, self.speakers[index:index + 1].clone()

    def on_device(self, device):
        """(corpus, speaker table) on `device`, uploaded at the first call."""
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = (self.frames.to(device), self.speakers.to(device))
        return self._device[device]


class Loader:
    """Iterable of (x (B, mel, T) f32, y (B, 1) int64) on the current device,
    each cut by one ops.crop_batch call on the current stream (module
    docstring: the random streams it consumes)."""

    def __init__(self, dataset, batch_size, shuffle=False, drop_last=False, sampler=None, generator=None):
        if sampler is not None and shuffle:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        if dataset.frames.numel() == 0:
            raise ValueError("resident.loader: the corpus is empty")
        self.dataset, self.generator = dataset, generator
        if sampler is None:
            sampler = RandomSampler(dataset, generator=generator) if shuffle else SequentialSampler(dataset)
        self.sampler = sampler
        self.batch_sampler = BatchSampler(sampler, batch_size, drop_last)

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        # the draw DataLoader's iterator makes when it is created (its base seed)
        seed = int(torch.empty((), dtype=torch.int64).random_(generator=self.generator).item())
        rng = random if self.generator is None else random.Random(seed)
        return self._batches(rng)

    def _plans(self, rng):
        """Host side of an epoch: per batch the utterance indices, the first
        corpus row and the length of every crop (crop_window in item order)."""
        ds = self.dataset
        offsets, lengths = ds.offsets.tolist(), ds.lengths
        for idx in self.batch_sampler:
            row0, length = [], []
            for i in idx:
                start, end = ds.crop_window(lengths[i], rng)
                row0.append(offsets[i] + start)
                length.append(end - start)
            yield idx, row0, length

    def _batches(self, rng):
        from .. import ops
        device = torch.device("cuda", torch.cuda.current_device())
        corpus, spk_table = self.dataset.on_device(device)
        mel, T = corpus.shape[1], self.dataset.crop_length
        for idx, row0, length in self._plans(rng):
            x = torch.empty((len(idx), mel, T), dtype=torch.float32, device=device)
            y = torch.empty((len(idx), 1), dtype=torch.int64, device=device)
            ops.crop_batch(corpus, spk_table, torch.tensor(row0, dtype=torch.int64),
                           torch.tensor(length, dtype=torch.int32), torch.tensor(idx, dtype=torch.int32), x, y)
            yield x, y


def loader(dataset, batch_size, shuffle=False, drop_last=False, sampler=None, generator=None):
    """The device-side replacement of `DataLoader(dataset, ...)`: see Loader."""
    return Loader(dataset, batch_size, shuffle=shuffle, drop_last=drop_last, sampler=sampler, generator=generator)
