"""Voice conversion over a decode directory with the hierarchical model
(`model_type: vae_npvc_amd.model.vqvae2`): `decoder.basic.Decoder` with the
conversion step `model.convert((feat (1, mel, T), target (1, 1)))`, which takes
utterances of any length one at a time.  A recipe selects it with

    decoder_type: vae_npvc_amd.decoder.hier

`decode_batch_size: N` (default 1: the loop above, unchanged) converts up to N
trials per call as one padded batch, `model.convert((x, y), lengths=...)`.
Trials are read `N * WINDOW_BATCHES` at a time in trial order; inside such a
window they are sorted by length and cut into batches of N neighbours, so an
utterance is padded only to the longest of its N neighbours and at most one
window of features is held on the host.  A source utterance listed with
several targets fills several slots.  The window is written out in trial
order, so `feats.ark` / `feats.scp` keep the order of `trials`.
"""
import inspect
import logging
from pathlib import Path

import numpy as np
import torch

from ..dataset.kaldi_io import WriteHelper, load_mat
from .basic import Decoder as _Decoder

logger = logging.getLogger()

WINDOW_BATCHES = 8  # batches formed from one window of trials


class Decoder(_Decoder):
    def __init__(self, config):
        super().__init__(config)
        n = config.get("decode_batch_size", 1)
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"decode_batch_size must be a positive integer, got {n!r}")
        if n > 1 and "lengths" not in inspect.signature(self.model.convert).parameters:
            raise NotImplementedError(f"decode_batch_size {n}: {type(self.model).__module__}.Model.convert takes no "
                                      "`lengths` (batches of different lengths are built for vqvae2 only)")
        self.decode_batch_size = n

    def decode_step(self, feat, spk):
        return self.model.convert((feat, spk))

    def decode_batch(self, feats, targets):
        """feats: (T_b, mel) host arrays, targets: speaker ids -> the converted (T_b, mel) arrays."""
        lens = [f.shape[0] for f in feats]
        x = np.zeros((len(feats), feats[0].shape[1], max(lens)), dtype=np.float32)
        for b, f in enumerate(feats):
            x[b, :, :lens[b]] = f.T
        y = torch.tensor(targets).long().view(-1, 1).to(self.device)
        out = self.model.convert((torch.from_numpy(x).to(self.device), y), lengths=lens).cpu().numpy()
        return [np.ascontiguousarray(out[b, :, :n].T) for b, n in enumerate(lens)]

    def decode_batched(self, decode_dir, output_dir, compress=True):
        """`decode` for decode_batch_size > 1 (decoder.basic.Decoder.decode hands over to it)."""
        N = self.decode_batch_size
        decode_dir = Path(decode_dir)
        for file in ["trials", "feats.scp"]:
            if not (decode_dir / file).is_file():
                raise FileNotFoundError(f"No such file {decode_dir / file}")
        trials = [line.strip().split(None, 1) for line in open(decode_dir / "trials") if line.strip()]
        feats_scp = dict(line.strip().split(None, 1) for line in open(decode_dir / "feats.scp") if line.strip())
        spk2spk_id = None
        if (decode_dir / "spk2spk_id").exists():
            spk2spk_id = dict(line.strip().split(None, 1) for line in open(decode_dir / "spk2spk_id") if line.strip())
        wspecifier = "ark,scp:{0}/feats.ark,{0}/feats.scp".format(str(output_dir))
        with WriteHelper(wspecifier, compression_method=1 if compress else None) as wf:
            for w0 in range(0, len(trials), N * WINDOW_BATCHES):
                window = trials[w0:w0 + N * WINDOW_BATCHES]
                loaded, feats, targets = {}, [], []
                for utt, target in window:
                    if utt not in loaded:  # one read for an utterance listed with several targets
                        loaded[utt] = np.array(load_mat(feats_scp[utt]), dtype=np.float32)
                    feats.append(loaded[utt])
                    ids = [int(spk2spk_id[t]) if spk2spk_id else int(t) for t in target.split()]
                    if len(ids) != 1:
                        raise ValueError(f"trial {utt}: one target speaker per utterance, got {ids}")
                    targets.append(ids[0])
                order = sorted(range(len(window)), key=lambda k: feats[k].shape[0])  # stable: ties keep trial order
                done = [None] * len(window)
                for k0 in range(0, len(order), N):
                    pick = order[k0:k0 + N]
                    logger.info(f"Decode {[w0 + k for k in pick]}: {[window[k][0] for k in pick]} to "
                                f"{[window[k][1] for k in pick]}")
                    for k, f in zip(pick, self.decode_batch([feats[k] for k in pick], [targets[k] for k in pick])):
                        done[k] = f
                for (utt, _), f in zip(window, done):
                    wf[utt] = f
