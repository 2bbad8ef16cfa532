"""Voice conversion over a decode directory: the
reference's `vae_npvc.decoder.basic.Decoder` (decoder/basic.py:10-86) on this
package's model and Kaldi writer.

`decode(decode_dir, output_dir)` reads `trials` (utt, target speaker(s)),
`feats.scp` and optionally `spk2spk_id`, converts every trial with
`model.infer((feat (1, mel, T), target (1, 1)))` and writes the converted
(T, mel) features to `output_dir/feats.{ark,scp}` as Kaldi compressed matrices
(compression_method=1, as the reference, :52-53).  Unlike the reference
(:31-37) there is no silent CPU retry: the model runs on the MI355X through
libvqx or raises.

`decode_batch_size: N` (default 1: the loop above, unchanged) converts up to N
trials per call as one padded batch, `model.infer((x, y), lengths=...)`.
Trials are read `N * WINDOW_BATCHES` at a time in trial order; inside such a
window they are sorted by length and cut into batches of N neighbours, so an
utterance is padded only to the longest of its N neighbours and at most one
window of features is held on the host.  A source utterance listed with
several targets is read once and fills several slots.  The window is written
out in trial order, so `feats.ark` / `feats.scp` keep the order of `trials`.
`decoder.hier` shares all of this and differs in its model call alone.
"""
import inspect
import logging
from importlib import import_module
from pathlib import Path

import numpy as np
import torch

from ..dataset.kaldi_io import WriteHelper, load_mat

logger = logging.getLogger()

WINDOW_BATCHES = 8  # batches formed from one window of trials


def length_batches(lengths, N):
    """The positions 0..len(lengths)-1 of one window sorted by length (stable:
    ties keep their order) and cut into batches of N neighbours."""
    order = sorted(range(len(lengths)), key=lambda k: lengths[k])
    return [order[k0:k0 + N] for k0 in range(0, len(order), N)]


class Decoder(object):
    batch_method = "infer"  # the model method decode_batch_step calls (checked for `lengths` at construction)

    def __init__(self, config):
        n = config.get("decode_batch_size", 1)  # checked first: a bad value builds no model
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"decode_batch_size must be a positive integer, got {n!r}")
        model_type = config.get("model_type", "vae_npvc_amd.model.vqvae:Model").split(":")
        if not config.get("use_gpu", True):
            raise RuntimeError("vae_npvc_amd decodes on the MI355X only (use_gpu: false is not supported)")
        self.device = torch.device("cuda")
        module = import_module(model_type[0], package=None)
        model_name = "Model" if len(model_type) < 2 else model_type[1]
        cls = getattr(module, model_name)
        if n > 1 and "lengths" not in inspect.signature(getattr(cls, self.batch_method)).parameters:
            raise NotImplementedError(f"decode_batch_size {n}: {cls.__module__}.{model_name}.{self.batch_method} takes "
                                      "no `lengths` (no batches of different lengths for this model)")
        self.model = cls(config).to(self.device)
        self.model.eval()
        self.decode_batch_size = n

    def decode_step(self, feat, spk):
        with torch.no_grad():
            return self.model.infer((feat, spk))

    def decode_batch_step(self, x, y, lens):
        """x (B, mel, max(lens)) padded with zeros, y (B, 1), lens host ints -> (B, mel, max(lens))."""
        with torch.no_grad():
            return self.model.infer((x, y), lengths=lens)

    def decode_batch(self, feats, targets):
        """feats: (T_b, mel) host arrays, targets: speaker ids -> the converted (T_b, mel) arrays."""
        lens = [f.shape[0] for f in feats]
        x = np.zeros((len(feats), feats[0].shape[1], max(lens)), dtype=np.float32)
        for b, f in enumerate(feats):
            x[b, :, :lens[b]] = f.T
        y = torch.tensor(targets).long().view(-1, 1).to(self.device)
        out = self.decode_batch_step(torch.from_numpy(x).to(self.device), y, lens).cpu().numpy()
        return [np.ascontiguousarray(out[b, :, :n].T) for b, n in enumerate(lens)]

    def decode_batched(self, decode_dir, output_dir, compress=True):
        """`decode` for decode_batch_size > 1."""
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
                done = [None] * len(window)
                for pick in length_batches([f.shape[0] for f in feats], N):
                    logger.info(f"Decode {[w0 + k for k in pick]}: {[window[k][0] for k in pick]} to "
                                f"{[window[k][1] for k in pick]}")
                    for k, f in zip(pick, self.decode_batch([feats[k] for k in pick], [targets[k] for k in pick])):
                        done[k] = f
                for (utt, _), f in zip(window, done):
                    wf[utt] = f

    def decode(self, decode_dir, output_dir, compress=True):
        if self.decode_batch_size > 1:
            return self.decode_batched(decode_dir, output_dir, compress=compress)
        decode_dir = Path(decode_dir)
        output_dir = str(output_dir)
        for file in ["trials", "feats.scp"]:
            if not (decode_dir / file).is_file():
                raise FileNotFoundError(f"No such file {decode_dir / file}")
        trials = [line.strip().split(None, 1) for line in open(decode_dir / "trials") if line.strip()]
        feats_scp = dict(line.strip().split(None, 1) for line in open(decode_dir / "feats.scp") if line.strip())
        spk2spk_id = None
        if (decode_dir / "spk2spk_id").exists():
            spk2spk_id = dict(line.strip().split(None, 1) for line in open(decode_dir / "spk2spk_id") if line.strip())
        wspecifier = "ark,scp:{0}/feats.ark,{0}/feats.scp".format(output_dir)
        with WriteHelper(wspecifier, compression_method=1 if compress else None) as wf:
            for i, (utt, target) in enumerate(trials):
                logger.info(f"Decode {i}: {utt} to {target}")
                feat = torch.from_numpy(np.array(load_mat(feats_scp[utt]))).float().to(self.device)
                feat = feat.t().unsqueeze(0)
                if spk2spk_id:
                    target = [int(spk2spk_id[t]) for t in target.split()]
                else:
                    target = [int(t) for t in target.split()]
                if len(target) != 1:
                    raise ValueError(f"trial {utt}: one target speaker per utterance, got {target}")
                target = torch.tensor(target).long().to(self.device).view(1, -1)
                feat_decode = self.decode_step(feat, target)
                wf[utt] = feat_decode[0].t().detach().cpu().numpy()

    def get_model_info(self):
        return self.model

    def load_checkpoint(self, checkpoint_file):
        checkpoint_data = torch.load(checkpoint_file, map_location="cpu", weights_only=True)
        self.model.load_state_dict(checkpoint_data["model"])
        return checkpoint_data["iteration"]
