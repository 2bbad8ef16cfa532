"""Shared set-up of the flat model's ragged-batch tests (tests/test_gpu_flat_ragged.py):
seeded weights, codebook and utterances of different lengths, and the CPU
oracle's answer for every utterance ALONE (oracle.vqvae_cpu.OracleVQVAE in eval
mode), computed once per case and never modified.

A case is a config of tests/helpers.cfg_of, or "vcc20_plain" (vcc20 with the
straight-through quantizer, the settings of the step_vcc20_plain fixture).
Weights come from seeded_state_dict(cfg, WSEED); the EMA codebook (N(0, 1) * 0.3)
and the features (N(0, 1)) from one PCG64(SEED[case]) stream, in that order, as
tests/test_gpu_inference.py::_setup draws them.

SEED[case] is the first seed from 3 up, found on the CPU with
helpers.oracle_encode_gaps, at which every valid frame's top-2 relative
distance gap in the oracle is at least NEAR_TIE = 1e-4: the tests assert that,
and may then demand exact indices.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests.helpers import cfg_of, oracle_encode_gaps

WSEED = 91
LENGTHS = {"vcc20": [130, 70, 64, 97, 1, 33], "aishell3": [130, 70, 64, 97, 1, 33],
           "vcc20_plain": [130, 70, 64, 97, 1, 33], "vcc20_multi": [128, 68, 64, 96, 4, 32]}
SEED = {"vcc20": 3, "aishell3": 4, "vcc20_plain": 3, "vcc20_multi": 12}  # min gaps 1.8e-4, 1.9e-4, 1.2e-4, 2.7e-4


def config(case, compute_dtype="fp32"):
    if case == "vcc20_plain":
        return cfg_of("vcc20", use_ema=False, compute_dtype=compute_dtype)
    return cfg_of(case, compute_dtype=compute_dtype)


def draw(case, seed):
    """(cfg, state dict, [x_b (mel, T_b) f32], y (B, 1) int64) of a case for a data seed."""
    from oracle.vqvae_cpu import seeded_state_dict
    cfg = config(case)
    sd = seeded_state_dict(cfg, WSEED)
    rng = np.random.Generator(np.random.PCG64(seed))
    if cfg.get("use_ema", False):
        sd["quantizer.emb_init"] = torch.tensor(True)
        sd["quantizer.embeddings"] = torch.from_numpy(
            (rng.standard_normal((cfg.get("z_num", 512), cfg.get("z_dim", 128))) * 0.3).astype(np.float32))
    mel = cfg["encoder"]["in_channels"][0]
    xs = [torch.from_numpy(rng.standard_normal((n, mel)).astype(np.float32).T.copy()) for n in LENGTHS[case]]
    y = torch.tensor([[(i * 37) % cfg.get("y_num", 10)] for i in range(len(xs))])
    return cfg, sd, xs, y


def oracle_alone(cfg, sd, xs, y):
    """Per utterance alone: (ids int64 (T_z,), top-2 gaps (T_z,), xhat f32 (mel, T)) of the eval-mode oracle."""
    from oracle.vqvae_cpu import OracleVQVAE
    orc = OracleVQVAE(cfg, sd)
    orc.training = False
    out = []
    with torch.no_grad():
        for b, x in enumerate(xs):
            ids, gap = oracle_encode_gaps(orc, x.unsqueeze(0))
            ids = torch.from_numpy(ids.astype(np.int64))
            out.append((ids, gap, orc.decode(ids.view(1, -1), y[b:b + 1])[0].clone()))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """The shared, read-only set-up and oracle reference of a case."""
    cfg, sd, xs, y = draw(name, SEED[name])
    ref = oracle_alone(cfg, sd, xs, y)
    S = int(np.prod(cfg["encoder"].get("downsample_scales", [1])))
    return SimpleNamespace(name=name, cfg=cfg, sd=sd, xs=xs, y=y, lens=list(LENGTHS[name]), S=S,
                           ids=[r[0] for r in ref], gaps=[r[1] for r in ref], xhat=[r[2] for r in ref])


def padded(c, T=None, fill=0.0, order=None):
    """The utterances `order` (default all) of case c as one (B, mel, T) batch, `fill` from each end up."""
    order = list(range(len(c.xs))) if order is None else list(order)
    lens = [c.lens[b] for b in order]
    x = torch.full((len(order), c.xs[0].shape[0], T or max(lens)), float(fill))
    for k, b in enumerate(order):
        x[k, :, :lens[k]] = c.xs[b]
    return x, lens


def model(c, compute_dtype="fp32"):
    from vae_npvc_amd.model.vqvae import Model
    m = Model(dict(c.cfg, compute_dtype=compute_dtype))
    m.load_state_dict(c.sd)
    return m.cuda().eval()


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())
