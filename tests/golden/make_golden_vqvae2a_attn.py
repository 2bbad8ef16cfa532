"""Fixtures of vqvae2a.Model with `attention.{i}`: tests/golden/vq2a_attn_<case>
(training steps, as make_golden_vqvae2a.py's vq2a_<case>) and
vq2a_attn_ragged_<case> (four utterances converted alone in eval mode, as
make_golden_vqvae2ab_ragged.py's vq2a_ragged_<case>), .npz + .json each.

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2a_attn.py --reference DIR [--only CASE]

The reference has no such key.  The model under reference here is the
reference's own `vqvae2a.Model` of make_golden_vqvae2a.model_arch(case) whose
level-i encoder is wrapped: it calls the reference encoder and returns
(z + mha(z^T, z^T, z^T, None)^T, feat) with a reference `MultiHeadedAttention`
(F = the encoder's z_channels).  The wrapper replaces the encoder's `forward`
on the instance, so the encoder keeps its module tree and keys, and the
attention modules hang on the model as `attentions.{i}.mha`, registered last:
the state_dict has this package's key names in this package's order.  The
reference's own `forward` and `encode` then run unchanged, and so do the two
generators this one imports: it hands them a stand-in for the reference module
whose `Model(arch)` builds the wrapped model, and a `save` that writes under
the new names and adds the `attention.{i}` keys to the stored arch.

Attention settings: `ema_gst` levels 0, 1, 2 with n_head 2, 1, 2 (d_k 32 and
64; level 2's attention runs before the style pool), `single_ema` level 0 with
n_head 2.  Every utterance and the training batch run at their full length, so
the mask is None throughout.  Seeds are advanced by the imported generators'
own rules: every top-2 distance gap >= 1e-3, identical indices in float32 and
float64.
"""
import argparse
import importlib
import os
import sys
from pathlib import Path

import torch
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden_vqvae2_model as base  # noqa: E402
import make_golden_vqvae2a as steps_gen  # noqa: E402
import make_golden_vqvae2ab_ragged as ragged_gen  # noqa: E402
from make_golden_attn import load_reference as load_mha  # noqa: E402

HEADS = {"ema_gst": {0: 2, 1: 1, 2: 2}, "single_ema": {0: 2}}


class Holder(nn.Module):
    """`attentions.{i}`: the key prefix `mha.` of SelfAttention."""

    def __init__(self, mha):
        super().__init__()
        self.mha = mha


def wrap(enc, mha):
    """enc(x) -> (z + mha(z^T, z^T, z^T, None)^T, feat)."""
    inner = enc.forward

    def forward(x):
        z, feat = inner(x)
        zt = z.transpose(1, 2)
        return z + mha(zt, zt, zt, None).transpose(1, 2), feat
    enc.forward = forward


class Wrapped:
    """Stands in for the reference's vqvae2a module: Model(arch) is its Model with the case's attentions."""

    def __init__(self, ref, gst, heads):
        self.ref, self.gst, self.heads = ref, gst, heads

    def Model(self, arch):
        m = self.ref.Model(arch)
        att = {}
        for i, h in self.heads.items():
            f = arch[f"encoder.{i}"]["z_channels"]
            att[str(i)] = Holder(self.gst.MultiHeadedAttention(f, f, f, h, f))
        m.attentions = nn.ModuleDict(att)  # after every module of the reference's: the existing order stays
        for i in self.heads:
            wrap(m.encoders[i], m.attentions[str(i)].mha)
        return m


def saver(heads):
    def save(kind, name, arrays, meta):
        arch = dict(meta["arch"], **{f"attention.{i}": {"n_head": h} for i, h in heads.items()})
        assert [k for k in meta["keys"] if k.startswith("attentions.")] == \
            [f"attentions.{i}.mha.linear_{n}.{p}" for i in heads for n in ("q", "k", "v", "out") for p in ("weight", "bias")]
        assert not any(k.startswith("attentions.") for k in meta["keys"][:-8 * len(heads)])
        base.save(kind.replace("vq2a", "vq2a_attn"), name, arrays, dict(meta, arch=arch))
        for f in Path(base.HERE).glob(f"{kind.replace('vq2a', 'vq2a_attn')}_{name}*"):
            assert f.stat().st_size < 1 << 20, f
    return save


def make(ref, gst, name):
    stand_in = Wrapped(ref, gst, HEADS[name])
    steps_gen.save = ragged_gen.save = saver(HEADS[name])
    try:
        steps_gen.make_model(stand_in, name)
        ragged_gen.make_ragged(stand_in, "vq2a", name)
    finally:
        steps_gen.save = ragged_gen.save = base.save


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE, as make_golden.py)")
    ap.add_argument("--only", default=None, choices=sorted(HEADS))
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    gst = load_mha(a.reference)
    sys.path.insert(0, str(Path(a.reference)))
    ref = importlib.import_module("vae_npvc.model.vqvae2a")
    for name in HEADS:
        if a.only in (None, name):
            make(ref, gst, name)
