"""Fixtures of the vqvae2b model: tests/golden/vq2b_<case> (.npz + .json each).

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2b.py --reference DIR [--only NAME]

vq2b   the reference's `vqvae2b.Model`: per step forward((x, y)) and
       loss.backward() (no optimizer), then in eval mode encode(x) and
       infer((x, ys)) with ys (B, levels) naming a different speaker per level.

As make_golden_vqvae2a.py, whose helpers this script imports: a float32 run
and a float64 twin from the same state_dict, consuming the generators alike,
the float64 run stored and `err32 = max|f32 - f64| / max|f64|` recorded per
tensor; the seed is advanced until every codebook lookup has a top-2 distance
gap >= 1e-3 in both runs and at every step, and both runs pick identical
indices (MAX_SEEDS tries).

One lookup cannot meet an absolute 1e-3: the mean-pooled top level of
`pooled_ema` hands its EMA codebook B = 2 frames for K = 16 codes, so the
codebook is `_tile`'s noisy copies of those frames at init and after every
update (a row is kept only while a frame picks it), and the two nearest codes
of a frame are copies of itself |noise|^2 ~ 1e-4 from it, whatever the seed.
As for `vqema_tile_k64` (make_golden_vqvae2a.py), such a lookup (N < K) is
held to the same gap in proportion to the distance's largest term,
gap >= 1e-3 / 128 * max(|z|^2 + |e|^2), and that level's z_proj (weight_g and
bias) is scaled by 0.01 in the state_dict so that the noise is large against
the frames, as that case scales its input.
"""
import argparse
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden_vqvae2_model import MAX_SEEDS, MIN_GAP, rel, save, top2_gap  # noqa: E402
from make_golden_vqvae2a import (JITTER_P, ZERO_GRAD, buffers_of, f32_noise, lookup, model_arch as arch_2a,  # noqa: E402
                                 reseed)

MODEL_CASES = ("ema_gst", "plain_last", "pooled_ema")
SEEDS = {n: 9900 + 10 * i for i, n in enumerate(MODEL_CASES)}
TOP_SCALE = 0.01  # pooled_ema: the top level's z_proj


def model_arch(case):
    """vq2a's dimensions (B 2, T 64, 24 mel, 16-32 channel convs, K 16, z_dim 64, y_num 4, y_dim 16); every level
    decoder reads its own level alone and writes 32 channels, final_decoder reads their stack without conditioning."""
    a = arch_2a("ema_gst")
    enc0, enc1, dec = a["encoder.0"], a["encoder.1"], dict(a["decoder.0"], final_channels=32)
    enc = {k: v for k, v in enc1.items() if k != "downsample_scales"}
    base = {"beta": 0.01, "y_num": 4, "y_dim": 16}
    ema = dict(z_num=16, z_dim=64, mu=0.9)
    plain = dict(z_num=16, z_dim=64, normalize=True)

    def final(levels):
        return dict(dec, in_channels=[32 * levels], final_channels=24, cond_channels=0)
    if case == "ema_gst":  # level lengths 64 / 16 / 1 (the style level is pooled)
        return dict(base, levels=3, use_gst=True, use_ema=True, jitter_p=JITTER_P, upsample_last=False, **{
            "encoder.0": enc0, "encoder.1": enc1, "encoder.2": dict(enc, downsample_scales=[4, 4]),
            "quantizer.0": dict(ema), "quantizer.1": dict(ema), "quantizer.2": a["quantizer.2"],
            "decoder.0": dict(dec, in_channels=[64]), "decoder.1": dict(dec, in_channels=[64]),
            "decoder.2": dict(dec, in_channels=[32]), "final_decoder": final(3)})
    if case == "plain_last":  # level lengths 64 / 16 / 4: the jittered top level needs more than one frame
        return dict(base, levels=3, use_gst=False, use_ema=False, jitter_p=JITTER_P, pooling_last=False,
                    upsample_last=True, **{
            "encoder.0": enc0, "encoder.1": enc1, "encoder.2": dict(enc, downsample_scales=[2, 2]),
            "quantizer.0": dict(plain), "quantizer.1": dict(plain), "quantizer.2": dict(plain),
            "decoder.0": dict(dec, in_channels=[64]), "decoder.1": dict(dec, in_channels=[64]),
            "decoder.2": dict(dec, in_channels=[64]), "final_decoder": final(3)})
    if case == "pooled_ema":  # level lengths 64 / 1: a decoder on one frame, stretched x64 afterwards
        return dict(base, levels=2, use_gst=False, use_ema=True, jitter_p=0.0, pooling_last=True, upsample_last=True, **{
            "encoder.0": enc0, "encoder.1": enc1, "quantizer.0": dict(ema), "quantizer.1": dict(ema),
            "decoder.0": dict(dec, in_channels=[64]), "decoder.1": dict(dec, in_channels=[64]),
            "final_decoder": final(2)})
    raise KeyError(case)


def load_reference(root):
    sys.path.insert(0, str(Path(root)))
    return importlib.import_module("vae_npvc.model.vqvae2b")


def codebooks(model):
    return [q for q in model.quantizers if hasattr(q, "embeddings")]


def watch(model, log):
    """Every codebook lookup of a training forward, in the order they run: (indices (B, T), gap, largest term of the
    distance, frames < codes).  An EMA level is caught in update_emb, where `embeddings` still is the codebook the
    lookup used; a plain level by a forward hook."""
    hooks = []
    for q in codebooks(model):
        if hasattr(q, "update_emb"):
            orig = q.update_emb

            def update_emb(z, z_idx, q=q, orig=orig):
                idx, gap, scale = lookup(z, q.embeddings)
                assert torch.equal(idx, z_idx)
                q._seen = (idx.clone(), gap, scale, z.shape[0] < q.z_num)
                return orig(z, z_idx)
            q.update_emb = update_emb
            hooks.append(q.register_forward_hook(
                lambda m, inp, out: log.append((m._seen[0].view(inp[0].shape[0], -1), *m._seen[1:]))))
        else:
            hooks.append(q.register_forward_hook(
                lambda m, inp, out: log.append((m.encode(inp[0].detach()), top2_gap(inp[0], m.embeddings, m.normalize),
                                                2.0, False))))
    return hooks


def enough(look):
    """The gap rule of the docstring over lookups (idx, gap, scale, tiled)."""
    return all(gap >= (MIN_GAP / 128 * scale if tiled else MIN_GAP) for _, gap, scale, tiled in look)


def spread_levels(model, x, y, gen):
    """plain_last: a random codebook leaves every frame of a level on one code.  Two rows of every level's codebook
    become evenly spaced frames of that level's quantizer input with 5 % noise (the inputs are the encoders' outputs,
    which do not depend on the codebooks); the z_proj biases, the part every frame shares, are zeroed first."""
    cap = {}
    with torch.no_grad():
        for enc in model.encoders:
            enc.z_proj.bias.zero_()
        hooks = [q.register_forward_hook(lambda m, inp, out, i=i: cap.__setitem__(i, inp[0].detach()))
                 for i, q in enumerate(model.quantizers)]
        model.eval()
        model((x, y))
        model.train()
        for h in hooks:
            h.remove()
        for i, q in enumerate(model.quantizers):
            zf = cap[i].transpose(1, 2).reshape(-1, q.z_dim)
            rows = zf[torch.linspace(0, zf.shape[0] - 1, 2).round().long()]
            rows = rows + 0.05 * rows.norm(dim=1, keepdim=True) / q.z_dim ** 0.5 * torch.randn(rows.shape, generator=gen)
            q.embeddings[:2] = rows
            q.embed_norm()


def run_model(model, x, y, ys, steps, run_seed, double):
    log, out = [], []
    hooks = watch(model, log)
    model.train()
    reseed(run_seed)
    with f32_noise(double):
        for _ in range(steps):
            model.zero_grad(set_to_none=True)
            xhat, loss, detail = model((x, y))
            loss.backward()
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
            out.append(dict(xhat=xhat.detach(), detail=dict(detail), grads=grads, lookups=list(log),
                            buffers=buffers_of(model)))
            log.clear()
        for h in hooks:
            h.remove()
        model.eval()
        with torch.no_grad():
            codes = [c.detach().clone() for c in model.encode(x)]
            look, feat = [], x
            for i in range(model.levels):  # the gaps of encode's lookups, against the codebooks as they are now
                z, feat = model.encoders[i](feat)
                q = model.quantizers[i]
                if model.pooling_last and i == model.levels - 1:
                    z = z.mean(dim=-1, keepdim=True)
                if hasattr(q, "update_emb"):
                    zf = z.transpose(1, 2).reshape(-1, q.z_dim)
                    look.append((codes[i], *lookup(zf, q.embeddings)[1:], zf.shape[0] < q.z_num))
                elif hasattr(q, "embeddings"):
                    look.append((codes[i], top2_gap(z, q.embeddings, q.normalize), 2.0, False))
            infer = model.infer((x, ys)).detach().clone()
    model.train()
    return out, codes, look, infer


def make_model(ref, name):
    arch = model_arch(name)
    steps = 1 if name == "plain_last" else 2
    B, T = 2, 64
    for seed in range(SEEDS[name], SEEDS[name] + MAX_SEEDS):
        torch.manual_seed(seed)
        m = ref.Model(arch)
        x = torch.randn(B, arch["encoder.0"]["in_channels"][0], T)
        y = torch.randint(0, arch["y_num"], (B, 1))
        ys = (y + 1 + torch.arange(arch["levels"])) % arch["y_num"]  # a different speaker per level, none of them y
        if name == "plain_last":
            spread_levels(m, x, y, torch.Generator().manual_seed(seed))
        if name == "pooled_ema":
            with torch.no_grad():
                m.encoders[1].z_proj.weight_g.mul_(TOP_SCALE)
                m.encoders[1].z_proj.bias.mul_(TOP_SCALE)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        o32, c32, el32, inf32 = run_model(m, x, y, ys, steps, seed, False)
        look32 = [l for s in o32 for l in s["lookups"]]
        varied = all(l[0].unique().numel() > 1 for l in look32 if l[0].numel() > B)
        if not varied or not enough(look32 + el32):
            continue
        m64 = ref.Model(arch)
        torch.nn.Module.load_state_dict(m64, sd)
        m64.double()
        o64, c64, el64, inf64 = run_model(m64, x.double(), y, ys, steps, seed, True)
        look64 = [l for s in o64 for l in s["lookups"]]
        same = all(torch.equal(a[0], b[0]) for a, b in zip(look32, look64)) and \
            all(torch.equal(a, b) for a, b in zip(c32, c64) if not a.is_floating_point())
        if same and enough(look64 + el64):
            break
    else:
        raise RuntimeError(f"vq2b_{name}: no seed in {MAX_SEEDS} gives varied indices with the required gaps")
    arrays = {"x": x.numpy(), "y": y.numpy(), "ys": ys.numpy()}
    err32, abs32 = {}, {}
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
    for n, (s32, s64) in enumerate(zip(o32, o64), 1):
        p = f"s{n}."
        arrays[p + "xhat"] = s64["xhat"].numpy()
        err32[p + "xhat"] = rel(s32["xhat"], s64["xhat"])
        for k, v in s64["detail"].items():
            arrays[p + "loss." + k] = np.float64(v)
            err32[p + "loss." + k] = rel(s32["detail"][k], v)
        for j, l in enumerate(s64["lookups"]):
            arrays[p + f"idx.{j}"] = l[0].numpy()
        for k, v in s64["buffers"].items():
            arrays[p + "buf." + k] = v.numpy()
            if v.is_floating_point():
                err32[p + "buf." + k] = rel(s32["buffers"][k], v)
        for k, g in s64["grads"].items():
            arrays[p + "grad." + k] = g.numpy()
            if k.endswith(ZERO_GRAD):  # mathematically zero: the float32 run's largest absolute value instead
                assert float(g.abs().max()) <= 1e-12 * float(s64["grads"][k[:-4] + "weight"].abs().max())
                abs32[p + "grad." + k] = float(s32["grads"][k].abs().max())
            else:
                err32[p + "grad." + k] = rel(s32["grads"][k], g)
    for i, c in enumerate(c64):
        arrays[f"enc.{i}"] = c.numpy()
        if c.is_floating_point():
            err32[f"enc.{i}"] = rel(c32[i], c)
    arrays["infer"] = inf64.numpy()
    err32["infer"] = rel(inf32, inf64)
    every = look32 + look64 + el32 + el64
    save("vq2b", name, arrays,
         {"seed": seed, "run_seed": seed, "steps": steps, "B": B, "T": T, "arch": arch, "err32": err32, "abs32": abs32,
          "keys": list(sd.keys()), "params": [k for k, _ in m.named_parameters()],
          "grads": list(o64[0]["grads"].keys()), "buffers": list(o64[0]["buffers"].keys()),
          "loss_keys": [list(s["detail"].keys()) for s in o64], "lookups": [len(s["lookups"]) for s in o64],
          "level_lengths": [int(c.shape[-1]) for c in c64],
          "gap": min(l[1] for l in every if not l[3]),
          "tiled_gap_ratio": min([l[1] / (MIN_GAP / 128 * l[2]) for l in every if l[3]], default=None),
          "gaps32": [l[1] for l in look32], "gaps64": [l[1] for l in look64],
          "encode_gaps": [l[1] for l in el32 + el64]})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE, as make_golden.py)")
    ap.add_argument("--only", default=None, choices=sorted(MODEL_CASES))
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    ref = load_reference(a.reference)
    for name in MODEL_CASES:
        if a.only in (None, name):
            make_model(ref, name)
