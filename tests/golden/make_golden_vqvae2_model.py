"""Fixtures of the hierarchical model: tests/golden/vqenc_<case>,
vqlevel_<case> and vqmodel_<case> (.npz + .json each).

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2_model.py --reference DIR [--only NAME]

vqenc    the reference's `vqvae2.Encoder`: (z, feat) = encoder(x) and one
         backward from gradients into z and feat (either may be absent).
vqlevel  the reference's `VectorQuantizer.forward` ('frame_mean'): z_vq, both
         losses, the perplexity, the indices, and the gradients of
         sum(z_vq * go) + w_qut * z_qut_loss + w_enc * z_enc_loss.
vqmodel  the reference's `vqvae2.Model`: forward((x, y)) and loss.backward().

Each runs once in float32 and once in float64 (a fresh module with the same
state_dict, `.double()`).  The float64 run is the expected result; the float32
run's distance from it per tensor (`err32 = max|f32 - f64| / max|f64|`) is the
reference's own rounding, from which the GPU tests derive their bound.  The
stored parameters are the seeded state_dict before the forward; a normalised
codebook is renormalised in place by every forward (embed_norm()), and its
gradient is taken at the renormalised value.

Quantizer inputs must not sit near a tie: the smallest gap between the two
nearest codes' distances over all frames is recorded (`gap`), in the float64
and the float32 run alike, and the seed is advanced until it is >= 1e-3 (the
project's near-tie threshold is 1e-4), so an fp32 run must reproduce every index.
"""
import argparse
import importlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
MIN_GAP = 1e-3

# ---------------------------------------------------------------- encoder
# case: B, T, encoder arguments (widths 16 / 32), gradient into z, gradient into feat
_ENC = dict(kernel_size=3, z_channels=16, stack_kernel_size=3, use_causal_conv=False)
ENC_CASES = {
    "s1": (2, 20, dict(in_channels=[16], out_channels=[32], downsample_scales=[1], stacks=[2], stack_layers=2,
                       dilation=True, use_weight_norm=True), True, True),
    "down2x2": (2, 24, dict(in_channels=[16, 32], out_channels=[32, 32], downsample_scales=[2, 2], stacks=[1, 1],
                            stack_layers=1, dilation=False, use_weight_norm=True), True, False),
    # a single output frame per utterance: utterances far shorter than a GEMM row tile
    "down4x4_T1": (3, 16, dict(in_channels=[16, 32], out_channels=[32, 32], downsample_scales=[4, 4], stacks=[1, 1],
                               stack_layers=1, dilation=False, use_weight_norm=True), True, True),
    "nown": (2, 24, dict(in_channels=[16, 32], out_channels=[32, 32], downsample_scales=[2, 2], stacks=[1, 1],
                         stack_layers=2, dilation=True, use_weight_norm=False), False, True),
}
# ---------------------------------------------------------------- quantizer level
# case: K, D, B, T, normalize
LEVEL_CASES = {
    "k16_norm": (16, 64, 2, 5, True),
    "k16_plain": (16, 64, 2, 5, False),
    "k512_norm": (512, 128, 2, 64, True),  # the recipe's quantizer
}
LEVEL_WEIGHTS = (1.0, 0.25)  # w_qut, w_enc
# ---------------------------------------------------------------- model
MODEL_CASES = {"gst": True, "plain_top": False}  # use_gst
ZERO_GRAD = "mha.linear_k.bias"
SEEDS = {n: 9500 + 10 * i for i, n in enumerate([*ENC_CASES, *LEVEL_CASES, *MODEL_CASES])}


def model_arch(use_gst):
    """levels 3, level lengths T / T/4 / T/64 (64 / 16 / 1 for T = 64), 16-32 channel convs, K = 16."""
    top = 32 if use_gst else 64  # channels of the top level's quantized output
    enc = dict(kernel_size=3, z_channels=64, dilation=False, stack_kernel_size=3, stack_layers=1,
               use_weight_norm=True, use_causal_conv=False)
    dec = dict(out_channels=[32], skip_channels=16, kernel_size=3, upsample_scales=[1], dilation=False,
               stack_kernel_size=3, stacks=[2], use_weight_norm=True, use_causal_conv=False)
    vq = dict(z_num=16, z_dim=64, normalize=True)
    arch = {"levels": 3, "use_gst": use_gst, "use_ema": False, "beta": 0.01, "y_num": 4, "y_dim": 16, "jitter_p": 0.0,
            "encoder.0": dict(enc, in_channels=[24], out_channels=[32], downsample_scales=[1], stacks=[1]),
            "encoder.1": dict(enc, in_channels=[32, 32], out_channels=[32, 32], downsample_scales=[2, 2], stacks=[1, 1]),
            "encoder.2": dict(enc, in_channels=[32, 32], out_channels=[32, 32], downsample_scales=[4, 4], stacks=[1, 1]),
            "quantizer.0": dict(vq), "quantizer.1": dict(vq),
            "quantizer.2": dict(ref_embed_dim=64, gst_tokens=6, gst_token_dim=32, gst_heads=2) if use_gst else dict(vq),
            "decoder.0": dict(dec, in_channels=[top + 128], cond_channels=16, final_channels=24),
            "decoder.1": dict(dec, in_channels=[64], cond_channels=top + 64, final_channels=64),
            "decoder.2": dict(dec, in_channels=[64], cond_channels=top, final_channels=64)}
    return arch


def load_reference(root):
    sys.path.insert(0, str(Path(root)))
    return (importlib.import_module("vae_npvc.model.vqvae2"), importlib.import_module("vae_npvc.model.layers_vq"))


def rel(a32, a64):
    a32, a64 = torch.as_tensor(a32).double(), torch.as_tensor(a64).double()
    return float((a32 - a64).abs().max() / a64.abs().max().clamp_min(1e-300))


def save(kind, name, arrays, meta):
    """One .npz per case, or several (<name>.npz, <name>.1.npz, ...) so that each stays below the 1 MiB file limit."""
    parts, size = [{}], 0
    for k, v in arrays.items():
        assert v.nbytes < 900_000, (kind, name, k, v.nbytes)
        if size + v.nbytes >= 900_000:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    files = [f"{kind}_{name}.npz" if i == 0 else f"{kind}_{name}.{i}.npz" for i in range(len(parts))]
    for f, part in zip(files, parts):
        np.savez_compressed(HERE / f, **part)
    meta = dict(meta, case=name, files=files)
    with open(HERE / f"{kind}_{name}.json", "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    err = meta["err32"].values()
    print(f"{kind}_{name}: err32 {min(err):.2e}..{max(err):.2e}  "
          + ", ".join(f"{f} {(HERE / f).stat().st_size} bytes" for f in files)
          + (f"  gap {meta['gap']}" if "gap" in meta else ""))


def top2_gap(z, emb, normalize):
    """Smallest difference between the two nearest codes' distances (layers_vq.py:103-105) over the frames of z (B, D, T)."""
    zf = z.detach().transpose(1, 2).reshape(-1, z.shape[1])
    emb = emb.detach()
    if normalize:
        zf = zf / zf.norm(dim=1, keepdim=True)
        emb = emb / emb.norm(dim=1, keepdim=True)
    d = zf.pow(2).sum(1, keepdim=True) + emb.pow(2).sum(1) - 2 * zf @ emb.t()
    t = d.topk(2, dim=1, largest=False).values
    return float((t[:, 1] - t[:, 0]).min())


# ---------------------------------------------------------------- encoder
def run_encoder(enc, x, dz, dfeat):
    x = x.clone().requires_grad_()
    z, feat = enc(x)
    outs = [(z, dz), (feat, dfeat)]
    torch.autograd.backward([o for o, g in outs if g is not None], [g for _, g in outs if g is not None])
    grads = {k: p.grad.detach() for k, p in enc.named_parameters() if p.grad is not None}
    return z.detach(), feat.detach(), x.grad.detach(), grads


def make_encoder(ref, name):
    B, T, args, with_dz, with_dfeat = ENC_CASES[name]
    args = dict(_ENC, **args)
    torch.manual_seed(SEEDS[name])
    enc = ref.Encoder(**args)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    Tz = T // int(np.prod(args["downsample_scales"]))
    x = torch.randn(B, args["in_channels"][0], T)
    dz = torch.randn(B, args["z_channels"], Tz) if with_dz else None
    dfeat = torch.randn(B, args["out_channels"][-1], Tz) if with_dfeat else None
    z32, f32, dx32, g32 = run_encoder(enc, x, dz, dfeat)
    enc64 = ref.Encoder(**args)
    enc64.load_state_dict(sd)
    enc64.double()
    d = lambda t: None if t is None else t.double()  # noqa: E731
    z64, f64, dx64, g64 = run_encoder(enc64, x.double(), d(dz), d(dfeat))
    arrays = {"x": x.numpy(), "z": z64.numpy(), "feat": f64.numpy(), "dx": dx64.numpy()}
    if with_dz:
        arrays["dz"] = dz.numpy()
    if with_dfeat:
        arrays["dfeat"] = dfeat.numpy()
    err32 = {"z": rel(z32, z64), "feat": rel(f32, f64), "dx": rel(dx32, dx64)}
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
    for k in g64:
        arrays["grad." + k] = g64[k].numpy()
        err32[k] = rel(g32[k], g64[k])
    save("vqenc", name, arrays,
         {"seed": SEEDS[name], "B": B, "T": T, "Tz": Tz, "encoder": args, "err32": err32, "keys": list(sd.keys()),
          "params": [k for k, _ in enc.named_parameters()], "grads": list(g64.keys())})


# ---------------------------------------------------------------- quantizer level
def run_level(q, z, go):
    z = z.clone().requires_grad_()
    z_vq, qut, enc, detail = q(z)
    (z_vq * go).sum().add(LEVEL_WEIGHTS[0] * qut + LEVEL_WEIGHTS[1] * enc).backward()
    with torch.no_grad():
        idx = q.encode(z)
    return {"z_vq": z_vq.detach(), "z_qut_loss": qut.detach(), "z_enc_loss": enc.detach(),
            "entropy": torch.tensor(detail["entropy"], dtype=z.dtype), "dz": z.grad.detach(),
            "dE": q.embeddings.grad.detach()}, idx, top2_gap(z, q.embeddings, q.normalize)


def make_level(vq_mod, name):
    K, D, B, T, normalize = LEVEL_CASES[name]
    seed = SEEDS[name]
    while True:
        torch.manual_seed(seed)
        q = vq_mod.VectorQuantizer(K, D, normalize=normalize, reduction="frame_mean")
        E0 = q.embeddings.detach().clone()
        z, go = torch.randn(B, D, T), torch.randn(B, D, T)
        r32, idx32, gap32 = run_level(q, z, go)
        q64 = vq_mod.VectorQuantizer(K, D, normalize=normalize, reduction="frame_mean")
        q64.load_state_dict({"embeddings": E0})
        q64.double()
        r64, idx64, gap64 = run_level(q64, z.double(), go.double())
        if min(gap32, gap64) >= MIN_GAP and torch.equal(idx32, idx64):
            break
        seed += 1
    arrays = {"z": z.numpy(), "go": go.numpy(), "param.embeddings": E0.numpy(), "idx": idx64.numpy()}
    arrays.update({k: v.numpy() for k, v in r64.items()})
    save("vqlevel", name, arrays,
         {"seed": seed, "K": K, "D": D, "B": B, "T": T, "normalize": normalize, "loss_weights": list(LEVEL_WEIGHTS),
          "gap": min(gap32, gap64), "gap32": gap32, "gap64": gap64, "err32": {k: rel(r32[k], r64[k]) for k in r64}})


# ---------------------------------------------------------------- model
def run_model(ref, model, x, y):
    gaps, hooks = [], []
    for q in model.quantizers:
        if hasattr(q, "embeddings"):
            hooks.append(q.register_forward_hook(
                lambda m, inp, out: gaps.append(top2_gap(inp[0], m.embeddings, m.normalize))))
    ids = []
    for q in model.quantizers:
        if hasattr(q, "embeddings"):
            hooks.append(q.register_forward_hook(lambda m, inp, out: ids.append(m.encode(inp[0].detach()))))
    xhat, loss, detail = model((x, y))
    for h in hooks:
        h.remove()
    loss.backward()
    grads = {k: p.grad.detach() for k, p in model.named_parameters()}
    return xhat.detach(), detail, grads, ids, gaps


SPREAD_ROWS = 2   # codebook rows taken from the quantizer's own input frames
MAX_SEEDS = 400


def spread_codebooks(model, x, y, gen):
    """A random codebook leaves every frame of these small models on one code
    (perplexity 1, one non-zero row of dE).  In the order the levels run, the
    first SPREAD_ROWS rows of each codebook become evenly spaced frames of that
    quantizer's own input with 5 % noise; the other rows keep their random
    values.  The biases of the convs that feed a quantizer (z_proj, the lower
    decoders' last conv) are zeroed first: they are the part every frame shares,
    and with them the frames' distances differ by less than the gap the
    fixtures require.  (More rows from the frames leave the gaps below it too.)"""
    order = [i for i in reversed(range(model.levels)) if hasattr(model.quantizers[i], "embeddings")]
    with torch.no_grad():
        for i in range(model.levels):
            model.encoders[i].z_proj.bias.zero_()
            if i > 0:
                model.decoders[i].final_layer[3].bias.zero_()
        for i in order:
            q, cap = model.quantizers[i], []
            h = q.register_forward_hook(lambda m, inp, out: cap.append(inp[0].detach()))
            model((x, y))
            h.remove()
            z = cap[0].transpose(1, 2).reshape(-1, q.z_dim)
            n = min(SPREAD_ROWS, z.shape[0])
            rows = z[torch.linspace(0, z.shape[0] - 1, n).round().long()]
            rows = rows + 0.05 * rows.norm(dim=1, keepdim=True) / q.z_dim ** 0.5 * torch.randn(rows.shape, generator=gen)
            q.embeddings[:n] = rows
            q.embed_norm()


def make_model(ref, name):
    use_gst = MODEL_CASES[name]
    arch = model_arch(use_gst)
    B, T = 2, 64
    seed = SEEDS[name]
    while True:
        torch.manual_seed(seed)
        m = ref.Model(arch)
        x = torch.randn(B, arch["encoder.0"]["in_channels"][0], T)
        y = torch.randint(0, arch["y_num"], (B, 1))
        spread_codebooks(m, x, y, torch.Generator().manual_seed(seed))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        xh32, d32, g32, ids32, gaps32 = run_model(ref, m, x, y)
        # every level with more than one frame must use more than one code
        varied = all(idx.unique().numel() > 1 for idx in ids32 if idx.numel() > x.shape[0])
        if min(gaps32) >= MIN_GAP and varied:
            m64 = ref.Model(arch)
            torch.nn.Module.load_state_dict(m64, sd)  # the class's own override reads an attribute it never sets
            m64.double()
            xh64, d64, g64, ids64, gaps64 = run_model(ref, m64, x.double(), y)
            if min(gaps64) >= MIN_GAP and all(torch.equal(a, b) for a, b in zip(ids32, ids64)):
                break
        seed += 1
        if seed - SEEDS[name] >= MAX_SEEDS:
            raise RuntimeError(f"vqmodel_{name}: no seed in {MAX_SEEDS} gives varied indices with gaps >= {MIN_GAP}")
    arrays = {"x": x.numpy(), "y": y.numpy(), "xhat": xh64.numpy()}
    err32 = {"xhat": rel(xh32, xh64)}
    for k, v in d64.items():
        arrays["loss." + k] = np.float64(v)
        err32[k] = rel(d32[k], v)
    for k, idx in enumerate(ids64):
        arrays[f"idx.{k}"] = idx.numpy()
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
    abs32 = {}
    for k in g64:
        arrays["grad." + k] = g64[k].numpy()
        if k.endswith(ZERO_GRAD):
            # mathematically zero (the softmax ignores a per-head constant); the float64 run leaves its own
            # rounding residue, so the float32 run's largest absolute value is recorded instead
            assert float(g64[k].abs().max()) <= 1e-12 * float(g64[k[:-4] + "weight"].abs().max())
            abs32[k] = float(g32[k].abs().max())
        else:
            err32[k] = rel(g32[k], g64[k])
    save("vqmodel", name, arrays,
         {"seed": seed, "abs32": abs32, "B": B, "T": T, "arch": arch, "err32": err32, "keys": list(sd.keys()),
          "params": [k for k, _ in m.named_parameters()], "loss_keys": list(d64.keys()),
          "gap": min(gaps32 + gaps64), "gaps32": gaps32, "gaps64": gaps64})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE, as make_golden.py)")
    ap.add_argument("--only", default=None, choices=sorted([*ENC_CASES, *LEVEL_CASES, *MODEL_CASES]))
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    ref, vq_mod = load_reference(a.reference)
    for name in ENC_CASES:
        if a.only in (None, name):
            make_encoder(ref, name)
    for name in LEVEL_CASES:
        if a.only in (None, name):
            make_level(vq_mod, name)
    for name in MODEL_CASES:
        if a.only in (None, name):
            make_model(ref, name)
