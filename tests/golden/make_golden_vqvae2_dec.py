"""Fixtures of the hierarchical decoder: tests/golden/vqdec_<case>.{npz,json}
and the `upsample` index maps tests/golden/vqdec_index_maps.json.

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2_dec.py --reference DIR [--only CASE]

For each case it seeds torch, builds the reference's `vqvae2.Decoder` (module
vae_npvc.model.vqvae2 of the checkout), and runs
`decoder((x, cat([upsample(l, T) for l in levels])))` and `.backward(go)` once
in float32 and once in float64 (a fresh decoder with the same state_dict,
`.double()`); the `tensor` case passes a plain random `c` instead of levels.
The float64 run is the expected result; the float32 run's distance from it,
per tensor (`err32 = max|f32 - f64| / max|f64|`), is the reference's own
rounding, from which the GPU test derives its bound.

The index maps are the reference's `Model.upsample` applied to arange(T_l):
the source frame of every output frame, for each (T, T_l) pair in PAIRS.
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

# every case: kernel_size 3, stack_kernel_size 3, one stage, stacks [2], Cin = C = 32,
# cond 24 = levels of 8 and 16 channels, skip 16, final 16
# case: B, T, level lengths (None: a plain tensor c), dilation
CASES = {
    "tail": (2, 20, (1, 3), False),      # replicate-pad tail; utterances shorter than a 128-frame tile
    "dilated": (3, 24, (1, 6), True),    # dilated conv_in
    "fallback": (2, 20, (3, 8), False),  # two-step stretch differs from the direct one: full-rate conditioning
    "tensor": (2, 20, None, False),      # the reference's call: c (B, 24, T)
}
SEEDS = {name: 9200 + i for i, name in enumerate(CASES)}
LEVEL_CH = (8, 16)
PAIRS = ((20, 3), (256, 64), (256, 1), (7, 7), (9, 2), (128, 3), (20, 8), (256, 5))


def decoder_args(dilation):
    return dict(in_channels=[32], out_channels=[32], upsample_scales=[1], cond_channels=sum(LEVEL_CH),
                skip_channels=16, final_channels=16, kernel_size=3, dilation=dilation, stack_kernel_size=3,
                stacks=[2], use_weight_norm=True, use_causal_conv=False)


def load_reference(root):
    sys.path.insert(0, str(Path(root)))
    return importlib.import_module("vae_npvc.model.vqvae2")


def run(ref, dec, x, cond, go):
    """cond: a list of levels or a tensor c.  -> out, dx, [d cond...], {key: grad}"""
    x = x.clone().requires_grad_()
    if isinstance(cond, list):
        cond = [z.clone().requires_grad_() for z in cond]
        c = torch.cat([ref.Model.upsample(None, z, x.shape[-1]) for z in cond], dim=1)
        leaves = cond
    else:
        c = cond.clone().requires_grad_()
        leaves = [c]
    out = dec((x, c))
    out.backward(go)
    grads = {k: p.grad.detach() for k, p in dec.named_parameters()}
    return out.detach(), x.grad.detach(), [z.grad.detach() for z in leaves], grads


def rel(a32, a64):
    return float((a32.double() - a64).abs().max() / a64.abs().max())


def make(ref, name):
    B, T, lens, dilation = CASES[name]
    args = decoder_args(dilation)
    torch.manual_seed(SEEDS[name])
    dec = ref.Decoder(**args)
    x = torch.randn(B, 32, T)
    cond = [torch.randn(B, C, Tl) for C, Tl in zip(LEVEL_CH, lens)] if lens else torch.randn(B, sum(LEVEL_CH), T)
    go = torch.randn(B, 16, T)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    out32, dx32, dc32, g32 = run(ref, dec, x, cond, go)
    dec64 = ref.Decoder(**args)
    dec64.load_state_dict(sd)
    dec64.double()
    cond64 = [z.double() for z in cond] if lens else cond.double()
    out64, dx64, dc64, g64 = run(ref, dec64, x.double(), cond64, go.double())

    arrays = {"x": x.numpy(), "go": go.numpy(), "out": out64.numpy(), "dx": dx64.numpy()}
    err32 = {"out": rel(out32, out64), "dx": rel(dx32, dx64)}
    names = [f"level.{i}" for i in range(len(lens))] if lens else ["c"]
    for n, z, d32, d64 in zip(names, cond if lens else [cond], dc32, dc64):
        arrays[n] = z.numpy()
        arrays["d" + n] = d64.numpy()
        err32["d" + n] = rel(d32, d64)
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
        arrays["grad." + k] = g64[k].numpy()
        err32[k] = rel(g32[k], g64[k])
    raw = sum(v.nbytes for v in arrays.values())
    assert raw < 900_000, raw  # one .npz per case stays below the 1 MiB file limit
    np.savez_compressed(HERE / f"vqdec_{name}.npz", **arrays)
    meta = {"case": name, "seed": SEEDS[name], "B": B, "T": T, "levels": list(lens) if lens else None,
            "level_channels": list(LEVEL_CH), "decoder": args, "err32": err32, "keys": list(sd.keys()),
            "params": [k for k, _ in dec.named_parameters()], "files": [f"vqdec_{name}.npz"]}
    with open(HERE / f"vqdec_{name}.json", "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(f"vqdec_{name}: err32 {min(err32.values()):.2e}..{max(err32.values()):.2e}  raw {raw} bytes, "
          f"{(HERE / f'vqdec_{name}.npz').stat().st_size} on disk")


def index_maps(ref):
    maps = []
    for T, Tl in PAIRS:
        z = torch.arange(Tl, dtype=torch.float32).view(1, 1, Tl)
        up = ref.Model.upsample(None, z, T)
        assert up.shape == (1, 1, T)
        maps.append({"T": T, "T_l": Tl, "src": [int(v) for v in up.view(-1).tolist()]})
    with open(HERE / "vqdec_index_maps.json", "w") as f:
        json.dump({"pairs": maps}, f)
        f.write("\n")
    print(f"vqdec_index_maps: {len(maps)} pairs")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE, as make_golden.py)")
    ap.add_argument("--only", default=None, choices=sorted(CASES))
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    ref = load_reference(a.reference)
    for name in CASES:
        if a.only in (None, name):
            make(ref, name)
    if a.only is None:
        index_maps(ref)
