"""Fixtures of the style-token (GST) layer: tests/golden/gst_<case>.{npz,json}.

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_gst.py --reference DIR [--only CASE]

For each case it seeds torch, builds the reference's StyleTokenLayer (loaded
by path from <reference>/vae_npvc/model/layers_gst.py), and runs
`layer(z.mean(-1))` and `.backward(go)` once in float32 and once in float64
(a fresh layer with the same state_dict, `.double()`).  The float64 run is
the expected result; the float32 run's distance from it, per tensor
(`err32 = max|f32 - f64| / max|f64|`), is the reference's own rounding, from
which the GPU test derives its bound.  `mha.linear_k.bias` has an exactly zero
gradient (the softmax ignores a per-head constant), so for it the float32
run's largest absolute value is recorded instead (`abs32`).
"""
import argparse
import importlib.util
import json
import os
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent

# case: B, R, N, F, H, T, input scale
CASES = {
    "vae2": (3, 128, 10, 128, 4, 4, 1.0),        # the recipe's quantizer.2; T = 256 / 64
    "default": (2, 128, 10, 256, 4, 1, 1.0),     # constructor defaults, d_k = 64, no pooling
    "odd": (5, 64, 7, 96, 3, 3, 1.0),            # non-power-of-two N, F, H, T
    "batch96": (96, 128, 10, 128, 4, 4, 1.0),    # the recipe batch: batch-reduction order, grid > 64
    "saturated": (3, 128, 10, 128, 4, 4, 50.0),  # softmax with one weight ~ 1
}
SEEDS = {name: 9100 + i for i, name in enumerate(CASES)}


def load_reference(root):
    path = Path(root) / "vae_npvc" / "model" / "layers_gst.py"
    spec = importlib.util.spec_from_file_location("reference_layers_gst", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(layer, z, go):
    z = z.clone().requires_grad_()
    out = layer(z.mean(-1))
    out.backward(go)
    grads = {k: p.grad.detach() for k, p in layer.named_parameters()}
    return out.detach(), z.grad.detach(), grads, float(layer.mha.attn.detach().max())


def rel(a32, a64):
    return float((a32.double() - a64).abs().max() / a64.abs().max())


def make(ref, name):
    B, R, N, F, H, T, scale = CASES[name]
    torch.manual_seed(SEEDS[name])
    layer = ref.StyleTokenLayer(ref_embed_dim=R, gst_tokens=N, gst_token_dim=F, gst_heads=H)
    z = torch.randn(B, R, T) * scale
    go = torch.randn(B, F)
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    out32, dz32, g32, attn_max = run(layer, z, go)
    layer64 = ref.StyleTokenLayer(ref_embed_dim=R, gst_tokens=N, gst_token_dim=F, gst_heads=H)
    layer64.load_state_dict(sd)
    layer64.double()
    out64, dz64, g64, _ = run(layer64, z.double(), go.double())

    arrays = {"z": z.numpy(), "go": go.numpy(), "out": out64.numpy(), "dz": dz64.numpy()}
    err32 = {"out": rel(out32, out64), "dz": rel(dz32, dz64)}
    abs32 = {}
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
        arrays["grad." + k] = g64[k].numpy()
        if k == "mha.linear_k.bias":
            # mathematically zero; the float64 run leaves its own rounding residue
            assert float(g64[k].abs().max()) <= 1e-12 * float(g64["mha.linear_k.weight"].abs().max())
            abs32[k] = float(g32[k].abs().max())
        else:
            err32[k] = rel(g32[k], g64[k])
    files = write_parts(name, arrays)
    meta = {"case": name, "seed": SEEDS[name], "B": B, "R": R, "N": N, "F": F, "H": H, "T": T, "scale": scale,
            "attn_max": attn_max, "err32": err32, "abs32": abs32, "keys": list(sd.keys()), "files": files}
    with open(HERE / f"gst_{name}.json", "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(f"gst_{name}: attn_max {attn_max:.4f}  err32 {min(err32.values()):.2e}..{max(err32.values()):.2e}  "
          f"abs32 {abs32}  {[(HERE / p).stat().st_size for p in files]} bytes")


PART_BYTES = 900_000  # raw array bytes per .npz: a committed file stays below 1 MiB


def write_parts(name, arrays):
    """gst_<name>.npz, and gst_<name>.<i>.npz for what does not fit the first
    (float64 weight gradients are incompressible); the .json lists them."""
    parts, size = [{}], 0
    for k, v in arrays.items():
        if size and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    files = []
    for old in HERE.glob(f"gst_{name}*.npz"):
        old.unlink()
    for i, part in enumerate(parts):
        files.append(f"gst_{name}.npz" if i == 0 else f"gst_{name}.{i}.npz")
        np.savez_compressed(HERE / files[-1], **part)
    return files


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
