"""Fixtures of the self-attention layer: tests/golden/attn_<case>.{npz,json}.

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_attn.py --reference DIR [--only CASE]

For each case it seeds torch, builds the reference's MultiHeadedAttention(F, F,
F, H, F) (loaded by path from <reference>/vae_npvc/model/layers_gst.py; its
masked branch names `numpy` without importing it, so the loaded module gets
`module.numpy = numpy`), and runs `out = mha(xt, xt, xt, mask)` and
`out.backward(go)` with xt = x^T
  * in float64 (a fresh module with the same state_dict, `.double()`): the
    expected result;
  * in float32: `err32 = max|f32 - f64| / max|f64|` per tensor is the
    reference's own rounding, from which the fp32 GPU test derives its bound;
  * in float32 under torch.autocast("cpu", dtype=torch.bfloat16): `l2_bf16`
    per tensor is the relative L2 distance of torch's own bf16 run from
    float64, the yardstick of the bf16 GPU test.
`linear_k.bias` has an exactly zero gradient (the softmax ignores a
per-query constant), so for it the largest absolute values are recorded
instead (`abs32`, `abs_bf16`).  The same holds for every gradient whose
float64 value is identically zero (T = 1: the softmax over one key is the
constant 1, so nothing flows into q and k); those are listed in `zero_ref`,
with err32 = l2_bf16 = 0.

With lengths: mask[b, 0, t2] = t2 < len[b], `go` is zero at t >= len[b], and
`out` is compared (and stored) on the frames t < len[b] only: its tail is
stored as zeros, which is what the layer under test writes there.  The
reference's masked branch cannot run under bf16 autocast (it asks numpy for the
limits of a bfloat16 tensor), so the autocast sample of a case with lengths
runs every utterance alone on its own frames without a mask, which is the same
function, and adds the parameter gradients up.

x, go, out and dx are stored as (B, F, T), the layout of SelfAttention.
"""
import argparse
import importlib.util
import json
import os
import re
from pathlib import Path

import numpy
import numpy as np
import torch

HERE = Path(__file__).resolve().parent

# case: B, F, H, T, lengths, input scale
CASES = {
    "one_tile": (2, 128, 4, 64, None, 1.0),       # d_k 32, a single key tile
    "single_frame": (2, 64, 2, 1, None, 1.0),     # softmax over one key
    "odd_T": (2, 128, 2, 77, None, 1.0),          # d_k 64, partial query and key tiles
    "multi_tile": (1, 128, 4, 320, None, 1.0),    # several key tiles, the online rescale
    "peaked": (2, 128, 4, 200, None, 6.0),        # one weight near 1; the row maximum moves between tiles
    "ragged": (4, 128, 4, 130, [130, 70, 64, 1], 1.0),  # the project's ragged lengths, a one-frame utterance
    "ragged64": (3, 64, 2, 200, [200, 137, 5], 1.0),    # F 64, masks inside a later tile
    "recipe_T": (2, 128, 4, 256, None, 1.0),      # the training crop length
}
SEEDS = {name: 9300 + i for i, name in enumerate(CASES)}
KB = "linear_k.bias"


def load_reference(root):
    path = Path(root) / "vae_npvc" / "model" / "layers_gst.py"
    spec = importlib.util.spec_from_file_location("reference_layers_gst", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.numpy = numpy  # the masked branch's `numpy.finfo`
    return mod


def key_mask(lengths, T):
    if lengths is None:
        return None
    return (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).unsqueeze(1)  # (B, 1, T)


def run(mha, x, go, lengths):
    """(out, dx, {key: grad}, attention weights) with x, go, out, dx as (B, F, T)."""
    mha.zero_grad(set_to_none=True)
    xt = x.transpose(1, 2).clone().requires_grad_()
    out = mha(xt, xt, xt, key_mask(lengths, x.shape[2]))
    out.backward(go.transpose(1, 2))
    grads = {k: p.grad.detach().clone() for k, p in mha.named_parameters()}
    return out.detach().transpose(1, 2), xt.grad.detach().transpose(1, 2), grads, mha.attn.detach()


def run_autocast(mha, x, go, lengths):
    """run() under bf16 autocast; with lengths, utterance by utterance without a mask (module docstring)."""
    mha.zero_grad(set_to_none=True)
    B, F, T = x.shape
    out, dx = torch.zeros(B, F, T), torch.zeros(B, F, T)
    for b in range(B) if lengths is not None else [slice(None)]:
        n = lengths[b] if lengths is not None else T
        sel = slice(b, b + 1) if lengths is not None else b
        xt = x[sel, :, :n].transpose(1, 2).clone().requires_grad_()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            o = mha(xt, xt, xt, None)
        o.float().backward(go[sel, :, :n].transpose(1, 2))
        out[sel, :, :n] = o.detach().float().transpose(1, 2)
        dx[sel, :, :n] = xt.grad.detach().transpose(1, 2)
    return out, dx, {k: p.grad.detach().clone() for k, p in mha.named_parameters()}


def valid(t, lengths):
    """(B, F, T) with the frames t >= len[b] zeroed."""
    if lengths is None:
        return t
    t = t.clone()
    for b, n in enumerate(lengths):
        t[b, :, n:] = 0
    return t


def rel(a, a64):
    return float((a.double() - a64).abs().max() / a64.abs().max())


def l2(a, a64):
    return float((a.double() - a64).norm() / a64.norm())


def make(ref, name):
    B, F, H, T, lengths, scale = CASES[name]
    torch.manual_seed(SEEDS[name])
    mha = ref.MultiHeadedAttention(F, F, F, H, F)
    x = torch.randn(B, F, T) * scale
    go = valid(torch.randn(B, F, T), lengths)
    sd = {k: v.detach().clone() for k, v in mha.state_dict().items()}
    out32, dx32, g32, _ = run(mha, x, go, lengths)
    outbf, dxbf, gbf = run_autocast(mha, x, go, lengths)
    mha64 = ref.MultiHeadedAttention(F, F, F, H, F)
    mha64.load_state_dict(sd)
    mha64.double()
    out64, dx64, g64, attn = run(mha64, x.double(), go.double(), lengths)
    out32, outbf, out64 = (valid(t, lengths) for t in (out32, outbf, out64))
    if lengths is not None:  # nothing flows into or out of a padded frame
        for b, n in enumerate(lengths):
            assert not dx64[b, :, n:].any() and not attn[b, :, :, n:].any()

    attn_max = float(attn.max())
    later = float((attn.argmax(-1) >= 128).double().mean()) if T > 128 else 0.0
    if name == "peaked":
        assert attn_max > 0.9, attn_max
        assert later >= 0.25, later  # the running maximum moves in a later key tile for these rows

    arrays = {"x": x.numpy(), "go": go.numpy(), "out": out64.numpy(), "dx": dx64.contiguous().numpy()}
    err32 = {"out": rel(out32, out64), "dx": rel(dx32, dx64)}
    l2_bf16 = {"out": l2(outbf, out64), "dx": l2(dxbf, dx64)}
    abs32, abs_bf16, zero_ref = {}, {}, []
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
        arrays["grad." + k] = g64[k].numpy()
        if k == KB:
            # mathematically zero; the float64 run leaves its own rounding residue
            assert float(g64[k].abs().max()) <= 1e-12 * float(g64["linear_k.weight"].abs().max())
            abs32[k], abs_bf16[k] = float(g32[k].abs().max()), float(gbf[k].abs().max())
        elif not g64[k].any():
            zero_ref.append(k)
            abs32[k], abs_bf16[k] = float(g32[k].abs().max()), float(gbf[k].abs().max())
            err32[k] = l2_bf16[k] = 0.0
        else:
            err32[k], l2_bf16[k] = rel(g32[k], g64[k]), l2(gbf[k], g64[k])
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    files = write_parts(name, arrays)
    meta = {"case": name, "seed": SEEDS[name], "B": B, "F": F, "H": H, "T": T, "lengths": lengths, "scale": scale,
            "attn_max": attn_max, "argmax_from_128": later, "err32": err32, "l2_bf16": l2_bf16, "abs32": abs32,
            "abs_bf16": abs_bf16, "zero_ref": zero_ref, "keys": list(sd.keys()), "files": files}
    with open(HERE / f"attn_{name}.json", "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(f"attn_{name}: attn_max {attn_max:.4f} later {later:.3f}  err32 {min(err32.values()):.2e}.."
          f"{max(err32.values()):.2e}  l2_bf16 {min(l2_bf16.values()):.2e}..{max(l2_bf16.values()):.2e}  "
          f"abs32 {abs32} abs_bf16 {abs_bf16}  {[(HERE / p).stat().st_size for p in files]} bytes")


PART_BYTES = 900_000  # raw array bytes per .npz: a committed file stays below 1 MiB


def write_parts(name, arrays, prefix="attn"):
    """<prefix>_<name>.npz, and <prefix>_<name>.<i>.npz for what does not fit
    the first (float64 gradients are incompressible); the .json lists them."""
    parts, size = [{}], 0
    for k, v in arrays.items():
        if size and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    files = []
    for old in HERE.glob(f"{prefix}_{name}*.npz"):
        if re.fullmatch(rf"{re.escape(prefix)}_{re.escape(name)}(\.\d+)?\.npz", old.name):  # not a longer case name
            old.unlink()
    for i, part in enumerate(parts):
        files.append(f"{prefix}_{name}.npz" if i == 0 else f"{prefix}_{name}.{i}.npz")
        np.savez_compressed(HERE / files[-1], **part)
        assert (HERE / files[-1]).stat().st_size < 1 << 20, files[-1]
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
