"""Fixtures of the hierarchical model's conversion: tests/golden/vqinfer_<case>
(.npz + .json each), cases `gst` and `plain_top` of make_golden_vqvae2_model.py's
small architecture at B = 1, T = 70.

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2_infer.py --reference DIR [--only NAME]

The reference's `forward` defines conversion: `xhat` of `forward((x, y'))` is x
rendered with speaker y'.  T = 70 is no multiple of the model's down-sampling:
the level lengths are 70, 17 and 1 (the strided convs floor: 70 -> 35 -> 17 and
17 -> 4 -> 1), and the level of 17 frames is stretched to 70 by repetition by 4
with a replicate-padded tail of 2.

Stored: the seeded state_dict before the forward (the codebooks spread and
normalised as in make_golden_vqvae2_model.py), x, the source speaker y (which
the codebook spreading ran with), a different target speaker y', the float64
xhat of forward((x, y')), the indices of every quantized level in the order
the levels run (top first), `err32` (the float32 run's distance from the
float64 run) and `gap` (the smallest top-2 distance gap over both runs).  The
seed is advanced until the gap is >= 1e-3 in both precisions and both runs
pick the same indices.
"""
import argparse
import os

import torch

from make_golden_vqvae2_model import (MAX_SEEDS, MIN_GAP, MODEL_CASES, load_reference, model_arch, rel, save,
                                      spread_codebooks, top2_gap)

B, T = 1, 70
LEVEL_LENGTHS = [70, 17, 1]
SEEDS = {n: 9700 + 10 * i for i, n in enumerate(MODEL_CASES)}


def run_forward(model, x, y):
    """xhat of forward((x, y)), the indices of the quantized levels in running order and their top-2 gaps."""
    gaps, ids, hooks = [], [], []
    for q in model.quantizers:
        if hasattr(q, "embeddings"):
            hooks.append(q.register_forward_hook(
                lambda m, inp, out: gaps.append(top2_gap(inp[0], m.embeddings, m.normalize))))
            hooks.append(q.register_forward_hook(lambda m, inp, out: ids.append(m.encode(inp[0].detach()))))
    with torch.no_grad():
        xhat = model((x, y))[0]
    for h in hooks:
        h.remove()
    return xhat.detach(), ids, gaps


def make_infer(ref, name):
    arch = model_arch(MODEL_CASES[name])
    seed = SEEDS[name]
    while True:
        torch.manual_seed(seed)
        m = ref.Model(arch)
        x = torch.randn(B, arch["encoder.0"]["in_channels"][0], T)
        y = torch.randint(0, arch["y_num"], (B, 1))
        y_tgt = (y + 1 + torch.randint(0, arch["y_num"] - 1, (B, 1))) % arch["y_num"]  # never y itself
        spread_codebooks(m, x, y, torch.Generator().manual_seed(seed))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        xh32, ids32, gaps32 = run_forward(m, x, y_tgt)
        lengths = sorted((idx.shape[1] for idx in ids32), reverse=True)
        assert lengths == LEVEL_LENGTHS[:len(lengths)], lengths
        varied = all(idx.unique().numel() > 1 for idx in ids32 if idx.numel() > B)
        if min(gaps32) >= MIN_GAP and varied:
            m64 = ref.Model(arch)
            torch.nn.Module.load_state_dict(m64, sd)  # the class's own override reads an attribute it never sets
            m64.double()
            xh64, ids64, gaps64 = run_forward(m64, x.double(), y_tgt)
            if min(gaps64) >= MIN_GAP and all(torch.equal(a, b) for a, b in zip(ids32, ids64)):
                break
        seed += 1
        if seed - SEEDS[name] >= MAX_SEEDS:
            raise RuntimeError(f"vqinfer_{name}: no seed in {MAX_SEEDS} gives varied indices with gaps >= {MIN_GAP}")
    assert not torch.equal(y, y_tgt)
    arrays = {"x": x.numpy(), "y": y.numpy(), "y_tgt": y_tgt.numpy(), "xhat": xh64.numpy()}
    for k, idx in enumerate(ids64):
        arrays[f"idx.{k}"] = idx.numpy()
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
    save("vqinfer", name, arrays,
         {"seed": seed, "B": B, "T": T, "level_lengths": LEVEL_LENGTHS, "arch": arch, "err32": {"xhat": rel(xh32, xh64)},
          "keys": list(sd.keys()), "gap": min(gaps32 + gaps64), "gaps32": gaps32, "gaps64": gaps64})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE, as make_golden.py)")
    ap.add_argument("--only", default=None, choices=sorted(MODEL_CASES))
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    ref, _ = load_reference(a.reference)
    for name in MODEL_CASES:
        if a.only in (None, name):
            make_infer(ref, name)
