"""Fixtures of the hierarchical model's batched conversion of utterances of
different lengths: tests/golden/vqragged_<case> (.npz + .json each), cases
`gst` and `plain_top` of make_golden_vqvae2_model.py's small architecture.

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2_ragged.py --reference DIR [--only NAME]

One seeded parameter set and four utterances of 130, 70, 64 and 97 frames, in
that order (the longest is not last; 64 and 130 -> 32 leave exact groups, 70
and 97 partial ones), each with a target speaker of its own.  The reference
converts them one at a time: `xhat` of `forward((x_b, y'_b))` at B = 1.  The
level lengths are 32 / 17 / 16 / 24 at level 1 and 2 / 1 / 1 / 1 at level 2
(the strided convs floor), so the stretch factors of `upsample` differ per
utterance.

Stored: the seeded state_dict before any forward (the codebooks spread on the
first utterance and normalised as in make_golden_vqvae2_model.py), and per
utterance b: `x.b`, the source speaker `y` (the spreading ran with y[0]), the
target speakers `y_tgt`, the float64 `xhat.b`, the indices `idx.b.k` of every
quantized level in the order the levels run (top first), `err32[b]` (the
float32 run's distance from the float64 run) and the smallest top-2 gap over
both runs.  The seed is advanced until every gap is >= 1e-3 in both precisions
and both runs pick the same indices for every utterance.
"""
import argparse
import os

import torch

from make_golden_vqvae2_infer import run_forward
from make_golden_vqvae2_model import (MAX_SEEDS, MIN_GAP, MODEL_CASES, load_reference, model_arch, rel, save,
                                      spread_codebooks)

LENGTHS = [130, 70, 64, 97]
LEVEL_LENGTHS = [[130, 70, 64, 97], [32, 17, 16, 24], [2, 1, 1, 1]]  # [level][utterance]
SEEDS = {n: 9900 + 10 * i for i, n in enumerate(MODEL_CASES)}


def make_ragged(ref, name):
    arch = model_arch(MODEL_CASES[name])
    mel, n_spk, U = arch["encoder.0"]["in_channels"][0], arch["y_num"], len(LENGTHS)
    seed = SEEDS[name]
    while True:
        torch.manual_seed(seed)
        m = ref.Model(arch)
        xs = [torch.randn(1, mel, T) for T in LENGTHS]
        y = torch.randint(0, n_spk, (U, 1))
        y_tgt = (y + 1 + torch.randint(0, n_spk - 1, (U, 1))) % n_spk  # never y itself
        spread_codebooks(m, xs[0], y[:1], torch.Generator().manual_seed(seed))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m64 = ref.Model(arch)
        torch.nn.Module.load_state_dict(m64, sd)  # the class's own override reads an attribute it never sets
        m64.double()
        runs, ok = [], True
        for b, x in enumerate(xs):
            xh32, ids32, gaps32 = run_forward(m, x, y_tgt[b:b + 1])
            n_q = len(ids32)
            assert [idx.shape[1] for idx in ids32] == [LEVEL_LENGTHS[i][b] for i in reversed(range(n_q))], b
            xh64, ids64, gaps64 = run_forward(m64, x.double(), y_tgt[b:b + 1])
            ok = min(gaps32 + gaps64) >= MIN_GAP and all(torch.equal(p, q) for p, q in zip(ids32, ids64))
            if not ok:
                break
            runs.append((xh32, xh64, ids64, gaps32, gaps64))
        # the level every utterance has many frames of must use more than one code somewhere
        if ok and any(r[2][-1].unique().numel() > 1 for r in runs):
            break
        seed += 1
        if seed - SEEDS[name] >= MAX_SEEDS:
            raise RuntimeError(f"vqragged_{name}: no seed in {MAX_SEEDS} gives gaps >= {MIN_GAP} for every utterance")
    arrays = {"y": y.numpy(), "y_tgt": y_tgt.numpy()}
    err32, gaps = [], []
    for b, (xh32, xh64, ids64, gaps32, gaps64) in enumerate(runs):
        arrays[f"x.{b}"] = xs[b][0].numpy()
        arrays[f"xhat.{b}"] = xh64[0].numpy()
        for k, idx in enumerate(ids64):
            arrays[f"idx.{b}.{k}"] = idx[0].numpy()
        err32.append(rel(xh32, xh64))
        gaps.append(min(gaps32 + gaps64))
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
    save("vqragged", name, arrays,
         {"seed": seed, "lengths": LENGTHS, "level_lengths": LEVEL_LENGTHS, "arch": arch,
          "err32": {f"xhat.{b}": e for b, e in enumerate(err32)}, "keys": list(sd.keys()), "gap": min(gaps),
          "gaps": gaps})


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
            make_ragged(ref, name)
