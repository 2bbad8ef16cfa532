"""Fixtures of vqvae2a's and vqvae2b's batched conversion of utterances of
different lengths: tests/golden/vq2a_ragged_<case> and vq2b_ragged_<case>
(.npz + .json each), with the cases and small architectures of
make_golden_vqvae2a.py (`ema_gst`, `plain_shared`, `single_ema`) and
make_golden_vqvae2b.py (`ema_gst`, `plain_last`, `pooled_ema`).

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2ab_ragged.py --reference DIR [--only KIND_NAME]

One seeded parameter set and four utterances of 130, 70, 64 and 97 frames, in
that order (make_golden_vqvae2_ragged.py), each with a target speaker of its
own; vqvae2b also gets a `ys` row naming a different speaker per level.  The
reference converts them one at a time in eval mode at B = 1: `xhat.b` is the
xhat of `forward((x_b, y'_b))`, and for vqvae2b `xinf.b` is
`infer((x_b, ys_b))`.  Each runs in float32 and in a float64 twin from the same
state_dict; the float64 outputs are stored with
`err32 = max|f32 - f64| / max|f64|` per output.

The stored state_dict is the one the eval runs start from.  Every codebook is
spread as spread_codebooks / spread_levels do: the z_proj biases are zeroed,
and two rows per level become evenly spaced frames of that level's quantizer
input for the first utterance with 5 % noise (one row where the level has one
frame).  An EMA codebook, which is all zeros before its first training forward,
starts from random rows, gets the two frames, and is marked initialised
(emb_init true, emb_sum = embeddings, emb_elem 1): no training forward runs, so
`_tile`'s near-duplicate rows never enter.

Stored per utterance b: `x.b`, `xhat.b` (and `xinf.b`), the indices `idx.b.k`
of every codebook lookup of forward in run order (bottom level first; infer's
lookups must pick the same), a style top's float64 embedding `style.b`, and in
the json `err32`, the level lengths (a mean-pooled or style top has 1) and the
smallest top-2 gap over both runs and both precisions.  The seed is advanced
until every lookup's gap is >= 1e-3 in both precisions, both precisions pick
identical indices, and some level with several frames uses more than one code.
Should the mean-pooled EMA top of `pooled_ema` fail that absolute rule for
every seed, that one lookup is held to the proportional rule of
make_golden_vqvae2b.py, gap >= 1e-3 / 128 * max(|z|^2 + |e|^2); the json's
`top_rule` says which rule applied.
"""
import argparse
import importlib
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden_vqvae2_model import MAX_SEEDS, MIN_GAP, rel, save  # noqa: E402
from make_golden_vqvae2a import MODEL_CASES as CASES_2A, model_arch as arch_2a  # noqa: E402
from make_golden_vqvae2b import MODEL_CASES as CASES_2B, model_arch as arch_2b  # noqa: E402

LENGTHS = [130, 70, 64, 97]
KINDS = {"vq2a": (CASES_2A, arch_2a, "vae_npvc.model.vqvae2a"), "vq2b": (CASES_2B, arch_2b, "vae_npvc.model.vqvae2b")}
SEEDS = {f"{kind}_{n}": 10100 + 100 * k + 10 * i for k, kind in enumerate(KINDS) for i, n in enumerate(KINDS[kind][0])}


def codebooks(model):
    """The codebook modules, once each (vqvae2a may share one)."""
    mods = list(model.quantizers) if getattr(model, "use_quantizers", True) else [model.quantizer]
    return [q for q in mods if hasattr(q, "embeddings")]


def nearest(z, q):
    """(indices (B, T), smallest top-2 gap, max(|z|^2 + |e|^2)) of z (B, D, T) against q's codebook."""
    zf, emb = z.detach().transpose(1, 2).reshape(-1, z.shape[1]), q.embeddings.detach()
    if getattr(q, "normalize", False):
        zf, emb = zf / zf.norm(dim=1, keepdim=True), emb / emb.norm(dim=1, keepdim=True)
    d = zf.pow(2).sum(1, keepdim=True) + emb.pow(2).sum(1) - 2 * zf @ emb.t()
    t = d.topk(2, dim=1, largest=False).values
    return (d.argmin(1).view(z.shape[0], -1), float((t[:, 1] - t[:, 0]).min()),
            float(zf.pow(2).sum(1).max() + emb.pow(2).sum(1).max()))


def spread(model, x, y, gen):
    """The docstring's codebook spreading, from the quantizer inputs of the eval-mode forward((x, y))."""
    books, cap = codebooks(model), []
    with torch.no_grad():
        for enc in model.encoders:
            enc.z_proj.bias.zero_()
        hooks = [q.register_forward_hook(lambda m, inp, out: cap.append((m, inp[0].detach()))) for q in books]
        model.eval()
        model((x, y))
        for h in hooks:
            h.remove()
        for q in books:
            if hasattr(q, "emb_init"):
                q.embeddings.copy_(torch.randn(q.embeddings.shape, generator=gen))
        at = {id(q): 0 for q in books}
        for q, z in cap:  # in run order: a shared codebook takes two rows per level
            zf = z.transpose(1, 2).reshape(-1, q.z_dim)
            n = min(2, zf.shape[0])
            rows = zf[torch.linspace(0, zf.shape[0] - 1, n).round().long()]
            rows = rows + 0.05 * rows.norm(dim=1, keepdim=True) / q.z_dim ** 0.5 * torch.randn(rows.shape, generator=gen)
            q.embeddings[at[id(q)]:at[id(q)] + n] = rows
            at[id(q)] += n
        for q in books:
            if hasattr(q, "emb_init"):
                q.emb_init.fill_(True)
                q.emb_sum.copy_(q.embeddings)
                q.emb_elem.fill_(1.0)
            else:
                q.embed_norm()


def run_utterance(model, x, y, ys):
    """The eval-mode conversions of one utterance: (xhat, xinf | None, style | None, forward's lookups, infer's
    lookups), a lookup being (indices, gap, scale, frames)."""
    look, style, hooks = [], [], []
    for q in codebooks(model):
        hooks.append(q.register_forward_hook(lambda m, inp, out: look.append((*nearest(inp[0], m), inp[0].shape[2]))))
    if model.use_gst:
        top = model.quantizers[model.levels - 1]
        hooks.append(top.register_forward_hook(lambda m, inp, out: style.append(out.detach().clone())))
    model.eval()
    with torch.no_grad():
        xhat = model((x, y))[0].detach().clone()
        for h in hooks:
            h.remove()
        fwd, xinf, inf = list(look), None, []
        if ys is not None:
            patched = []
            for q in codebooks(model):
                orig = q.encode

                def encode(z, q=q, orig=orig):
                    idx = orig(z)
                    found = nearest(z, q)
                    assert torch.equal(idx, found[0])
                    inf.append((*found, z.shape[2]))
                    return idx
                q.encode = encode
                patched.append(q)
            xinf = model.infer((x, ys)).detach().clone()
            for q in patched:
                del q.encode
    return xhat, xinf, (style[0] if style else None), fwd, inf


def enough(look, top_rule):
    """The gap rule over lookups; with top_rule 'proportional' the last (mean-pooled) lookup is held to the
    proportional rule."""
    need = [MIN_GAP] * len(look)
    if top_rule == "proportional":
        need[-1] = MIN_GAP / 128 * look[-1][2]
    return all(l[1] >= n for l, n in zip(look, need))


def attempt(ref, kind, arch, seed, top_rule):
    """One seed: None, or what make_ragged stores."""
    torch.manual_seed(seed)
    m = ref.Model(arch)
    mel, n_spk, U, levels = arch["encoder.0"]["in_channels"][0], arch["y_num"], len(LENGTHS), arch["levels"]
    xs = [torch.randn(1, mel, T) for T in LENGTHS]
    y = torch.randint(0, n_spk, (U, 1))
    y_tgt = (y + 1 + torch.randint(0, n_spk - 1, (U, 1))) % n_spk  # never y itself
    ys = (y_tgt + torch.arange(levels)) % n_spk if kind == "vq2b" else None  # a different speaker per level
    spread(m, xs[0], y[:1], torch.Generator().manual_seed(seed))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m64 = ref.Model(arch)
    torch.nn.Module.load_state_dict(m64, sd)  # the class's own override reads an attribute it never sets
    m64.double()
    runs = []
    for b, x in enumerate(xs):
        ysb = None if ys is None else ys[b:b + 1]
        r32 = run_utterance(m, x, y_tgt[b:b + 1], ysb)
        r64 = run_utterance(m64, x.double(), y_tgt[b:b + 1], ysb)
        every = [r32[3], r32[4], r64[3], r64[4]]
        if not all(enough(look, top_rule) for look in every if look):
            return None
        if not all(torch.equal(p[0], q[0]) for look in every[1:] if look for p, q in zip(every[0], look)):
            return None
        runs.append((r32, r64))
    # eval mode writes nothing but a normalised codebook, renormalised in place (embed_norm): its direction stays
    assert all(torch.allclose(v.float(), sd[k].float(), rtol=1e-5, atol=0) for k, v in m.state_dict().items())
    if not any(l[0].unique().numel() > 1 for _, r64 in runs for l in r64[3]):
        return None
    return xs, y, y_tgt, ys, sd, runs


def make_ragged(ref, kind, name):
    arch = KINDS[kind][1](name)
    key = f"{kind}_{name}"
    rules = ["absolute"] + (["proportional"] if name == "pooled_ema" else [])
    for top_rule in rules:
        for seed in range(SEEDS[key], SEEDS[key] + MAX_SEEDS):
            got = attempt(ref, kind, arch, seed, top_rule)
            if got:
                break
        if got:
            break
    else:
        raise RuntimeError(f"{key}: no seed in {MAX_SEEDS} gives the required gaps for every utterance")
    xs, y, y_tgt, ys, sd, runs = got
    arrays = {"y": y.numpy(), "y_tgt": y_tgt.numpy()}
    if ys is not None:
        arrays["ys"] = ys.numpy()
    err32, gaps, level_lengths = {}, [], None
    for b, (r32, r64) in enumerate(runs):
        arrays[f"x.{b}"] = xs[b][0].numpy()
        for tag, a32, a64 in (("xhat", r32[0], r64[0]), ("xinf", r32[1], r64[1]), ("style", r32[2], r64[2])):
            if a64 is not None:
                arrays[f"{tag}.{b}"] = a64[0].numpy()
                err32[f"{tag}.{b}"] = rel(a32, a64)
        for k, l in enumerate(r64[3]):
            arrays[f"idx.{b}.{k}"] = l[0][0].numpy()
        gaps.append(min(l[1] for r in (r32, r64) for look in (r[3], r[4]) for l in look))
        lens = [l[3] for l in r64[3]] + ([1] if r64[2] is not None else [])
        level_lengths = [[n] for n in lens] if level_lengths is None else [a + [n] for a, n in zip(level_lengths, lens)]
    for k in sd:
        arrays["param." + k] = sd[k].numpy()
    save(f"{kind}_ragged", name, arrays,
         {"seed": seed, "lengths": LENGTHS, "level_lengths": level_lengths, "arch": arch, "err32": err32,
          "keys": list(sd.keys()), "gap": min(gaps), "gaps": gaps, "top_rule": top_rule,
          "lookups": len(runs[0][1][3]), "style": runs[0][1][2] is not None})


if __name__ == "__main__":
    names = [f"{kind}_{n}" for kind in KINDS for n in KINDS[kind][0]]
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE, as make_golden.py)")
    ap.add_argument("--only", default=None, choices=names)
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    sys.path.insert(0, str(Path(a.reference)))
    for kind, (cases, _, module) in KINDS.items():
        ref = importlib.import_module(module)
        for name in cases:
            if a.only in (None, f"{kind}_{name}"):
                make_ragged(ref, kind, name)
