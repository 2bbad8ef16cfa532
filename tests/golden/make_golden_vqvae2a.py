"""Fixtures of the vqvae2a family: tests/golden/vqema_<case>, vqjit_<case> and
vq2a_<case> (.npz + .json each).

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2a.py --reference DIR [--only NAME]

vqema  the reference's `EMAVectorQuantizer` alone ('frame_mean'), in training
       mode: per step z, z_vq, z_enc_loss, the detail dict, the indices, dz of
       (W_ENC * z_enc_loss).backward(), the codebook the lookup used (K <= 64)
       and the four buffers after the step.
vqjit  the reference's `Jitter` alone, and `VectorQuantizer` followed by it.
vq2a   the reference's `vqvae2a.Model`: per step forward((x, y)) and
       loss.backward() (no optimizer), then encode(x) in eval mode.

As make_golden_vqvae2_model.py: a float32 run and a float64 twin from the same
state_dict, the float64 run stored as the expected value and
`err32 = max|f32 - f64| / max|f64|` recorded per tensor.

Both runs must consume the generators identically: torch and numpy are
reseeded (`run_seed`) right before each run, and where `_tile` draws noise
(N < K) the float64 run draws it in float32 and widens it (`torch.randn_like`
is wrapped for that run only: for float64 it draws other values).  The
float64 run also sets torch's default dtype to float64: update_emb multiplies
a `torch.zeros` one-hot matrix with z, which fails between dtypes.

The seed is advanced until every quantizer input has a top-2 distance gap
>= 1e-3 against the codebook it is looked up in, in both runs and at every
step, and both runs pick identical indices (MAX_SEEDS tries).

One case cannot meet an absolute 1e-3: in `vqema_tile_k64` (N = 10 < K = 64)
the codebook is `_tile`'s noisy copies of the frames, so the two nearest codes
of every frame are copies of itself, |noise|^2 ~ 1e-4 from it and ~1e-5 from
each other, whatever the seed.  Its input is scaled by 0.01 and its gap is
required in the same proportion to the distance's largest term as 1e-3 is in
the unit-variance D = 64 cases (|z|^2 + |e|^2 ~ 128 there):
gap >= 1e-3 / 128 * max(|z|^2 + |e|^2), i.e. ~65 fp32 ulp of that term.
"""
import argparse
import contextlib
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden_vqvae2_model import MAX_SEEDS, MIN_GAP, rel, save, top2_gap  # noqa: E402

W_ENC = 0.25
ZERO_GRAD = "mha.linear_k.bias"

# case: K, D, B, T, mu, training steps, input scale, eval forward afterwards, preloaded dead rows
EMA_CASES = {
    "init_k16": dict(K=16, D=64, B=2, T=16, mu=0.9, steps=2, scale=1.0, eval_after=True, dead=0),
    "tile_k64": dict(K=64, D=64, B=2, T=5, mu=0.9, steps=1, scale=0.01, eval_after=False, dead=0),
    "dead_k16": dict(K=16, D=64, B=2, T=16, mu=0.5, steps=1, scale=1.0, eval_after=False, dead=4),
    "k512": dict(K=512, D=128, B=9, T=64, mu=0.9, steps=1, scale=1.0, eval_after=False, dead=0),  # the recipe's
}
JIT_CASES = ("jitter", "plain_jitter")
JITTER_P = 0.12
MODEL_CASES = ("ema_gst", "plain_shared", "single_ema")
SEEDS = {n: 9700 + 10 * i for i, n in enumerate([*EMA_CASES, *JIT_CASES, *MODEL_CASES])}


def model_arch(case):
    """B 2, T 64, 16-32 channel convs, K 16, z_dim 64 as make_golden_vqvae2_model.model_arch, the decoders wired
    for vqvae2a's chain: decoder i reads cat([z_vq_i, decoder i+1's output]) and the 16-channel speaker embedding."""
    enc = dict(kernel_size=3, z_channels=64, dilation=False, stack_kernel_size=3, stack_layers=1,
               use_weight_norm=True, use_causal_conv=False)
    dec = dict(out_channels=[32], skip_channels=16, kernel_size=3, upsample_scales=[1], dilation=False,
               stack_kernel_size=3, stacks=[2], use_weight_norm=True, use_causal_conv=False, cond_channels=16)
    enc0 = dict(enc, in_channels=[24], out_channels=[32], downsample_scales=[1], stacks=[1])
    enc1 = dict(enc, in_channels=[32, 32], out_channels=[32, 32], downsample_scales=[2, 2], stacks=[1, 1])
    base = {"beta": 0.01, "y_num": 4, "y_dim": 16}
    ema = dict(z_num=16, z_dim=64, mu=0.9)
    if case == "single_ema":
        return dict(base, levels=1, use_ema=True, jitter_p=0.0, **{
            "encoder.0": enc0, "quantizer.0": ema, "decoder.0": dict(dec, in_channels=[64], final_channels=24)})
    if case == "ema_gst":  # level lengths 64 / 16 / 1 (the style level is pooled)
        return dict(base, levels=3, use_gst=True, use_ema=True, jitter_p=JITTER_P, **{
            "encoder.0": enc0, "encoder.1": enc1,
            "encoder.2": dict(enc, in_channels=[32, 32], out_channels=[32, 32], downsample_scales=[4, 4], stacks=[1, 1]),
            "quantizer.0": ema, "quantizer.1": dict(ema),
            "quantizer.2": dict(ref_embed_dim=64, gst_tokens=6, gst_token_dim=32, gst_heads=2),
            "decoder.2": dict(dec, in_channels=[32], final_channels=64),
            "decoder.1": dict(dec, in_channels=[128], final_channels=64),
            "decoder.0": dict(dec, in_channels=[128], final_channels=24)})
    if case == "plain_shared":  # level lengths 64 / 16 / 4: the jittered top level needs more than one frame
        return dict(base, levels=3, use_gst=False, use_ema=False, jitter_p=JITTER_P, use_quantizers=False,
                    use_embeds=False, pooling_last=False, upsample_last=True, **{
            "encoder.0": enc0, "encoder.1": enc1,
            "encoder.2": dict(enc, in_channels=[32, 32], out_channels=[32, 32], downsample_scales=[2, 2], stacks=[1, 1]),
            # not normalised: the reference's embed_norm() rewrites the shared parameter in place at every level,
            # under the graph of the level before, and its backward then refuses
            "quantizer": dict(z_num=16, z_dim=64, normalize=False),
            "decoder.2": dict(dec, in_channels=[64], final_channels=64),
            "decoder.1": dict(dec, in_channels=[128], final_channels=64),
            "decoder.0": dict(dec, in_channels=[128], final_channels=24)})
    raise KeyError(case)


def load_reference(root):
    sys.path.insert(0, str(Path(root)))
    return (importlib.import_module("vae_npvc.model.vqvae2a"), importlib.import_module("vae_npvc.model.layers_vq"))


@contextlib.contextmanager
def f32_noise(on):
    """The float64 run: torch.randn_like of a float64 tensor draws the float32 values, widened, and torch's default
    dtype is float64 (update_emb builds its one-hot matrix with torch.zeros and multiplies it with z)."""
    orig = torch.randn_like
    if on:
        torch.randn_like = lambda t, **kw: (orig(t, dtype=torch.float32, **kw).to(t.dtype)
                                            if t.dtype == torch.float64 else orig(t, **kw))
        torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.randn_like = orig
        torch.set_default_dtype(torch.float32)


def reseed(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)


def lookup(zf, E):
    """(indices, smallest top-2 gap, max(|z|^2 + |e|^2)) of frames zf [N, D] against E (layers_vq.py:287-291)."""
    zf, E = zf.detach(), E.detach()
    d = zf.pow(2).sum(1, keepdim=True) + E.pow(2).sum(1) - 2 * zf @ E.t()
    t = d.topk(2, dim=1, largest=False).values
    return d.argmin(1), float((t[:, 1] - t[:, 0]).min()), float(zf.pow(2).sum(1).max() + E.pow(2).sum(1).max())


def watch_ema(q, log):
    """Record (indices, gap, scale, codebook) of every training lookup of an EMAVectorQuantizer: update_emb receives the
    flattened frames while `embeddings` still holds the codebook the lookup used."""
    orig = q.update_emb

    def update_emb(z, z_idx):
        idx, gap, scale = lookup(z, q.embeddings)
        assert torch.equal(idx, z_idx)
        log.append((idx.clone(), gap, scale, q.embeddings.detach().clone()))
        return orig(z, z_idx)
    q.update_emb = update_emb


def buffers_of(mod, prefix=""):
    return {prefix + k: v.detach().clone() for k, v in mod.named_buffers()}


# ---------------------------------------------------------------- EMA quantizer alone
def ema_state(c, z, gen):
    """dead_k16: an initialised codebook whose first K - dead rows are frames of z and whose last `dead` rows lie far
    from every frame with emb_elem 0.5 < threshold (mu 0.5: 0.25 after the step, so they are replaced)."""
    K, D, dead = c["K"], c["D"], c["dead"]
    zf = z.transpose(1, 2).reshape(-1, D)
    E = torch.empty(K, D)
    E[:K - dead] = zf[torch.linspace(0, zf.shape[0] - 1, K - dead).round().long()]
    E[K - dead:] = 50.0 + torch.randn(dead, D, generator=gen)
    elem = torch.ones(K)
    elem[K - dead:] = 0.5
    return {"emb_init": torch.tensor(True), "emb_sum": E * elem[:, None], "emb_elem": elem, "embeddings": E.clone()}


def run_ema(vq_mod, c, state, zs, run_seed, double):
    q = vq_mod.EMAVectorQuantizer(c["K"], c["D"], c["mu"])
    if state is not None:
        q.load_state_dict(state)
    if double:
        q.double()
    q.train()
    log, steps = [], []
    watch_ema(q, log)
    reseed(run_seed)
    with f32_noise(double):
        for z in zs:
            zz = (z.double() if double else z).clone().requires_grad_()
            z_vq, _, enc, detail = q(zz)
            (W_ENC * enc).backward()
            idx, gap, scale, E = log.pop()
            r = {"z_vq": z_vq.detach(), "z_enc_loss": enc.detach(), "dz": zz.grad.detach()}
            if c["K"] <= 64:
                r["codebook"] = E  # the codebook the lookup used (after init_emb on the first step)
            r.update({k: torch.tensor(float(v), dtype=zz.dtype) for k, v in detail.items()})
            r.update(buffers_of(q, "buf."))
            steps.append((r, idx.view(z.shape[0], z.shape[2]), gap, scale))
        if c["eval_after"]:
            q.eval()
            zz = zs[-1].double() if double else zs[-1]
            before = buffers_of(q)
            z_vq, _, enc, detail = q(zz)
            assert detail == {} and all(torch.equal(v, before[k]) for k, v in buffers_of(q).items())
            idx, gap, scale = lookup(zz.transpose(1, 2).reshape(-1, c["D"]), q.embeddings)
            steps.append(({"z_vq": z_vq.detach(), "z_enc_loss": enc.detach()}, idx.view(zz.shape[0], zz.shape[2]),
                          gap, scale))
    return steps


def make_ema(vq_mod, name):
    c = EMA_CASES[name]
    relative = name == "tile_k64"
    for seed in range(SEEDS[name], SEEDS[name] + MAX_SEEDS):
        gen = torch.Generator().manual_seed(seed)
        zs = [c["scale"] * torch.randn(c["B"], c["D"], c["T"], generator=gen) for _ in range(c["steps"])]
        state = ema_state(c, zs[0], gen) if c["dead"] else None
        s32 = run_ema(vq_mod, c, state, zs, seed, False)
        s64 = run_ema(vq_mod, c, state, zs, seed, True)
        need = lambda scale: MIN_GAP / 128 * scale if relative else MIN_GAP  # noqa: E731
        ok = all(torch.equal(a[1], b[1]) and min(a[2], b[2]) >= need(max(a[3], b[3])) for a, b in zip(s32, s64))
        if c["dead"]:
            ok = ok and float(s64[0][0]["usage"]) < c["K"]
        if ok:
            break
    else:
        raise RuntimeError(f"vqema_{name}: no seed in {MAX_SEEDS} gives the required gaps")
    arrays, err32 = {}, {}
    names = [f"s{i + 1}" for i in range(c["steps"])] + (["eval"] if c["eval_after"] else [])
    for n, (r32, _, _, _), (r64, idx, _, _) in zip(names, s32, s64):
        arrays[f"{n}.idx"] = idx.numpy()
        for k, v in r64.items():
            arrays[f"{n}.{k}"] = v.numpy()
            if v.is_floating_point():
                err32[f"{n}.{k}"] = rel(r32[k], v)
    for i, z in enumerate(zs):
        arrays[f"s{i + 1}.z"] = z.numpy()
    if state is not None:
        arrays.update({"state." + k: v.numpy() for k, v in state.items()})
    save("vqema", name, arrays,
         dict({k: c[k] for k in ("K", "D", "B", "T", "mu", "steps", "eval_after")}, seed=seed, run_seed=seed,
              w_enc=W_ENC, threshold=1.0, steps_names=names, relative_gap=relative,
              gaps32=[s[2] for s in s32], gaps64=[s[2] for s in s64], gap=min(s[2] for s in s32 + s64),
              detail_keys=["entropy", "used_curr", "usage", "diff_emb"], err32=err32))


# ---------------------------------------------------------------- jitter
def jitter_map(x, y):
    """The neighbour map the reference's Jitter applied: frame t of y is frame t-1, t or t+1 of x."""
    T = x.shape[2]
    out = []
    for t in range(T):
        hit = [s for s in (t, t - 1, t + 1) if 0 <= s < T and torch.equal(y[:, :, t], x[:, :, s])]
        assert len(hit) == 1, (t, hit)
        out.append(hit[0])
    return np.asarray(out, dtype=np.int32)


def run_jitter(vq_mod, x, go, run_seed, double):
    jit = vq_mod.Jitter(JITTER_P).train()
    xx = (x.double() if double else x).clone().requires_grad_()
    reseed(run_seed)
    y = jit(xx * 1.0)  # the reference writes into its argument: not a leaf
    nxt = float(np.random.random_sample())
    (y * (go.double() if double else go)).sum().backward()
    return {"y": y.detach(), "dx": xx.grad.detach()}, jitter_map(xx.detach(), y.detach()), nxt


def make_jitter(vq_mod, name):
    B, C, T = 2, 64, 7
    for seed in range(SEEDS[name], SEEDS[name] + MAX_SEEDS):
        gen = torch.Generator().manual_seed(seed)
        x, go = torch.randn(B, C, T, generator=gen), torch.randn(B, C, T, generator=gen)
        r32, m32, n32 = run_jitter(vq_mod, x, go, seed, False)
        r64, m64, n64 = run_jitter(vq_mod, x, go, seed, True)
        moved = m64 != np.arange(T)
        if (m32 == m64).all() and n32 == n64 and moved[1:-1].any() and not moved.all():
            break
    else:
        raise RuntimeError("vqjit_jitter: no seed gives a map with kept and replaced frames")
    arrays = {"x": x.numpy(), "go": go.numpy(), "map": m64, "y": r64["y"].numpy(), "dx": r64["dx"].numpy()}
    save("vqjit", name, arrays, {"seed": seed, "run_seed": seed, "p": JITTER_P, "B": B, "C": C, "T": T,
                                 "next_uniform": n64, "err32": {k: rel(r32[k], r64[k]) for k in r64}})


def run_plain_jitter(vq_mod, E0, z, go, run_seed, double):
    K, D = E0.shape
    q = vq_mod.VectorQuantizer(K, D, normalize=True, reduction="frame_mean")
    q.load_state_dict({"embeddings": E0})
    jit = vq_mod.Jitter(JITTER_P).train()
    if double:
        q.double()
    zz = (z.double() if double else z).clone().requires_grad_()
    reseed(run_seed)
    z_vq, qut, enc, detail = q(zz)
    plain = z_vq.detach().clone()
    y = jit(z_vq)
    nxt = float(np.random.random_sample())
    ((y * (go.double() if double else go)).sum() + 1.0 * qut + W_ENC * enc).backward()
    with torch.no_grad():
        idx = q.encode(zz)
    r = {"z_vq": y.detach(), "z_qut_loss": qut.detach(), "z_enc_loss": enc.detach(),
         "entropy": torch.tensor(detail["entropy"], dtype=zz.dtype), "dz": zz.grad.detach(),
         "dE": q.embeddings.grad.detach()}
    return r, idx, jitter_map(plain, y.detach()), nxt, top2_gap(zz, q.embeddings, True)


def make_plain_jitter(vq_mod, name):
    K, D, B, T = 16, 64, 2, 7
    for seed in range(SEEDS[name], SEEDS[name] + MAX_SEEDS):
        gen = torch.Generator().manual_seed(seed)
        E0 = torch.randn(K, D, generator=gen)
        z, go = torch.randn(B, D, T, generator=gen), torch.randn(B, D, T, generator=gen)
        r32, i32, m32, n32, g32 = run_plain_jitter(vq_mod, E0, z, go, seed, False)
        r64, i64, m64, n64, g64 = run_plain_jitter(vq_mod, E0, z, go, seed, True)
        moved = m64 != np.arange(T)
        if (m32 == m64).all() and n32 == n64 and moved[1:-1].any() and not moved.all() and torch.equal(i32, i64) \
                and min(g32, g64) >= MIN_GAP and i64.unique().numel() > 1:
            break
    else:
        raise RuntimeError("vqjit_plain_jitter: no seed gives the required gap and map")
    arrays = {"z": z.numpy(), "go": go.numpy(), "param.embeddings": E0.numpy(), "idx": i64.numpy(), "map": m64}
    arrays.update({k: v.numpy() for k, v in r64.items()})
    save("vqjit", name, arrays, {"seed": seed, "run_seed": seed, "p": JITTER_P, "K": K, "D": D, "B": B, "T": T,
                                 "normalize": True, "loss_weights": [1.0, W_ENC], "next_uniform": n64,
                                 "gap": min(g32, g64), "err32": {k: rel(r32[k], r64[k]) for k in r64}})


# ---------------------------------------------------------------- model
def quantized(model):
    """The codebook modules of a vqvae2a.Model, once each."""
    mods = list(model.quantizers) if model.use_quantizers else [model.quantizer]
    return [q for q in mods if hasattr(q, "embeddings")]


def watch_model(model, log):
    """Every codebook lookup of the forward, in the order they run: (indices (B, T), gap)."""
    hooks = []
    for q in quantized(model):
        if hasattr(q, "update_emb"):
            cur = {}
            watch_ema(q, cur.setdefault("log", []))
            hooks.append(q.register_forward_hook(
                lambda m, inp, out, cur=cur: log.append((cur["log"][-1][0].view(inp[0].shape[0], -1), cur["log"].pop()[1]))))
        else:
            hooks.append(q.register_forward_hook(
                lambda m, inp, out: log.append((m.encode(inp[0].detach()), top2_gap(inp[0], m.embeddings, m.normalize)))))
    return hooks


def spread_shared(model, x, y, gen):
    """plain_shared: a random codebook leaves every frame of a level on one code.  Two rows of the shared codebook per
    level become evenly spaced frames of that level's quantizer input with 5 % noise (the inputs are the encoders'
    outputs, which do not depend on the codebook); the z_proj biases, the part every frame shares, are zeroed first."""
    q, cap = model.quantizer, []
    with torch.no_grad():
        for enc in model.encoders:
            enc.z_proj.bias.zero_()
        h = q.register_forward_hook(lambda m, inp, out: cap.append(inp[0].detach()))
        model.eval()
        model((x, y))
        model.train()
        h.remove()
        for lvl, z in enumerate(cap):
            zf = z.transpose(1, 2).reshape(-1, q.z_dim)
            rows = zf[torch.linspace(0, zf.shape[0] - 1, 2).round().long()]
            rows = rows + 0.05 * rows.norm(dim=1, keepdim=True) / q.z_dim ** 0.5 * torch.randn(rows.shape, generator=gen)
            q.embeddings[2 * lvl:2 * lvl + 2] = rows
        q.embed_norm()


def run_model(model, x, y, steps, run_seed, double):
    log, out = [], []
    hooks = watch_model(model, log)
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
        gaps = []
        feat = x
        for i in range(model.levels):  # the gaps of encode's lookups, against the codebooks as they are now
            z, feat = model.encoders[i](feat)
            q = model.quantizers[i] if model.use_quantizers else model.quantizer
            if hasattr(q, "embeddings"):
                if model.pooling_last and i == model.levels - 1:
                    z = z.mean(dim=-1, keepdim=True)
                gaps.append(top2_gap(z, q.embeddings, getattr(q, "normalize", False)))
    model.train()
    return out, codes, gaps


def make_model(ref, name):
    arch = model_arch(name)
    steps = 1 if name == "plain_shared" else 2
    B, T = 2, 64
    for seed in range(SEEDS[name], SEEDS[name] + MAX_SEEDS):
        torch.manual_seed(seed)
        m = ref.Model(arch)
        x = torch.randn(B, arch["encoder.0"]["in_channels"][0], T)
        y = torch.randint(0, arch["y_num"], (B, 1))
        if name == "plain_shared":
            spread_shared(m, x, y, torch.Generator().manual_seed(seed))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        o32, c32, eg32 = run_model(m, x, y, steps, seed, False)
        look32 = [l for s in o32 for l in s["lookups"]]
        varied = all(idx.unique().numel() > 1 for idx, _ in look32 if idx.numel() > B)
        if not varied or min([g for _, g in look32] + eg32) < MIN_GAP:
            continue
        m64 = ref.Model(arch)
        torch.nn.Module.load_state_dict(m64, sd)
        m64.double()
        o64, c64, eg64 = run_model(m64, x.double(), y, steps, seed, True)
        look64 = [l for s in o64 for l in s["lookups"]]
        same = all(torch.equal(a[0], b[0]) for a, b in zip(look32, look64)) and \
            all(torch.equal(a, b) for a, b in zip(c32, c64) if not a.is_floating_point())
        if same and min([g for _, g in look64] + eg64) >= MIN_GAP:
            break
    else:
        raise RuntimeError(f"vq2a_{name}: no seed in {MAX_SEEDS} gives varied indices with gaps >= {MIN_GAP}")
    arrays = {"x": x.numpy(), "y": y.numpy()}
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
        for j, (idx, _) in enumerate(s64["lookups"]):
            arrays[p + f"idx.{j}"] = idx.numpy()
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
    save("vq2a", name, arrays,
         {"seed": seed, "run_seed": seed, "steps": steps, "B": B, "T": T, "arch": arch, "err32": err32, "abs32": abs32,
          "keys": list(sd.keys()), "params": [k for k, _ in m.named_parameters()],
          "grads": list(o64[0]["grads"].keys()), "buffers": list(o64[0]["buffers"].keys()),
          "loss_keys": [list(s["detail"].keys()) for s in o64], "lookups": [len(s["lookups"]) for s in o64],
          "gap": min([g for _, g in look32 + look64] + eg32 + eg64),
          "gaps32": [g for _, g in look32], "gaps64": [g for _, g in look64], "encode_gaps": eg32 + eg64})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE, as make_golden.py)")
    ap.add_argument("--only", default=None, choices=sorted([*EMA_CASES, *JIT_CASES, *MODEL_CASES]))
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    ref, vq_mod = load_reference(a.reference)
    for name in EMA_CASES:
        if a.only in (None, name):
            make_ema(vq_mod, name)
    if a.only in (None, "jitter"):
        make_jitter(vq_mod, "jitter")
    if a.only in (None, "plain_jitter"):
        make_plain_jitter(vq_mod, "plain_jitter")
    for name in MODEL_CASES:
        if a.only in (None, name):
            make_model(ref, name)
