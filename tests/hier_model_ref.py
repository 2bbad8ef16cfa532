"""Plain-torch restatement of the hierarchical model (reference vqvae2.py
Encoder.forward and Model.forward, layers_vq.py VectorQuantizer.forward,
layers_gst.py StyleTokenLayer, layers.py log_loss) for the tests, beside
tests/hier_ref.py (the decoder).  tests/test_hier_model_host.py pins it to the
reference's float64 fixtures (tests/golden/make_golden_vqvae2_model.py); the
GPU tests use it for shapes the fixtures do not cover."""
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import GOLD
from tests.hier_ref import as_numpy, restated_decoder, stretch

ENC_CASES = ("s1", "down2x2", "down4x4_T1", "nown")
LEVEL_CASES = ("k16_norm", "k16_plain", "k512_norm")
MODEL_CASES = ("gst", "plain_top")
ULP16 = 16 * 2.0 ** -23
_cache = {}


def fixture(kind, case):
    """(meta, arrays) of tests/golden/<kind>_<case> (kind: vqenc | vqlevel | vqmodel); loaded once, read-only."""
    key = f"{kind}_{case}"
    if key not in _cache:
        meta = json.load(open(GOLD / f"{key}.json"))
        arr = {}
        for name in meta["files"]:
            arr.update(np.load(GOLD / name, allow_pickle=False))
        for v in arr.values():
            v.setflags(write=False)
        _cache[key] = (meta, arr)
    return _cache[key]


def _conv_w(params, pre):
    if pre + ".weight_g" in params:
        return torch._weight_norm(params[pre + ".weight_v"], params[pre + ".weight_g"], 0)
    return params[pre + ".weight"]


def restated_encoder(args, params, x, prefix=""):
    """vqvae2.Encoder(**args) with parameters `params` on x -> (z, feat)."""
    k, ks, L = args["kernel_size"], args["stack_kernel_size"], args["stack_layers"]
    i = 0
    for cout, s, nst in zip(args["out_channels"], args["downsample_scales"], args["stacks"]):
        pre = f"{prefix}encode.{i}"
        if s == 1:
            x = F.conv1d(x, _conv_w(params, pre), params[pre + ".bias"], padding=(k - 1) // 2)
        else:
            x = F.conv1d(x, _conv_w(params, pre), params[pre + ".bias"], stride=s, padding=s // 2 + s % 2)
        i += 1
        for j in range(nst):
            d = 2 ** j if args["dilation"] else 1
            pre = f"{prefix}encode.{i}"
            h = x
            for l in range(L):
                dl = d if l == 0 else 1
                h = F.conv1d(F.leaky_relu(h, 0.2), _conv_w(params, f"{pre}.stack.{3 * l + 1}"),
                             params[f"{pre}.stack.{3 * l + 1}.bias"], padding=(ks - 1) // 2 * dl, dilation=dl)
                h = F.group_norm(h, 1, params[f"{pre}.stack.{3 * l + 2}.weight"],
                                 params[f"{pre}.stack.{3 * l + 2}.bias"], eps=1e-5)
            x = h + F.conv1d(x, _conv_w(params, pre + ".skip_layer"), params[pre + ".skip_layer.bias"])
            i += 1
        x = F.leaky_relu(x, 0.2)
        i += 1
    pre = f"{prefix}z_proj"
    return F.conv1d(x, _conv_w(params, pre), params[pre + ".bias"]), x


def restated_quantizer(E, z, normalize):
    """VectorQuantizer.forward (layers_vq.py:79-150, 'frame_mean') on z (B, D, T)
    with the codebook E *after* embed_norm() -> z_vq, z_qut_loss, z_enc_loss,
    perplexity, indices (B, T), smallest top-2 distance gap."""
    B, D, T = z.shape
    zf = z.transpose(1, 2).reshape(-1, D)
    if normalize:
        zn = 1.0 * zf / zf.norm(dim=1, keepdim=True)
        emb = 1.0 * E / E.norm(dim=1, keepdim=True)
    else:
        zn, emb = zf, E
    dist = zn.pow(2).sum(1, keepdim=True) + emb.pow(2).sum(1) - 2 * zn @ emb.t()
    idx = dist.argmin(1)
    top2 = dist.detach().topk(2, dim=1, largest=False).values
    gap = float((top2[:, 1] - top2[:, 0]).min())
    zq = emb.index_select(0, idx)
    counts = torch.bincount(idx, minlength=E.shape[0]).to(z.dtype)
    p = counts / idx.numel()
    perplexity = torch.exp(-(p * torch.log(p + 1e-10)).sum())
    qut = (zq - zn.detach()).pow(2).sum() / (B * T)
    enc = (zq.detach() - zn).pow(2)
    if normalize:
        enc = enc + (zn - zf).pow(2)
    enc = enc.sum() / (B * T)
    z_vq = zn + (zq - zn).detach()
    return z_vq.view(B, T, D).transpose(1, 2), qut, enc, perplexity, idx.view(B, T), gap


def embed_norm(E):
    """embed_norm() (layers_vq.py:28-33): the in-place row renormalisation forward applies first."""
    return E * (1.0 / E.norm(dim=1, keepdim=True))


def restated_gst(params, ref, heads, prefix=""):
    """StyleTokenLayer.forward (layers_gst.py) on ref (B, R) -> (B, F)."""
    p = lambda n: params[prefix + n]  # noqa: E731
    B = ref.shape[0]
    tok = torch.tanh(p("gst_embs"))
    q = F.linear(ref, p("mha.linear_q.weight"), p("mha.linear_q.bias")).view(B, heads, 1, -1)
    k = F.linear(tok, p("mha.linear_k.weight"), p("mha.linear_k.bias")).view(-1, heads, q.shape[-1]).transpose(0, 1)
    v = F.linear(tok, p("mha.linear_v.weight"), p("mha.linear_v.bias")).view(-1, heads, q.shape[-1]).transpose(0, 1)
    attn = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(q.shape[-1]), dim=-1)  # (B, H, 1, N)
    ctx = (attn @ v).transpose(1, 2).reshape(B, -1)
    return F.linear(ctx, p("mha.linear_out.weight"), p("mha.linear_out.bias"))


def _sub(params, prefix):
    return {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}


def restated_model(arch, params, x, y_idx):
    """Model.forward (vqvae2.py:74-127) with `params` holding the codebooks
    *after* embed_norm(): xhat, loss, {Total, VQ loss, X like, entropy.k,
    quanti_err.k} as tensors, indices per quantized level (append order), gaps."""
    levels, use_gst, beta = arch["levels"], arch["use_gst"], arch["beta"]
    y = params["embeds._embedding.weight"][y_idx[..., :1]].transpose(1, 2)
    z_levels, times, feat = [], [x.shape[-1]], x
    for i in range(levels):
        z, feat = restated_encoder(arch[f"encoder.{i}"], _sub(params, f"encoders.{i}."), feat)
        z_levels.append(z)
        times.append(z.shape[-1])
    z_vq_levels, quts, encs, perps, ids, gaps = [], [], [], [], [], []
    z = z_levels.pop()
    for i in reversed(range(levels)):
        if use_gst and i == levels - 1:
            z_vq = restated_gst(params, z.mean(dim=-1), arch[f"quantizer.{i}"]["gst_heads"],
                                f"quantizers.{i}.").unsqueeze(-1)
        else:
            z_vq, qut, enc, perp, idx, gap = restated_quantizer(params[f"quantizers.{i}.embeddings"], z,
                                                               arch[f"quantizer.{i}"].get("normalize", False))
            quts.append(qut)
            encs.append(enc)
            perps.append(perp)
            ids.append(idx)
            gaps.append(gap)
        z_vq_levels.append([stretch(z_vq, t) for t in times[:i + 1]])
        if i > 0:
            cond = torch.cat([zs[i] for zs in z_vq_levels], dim=1)
            z = restated_decoder(arch[f"decoder.{i}"], _sub(params, f"decoders.{i}."), z_levels.pop(), cond)
    z_vq = torch.cat([zs[0] for zs in z_vq_levels], dim=1)
    xhat = restated_decoder(arch["decoder.0"], _sub(params, "decoders.0."), z_vq, stretch(y, times[0]))
    z_qut, z_enc = sum(quts), sum(encs)
    x_loss = (0.5 * (math.log(2.0 * math.pi) + (xhat - x).pow(2))).sum() / (x.shape[0] * x.shape[2])
    loss = x_loss + z_qut + beta * z_enc
    detail = {"Total": loss, "VQ loss": z_enc, "X like": x_loss}
    for k, (p, e) in enumerate(zip(perps, encs)):
        detail[f"entropy.{k}"] = p
        detail[f"quanti_err.{k}"] = e
    return xhat, loss, detail, ids, gaps


def tensors(arr, keys, prefix, dtype, grad=True):
    """{key: tensor of arr[prefix + key]} as `dtype` leaves."""
    out = {}
    for k in keys:
        t = torch.from_numpy(as_numpy(arr[prefix + k]))
        if t.is_floating_point():
            t = t.to(dtype)
            if grad:
                t.requires_grad_()
        out[k] = t
    return out


def run_restated_encoder(args, sd, x, dz, dfeat, dtype=torch.float64, autocast=False):
    """{"z", "feat", "dx", "<key>" gradient...}; dz / dfeat may be None."""
    t = lambda a: torch.from_numpy(as_numpy(a)).to(dtype)  # noqa: E731
    params = {k: t(v).requires_grad_() for k, v in sd.items()}
    xx = t(x).requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        z, feat = restated_encoder(args, params, xx)
    outs, gos = [], []
    for o, g in ((z, dz), (feat, dfeat)):
        if g is not None:
            outs.append(o.float() if autocast else o)
            gos.append(t(g).float() if autocast else t(g))
    torch.autograd.backward(outs, gos)
    res = {"z": z.detach(), "feat": feat.detach(), "dx": xx.grad}
    res.update({k: p.grad for k, p in params.items() if p.grad is not None})
    return res


def fast_encoder_case(seed=9400, B=2, T=256, C=128):
    """The fast-kernel encoder case (T' % 128 == 0, C % 128 == 0): args, a seeded state_dict, x, dz, dfeat."""
    from vae_npvc_amd.model.vqvae2 import Encoder
    args = dict(in_channels=[C], out_channels=[C], downsample_scales=[1], kernel_size=3, z_channels=C, dilation=True,
                stack_kernel_size=3, stack_layers=2, stacks=[2], use_weight_norm=True, use_causal_conv=False)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    enc = Encoder(**args)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    for k, v in sd.items():  # move the GroupNorm affine off its 1 / 0 initial values
        if ".stack." in k and (k.endswith(".weight") or k.endswith(".bias")) and v.dim() == 1 \
                and k.rsplit(".", 2)[1] in ("2", "5"):
            v.add_(0.2 * torch.randn(v.shape, generator=g))
    x = torch.randn(B, C, T, generator=g)
    dz = torch.randn(B, C, T, generator=g)
    dfeat = torch.randn(B, C, T, generator=g)
    return args, sd, x, dz, dfeat
