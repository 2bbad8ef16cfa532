"""What every piece of the hierarchical models uses (reference model/vqvae2.py,
recipe egs/vcc20/vae2) on the MI355X: the host logic of level upsampling
(`Model.upsample`, vqvae2.py:130-143) and its concatenation (vqvae2.py:105-114)
with their autograd function, the mean pool of a top level, the fused log-loss
and the conv helpers of the decoder and encoder plans.  There is no CPU path.
"""
import functools

import torch
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops

F32 = torch.float32
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ------------------------------------------------------------------ host logic
def src_index(target_len, level_len):
    """Source frame of every output frame of `upsample` (vqvae2.py:130-143):
    repetition by target_len // level_len, the tail replicate-padded."""
    if not 1 <= level_len <= target_len:
        raise ValueError(f"upsample: level length {level_len} not in 1..{target_len}")
    r = target_len // level_len
    return [min(t // r, level_len - 1) for t in range(target_len)]


@functools.lru_cache(maxsize=256)
def choose_tc(T, level_lens):
    """Rate Tc of the conditioning term for levels of lengths `level_lens`
    stretched to T: max T_l when stretching every level to Tc and then to T
    lands on the frames of the direct stretch, else T (full rate)."""
    level_lens = tuple(level_lens)
    Tc = max(level_lens)
    if Tc == T:
        return T
    outer = src_index(T, Tc)
    for Tl in level_lens:
        inner, direct = src_index(Tc, Tl), src_index(T, Tl)
        if any(inner[outer[t]] != direct[t] for t in range(T)):
            return T
    return Tc


def to_rows(z):
    """(B, C, T) -> frame-major f32 [B*T, C]."""
    B, C, T = z.shape
    y = torch.empty(B * T, C, device=z.device, dtype=F32)
    ops.nct_to_ntc(z.float().contiguous(), y)
    return y


def to_nct(y, B, T):
    x = torch.empty(B, y.shape[1], T, device=y.device, dtype=F32)
    ops.ntc_to_nct(y, x)
    return x


# ------------------------------------------------------------------ upsampling
class _UpsampleCatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target_len, *levels):
        if not all(z.is_cuda for z in levels):
            raise L.VqxError("upsample_cat runs on the MI355X only (libvqx); move the levels with .cuda()")
        B = levels[0].shape[0]
        rows = [to_rows(z) for z in levels]
        out = torch.empty(B * target_len, sum(r.shape[1] for r in rows), device=levels[0].device, dtype=F32)
        ops.upsample_cat_fwd(rows, B, target_len, out)
        ctx.shapes, ctx.T = [tuple(z.shape) for z in levels], target_len
        return to_nct(out, B, target_len)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        B, T = ctx.shapes[0][0], ctx.T
        d = to_rows(dout)
        dl = [torch.empty(B * Tl, C, device=dout.device, dtype=F32) for _, C, Tl in ctx.shapes]
        ops.upsample_cat_bwd(dl, B, T, d)
        return (None, *[to_nct(g, B, s[2]) for g, s in zip(dl, ctx.shapes)])


def upsample_cat(levels, target_len):
    """cat([upsample(l, target_len) for l in levels], dim=1) for levels (B, C_l, T_l)."""
    levels = list(levels)
    if not levels or any(z.dim() != 3 or z.shape[0] != levels[0].shape[0] for z in levels):
        raise ValueError("upsample_cat: levels must be (B, C_l, T_l) tensors of one batch size")
    for z in levels:
        src_index(target_len, z.shape[2])
    return _UpsampleCatFn.apply(target_len, *levels)


def upsample(z, target_len):
    """The reference's Model.upsample (vqvae2.py:130-143) for z (B, C, T_l), T_l <= target_len."""
    return upsample_cat([z], target_len)


class _MeanPoolFn(torch.autograd.Function):
    """torch.mean(z, dim=-1, keepdim=True) of z (B, C, T) (vqvae2a.py:145-146):
    the per-utterance column sums of vqx_upsample_cat_bwd (one level of one
    frame) times 1/T; the backward stretches g/T back over the T frames."""

    @staticmethod
    def forward(ctx, z):
        B, C, T = z.shape
        total = torch.empty(B, C, device=z.device, dtype=F32)
        ops.upsample_cat_bwd([total], B, T, to_rows(z))
        ctx.dims = (B, C, T)
        return ops.scale_act_2d(total, torch.empty_like(total), 1.0 / T, L.PRO_NONE).view(B, C, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        B, C, T = ctx.dims
        rows = g.float().reshape(B, C).contiguous()
        rows = ops.scale_act_2d(rows, torch.empty_like(rows), 1.0 / T, L.PRO_NONE)
        out = ops.upsample_cat_fwd([rows], B, T, torch.empty(B * T, C, device=g.device, dtype=F32))
        return to_nct(out, B, T)


def mean_pool(z):
    if not z.is_cuda:
        raise L.VqxError("vqvae2a.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
    return _MeanPoolFn.apply(z)


# ------------------------------------------------------------------ loss
class LogLossFn(torch.autograd.Function):
    """log_loss(xhat, x) (layers.py:283-296, 'frame_mean') as vqx_logloss_fwd_bwd:
    the launch that sums the loss also writes d loss / d xhat; the backward is
    its layout change with the upstream gradient folded in (vqx_ntc_to_nct_scale)."""

    @staticmethod
    def forward(ctx, xhat, x):
        B, C, T = x.shape
        rows = to_rows(xhat)
        loss = torch.empty(1, device=x.device, dtype=F32)
        dxhat = torch.empty_like(rows)
        ops.logloss_fwd_bwd(x, rows, 1.0 / (B * T), dxhat, loss, torch.empty(1024, device=x.device, dtype=F32))
        ctx.dims = (B, T)
        ctx.save_for_backward(dxhat)
        return loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dxhat, = ctx.saved_tensors
        B, T = ctx.dims
        dx = torch.empty(B, dxhat.shape[1], T, device=dxhat.device, dtype=F32)
        return ops.ntc_to_nct_scale(dxhat, g.detach().float().reshape(1).contiguous(), dx), None


# ------------------------------------------------------------------ conv helpers
# `cv` is one conv of a plan (hier_decoder._Conv, hier_encoder._EConv): its
# geometry as transposed, k, dil, pad, cin, cout.
def pack(w, transposed, dt):
    """torch-layout effective weight -> the GEMMs' [cout, k*cin] (include/vqx.h;
    ConvTranspose: tap j reads v[ci][co][k-1-j])."""
    if transposed:
        return w.flip(2).permute(1, 2, 0).reshape(w.shape[1], -1).to(dt).contiguous()
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).to(dt).contiguous()


def _unpack_grad(slabs, transposed, k):
    """Split-K weight-gradient slabs [splits, r, k*c] -> dL/dw in torch's layout."""
    g = slabs.sum(0) if slabs.shape[0] > 1 else slabs[0]
    g = g.view(g.shape[0], k, -1)
    return (g.flip(1) if transposed else g).permute(0, 2, 1)


def wgrad(cv, dy, x, T):
    """Slabs of dL/dw (fp32) of conv `cv` from its output gradient dy and input x."""
    n = dy.shape[0]
    if cv.transposed:
        p, q, r, c, sign = x, dy, cv.cin, cv.cout, -1
    else:
        p, q, r, c, sign = dy, x, cv.cout, cv.cin, 1
    tiles = ops.wgrad_tiles(n, T, r, c, cv.k, cv.pad, ops.dt_code(dy.dtype), dil=cv.dil)
    splits = max(1, min(512 // max(1, tiles), n // 512))
    slabs = torch.empty(splits, r, cv.k * c, device=dy.device, dtype=F32)
    ops.conv_wgrad(p, q, slabs, T=T, r_dim=r, c_dim=c, ntaps=cv.k, pad=cv.pad, dil=cv.dil, shift_sign=sign,
                   splits=splits)
    return _unpack_grad(slabs, cv.transposed, cv.k)


def fwd(cv, x, w, y, T, **kw):
    return ops.conv_fwd(x, w, y, T=T, cin=cv.cin, cout=cv.cout, ntaps=cv.k, pad=cv.pad, dil=cv.dil, **kw)


def dgrad(cv, dy, w, dx, T, **kw):
    return ops.conv_dgrad(dy, w, dx, T=T, cin=cv.cout, cout=cv.cin, ntaps=cv.k, pad=(cv.k - 1) * cv.dil - cv.pad,
                          dil=cv.dil, **kw)


def colsum(x, part):
    out = torch.empty(x.shape[1], device=x.device, dtype=F32)
    return ops.colsum(x, part, out)
