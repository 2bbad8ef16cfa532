"""Building blocks of the hierarchical model (reference model/vqvae2.py, recipe
egs/vcc20/vae2) on the MI355X: level upsampling (`Model.upsample`,
vqvae2.py:130-143), its concatenation (vqvae2.py:105-114) and the decoder
with conditioning that varies in time (`Decoder`, vqvae2.py:274-371).

`Decoder` has the reference's constructor arguments, module tree, parameter
order and state_dict keys (those of `model.vqvae.Decoder`, which it extends)
plus `compute_dtype: fp32|bf16`.  `forward((x, c))` takes the reference's
full-rate conditioning tensor `c` (B, cond, T) or a list of levels
(B, C_l, T_l) that stands for `cat([upsample(l, T)])`.

Every ResSkip block adds conv_cond(c) before its GroupNorm (layers.py:229-236).
conv_cond is 1x1, so it commutes with the stretching: the term is computed at
the conditioning's own rate Tc (B*Tc rows) and added in the conv_in GEMM's
epilogue by segment (vqx_conv_args.rowbias_T); neither the stretched `c` nor
conv_cond(c) exists at full rate, forward or backward.

The forward and backward are the launch sequences of engine/step.py
decoder_fwd / decoder_bwd composed from `ops.*` calls inside one
torch.autograd.Function.  Weight norm goes through torch autograd on
`effective_weight()`: the function receives w = g*v/||v|| in torch's layout,
packs it for the GEMMs and returns dL/dw in the same layout.  The conditioning
GEMMs (conv_cond and its gradients) run in fp32 in both compute dtypes, as the
engine's speaker conditioning does.  There is no CPU path.
"""
import functools
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .layers import Conditions, ResSkipBlock, WNConv1d
from .layers_gst import StyleTokenLayer
from .layers_vq import Jitter, VectorQuantizer
from .resample import ResampleConv1d
from .vqvae import Decoder as _Decoder
from .vqvae import Encoder as _Encoder

F32 = torch.float32
_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


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


def _to_rows(z):
    """(B, C, T) -> frame-major f32 [B*T, C]."""
    B, C, T = z.shape
    y = torch.empty(B * T, C, device=z.device, dtype=F32)
    ops.nct_to_ntc(z.float().contiguous(), y)
    return y


def _to_nct(y, B, T):
    x = torch.empty(B, y.shape[1], T, device=y.device, dtype=F32)
    ops.ntc_to_nct(y, x)
    return x


class _UpsampleCatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target_len, *levels):
        if not all(z.is_cuda for z in levels):
            raise L.VqxError("upsample_cat runs on the MI355X only (libvqx); move the levels with .cuda()")
        B = levels[0].shape[0]
        rows = [_to_rows(z) for z in levels]
        out = torch.empty(B * target_len, sum(r.shape[1] for r in rows), device=levels[0].device, dtype=F32)
        ops.upsample_cat_fwd(rows, B, target_len, out)
        ctx.shapes, ctx.T = [tuple(z.shape) for z in levels], target_len
        return _to_nct(out, B, target_len)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        B, T = ctx.shapes[0][0], ctx.T
        d = _to_rows(dout)
        dl = [torch.empty(B * Tl, C, device=dout.device, dtype=F32) for _, C, Tl in ctx.shapes]
        ops.upsample_cat_bwd(dl, B, T, d)
        return (None, *[_to_nct(g, B, s[2]) for g, s in zip(dl, ctx.shapes)])


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


# ------------------------------------------------------------------ decoder
def _pack(w, transposed, dt):
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


class _Conv:
    """One conv of the plan: geometry + where its tensors sit in the flat argument list."""

    def __init__(self, mod, at):
        self.transposed, self.k, self.dil = mod.transposed, mod.k, mod.dilation
        self.cin, self.cout = mod.cin, mod.cout
        self.pad = (mod.k - 1) * mod.dilation - mod.padding if mod.transposed else mod.padding
        if 2 * self.pad != (mod.k - 1) * mod.dilation:
            raise NotImplementedError("asymmetric padding (the output length would change)")
        self.at = at  # index of w in the tensor list; bias follows


def _wgrad(cv, dy, x, T):
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


def _fwd(cv, x, w, y, T, **kw):
    return ops.conv_fwd(x, w, y, T=T, cin=cv.cin, cout=cv.cout, ntaps=cv.k, pad=cv.pad, dil=cv.dil, **kw)


def _dgrad(cv, dy, w, dx, T, **kw):
    return ops.conv_dgrad(dy, w, dx, T=T, cin=cv.cout, cout=cv.cin, ntaps=cv.k, pad=(cv.k - 1) * cv.dil - cv.pad,
                          dil=cv.dil, **kw)


def _colsum(x, part):
    out = torch.empty(x.shape[1], device=x.device, dtype=F32)
    return ops.colsum(x, part, out)


class _Plan:
    """Static description of a Decoder for _DecoderFn (no tensors)."""

    def __init__(self, dec):
        self.dt = _DT[dec.compute_dtype]
        self.steps, at = [], 0  # ("conv", _Conv) | ("block", conv_in, conv_cond | None, res_skip, at of gamma)
        for layer in dec.layers:
            if isinstance(layer, ResSkipBlock):
                if layer.conv_cond is None:  # unconditioned: 6 tensors per block
                    ci, cc, rs = _Conv(layer.conv_in, at), None, _Conv(layer.res_skip_layers, at + 4)
                    self.steps.append(("block", ci, cc, rs, at + 2))
                    at += 6
                    continue
                ci, cc, rs = _Conv(layer.conv_in, at), _Conv(layer.conv_cond, at + 2), _Conv(layer.res_skip_layers, at + 6)
                self.steps.append(("block", ci, cc, rs, at + 4))
                at += 8
            elif isinstance(layer, WNConv1d):
                self.steps.append(("conv", _Conv(layer, at)))
                at += 2
            else:
                raise NotImplementedError("resampling decoder stages are not built for the hierarchical decoder")
        if self.steps[-1][0] != "block" or any(a[0] == b[0] == "conv" for a, b in zip(self.steps, self.steps[1:])):
            raise NotImplementedError("every decoder stage needs at least one ResSkip block")
        self.fin1, self.fin2 = _Conv(dec.final_layer[1], at), _Conv(dec.final_layer[3], at + 2)
        self.n_tensors = at + 4
        self.scale = math.sqrt(1.0 / len(dec.layers))
        self.S, self.final, self.cond = dec.skip_ch, dec.final_ch, dec.cond_ch or 0

    @staticmethod
    def tensors(dec):
        """The flat tensor list the plan indexes: per conv (w, bias), per block
        conv_in, conv_cond (a conditioned block only), GroupNorm (gamma, beta), res_skip; then the final convs."""
        out = []
        for layer in dec.layers:
            if isinstance(layer, ResSkipBlock):
                out += [layer.conv_in.effective_weight(), layer.conv_in.bias]
                if layer.conv_cond is not None:
                    out += [layer.conv_cond.effective_weight(), layer.conv_cond.bias]
                out += [layer.norm_layer.weight, layer.norm_layer.bias,
                        layer.res_skip_layers.effective_weight(), layer.res_skip_layers.bias]
            else:
                out += [layer.effective_weight(), layer.bias]
        for i in (1, 3):
            out += [dec.final_layer[i].effective_weight(), dec.final_layer[i].bias]
        return out


def _decoder_rows(plan, x2, B, T, rows, T_levels, ts, lengths=None):
    """The decoder's forward launches on frame-major operands: x2 [B*T, C] in
    the compute dtype, the conditioning levels `rows` (f32 [B*T_l, C_l]) and the
    flat tensor list `ts`.  Returns xhat f32 [B*T, final] and what the backward
    reads (Tc, c_low, saved, wp, a_skip, f1, w1, w2).  An unconditioned plan
    (plan.cond == 0) takes rows = None: no row bias in the conv_in GEMMs, no
    conv_cond launches; Tc and c_low are None.

    lengths (forward only): utterance b owns rows t < lengths[b] of the padded
    T.  x2 must hold zeros in the other rows, the conditioning is one row per
    utterance or already at full rate (a per-utterance stretch is the caller's,
    vqx_codes_upsample_cat_len).  The GroupNorm statistics run over the valid
    rows (the *_len kernels, never the GEMM tiles), every operand of a conv
    with more than one tap is given a zero tail (ops.mask_tail after the GEMM
    that wrote it), and xhat comes back with zero tails."""
    dev, dt = x2.device, plan.dt
    lens = None if lengths is None else ops.len_array(lengths, B, "vqvae2.Decoder lengths")
    if lens is not None and plan.cond and T_levels and choose_tc(T, T_levels) not in (1, T):
        raise ValueError("vqvae2.Decoder: with lengths the conditioning is one row per utterance or full rate")
    N = B * T
    e = functools.partial(torch.empty, device=dev)
    # conditioning at its own rate: c_low [B*Tc, cond] f32
    if not plan.cond:
        Tc, c_low = None, None
    elif T_levels:
        Tc = choose_tc(T, T_levels)
        c_low = ops.upsample_cat_fwd(rows, B, Tc, e(B * Tc, plan.cond, dtype=F32))
    else:
        Tc, c_low = T, rows[0]
    skip32 = e(N, plan.S, dtype=F32)
    gn_part = e(B * 2 * 24, dtype=F32)
    wp, saved, first = {}, [], True  # packed weights by tensor index; per step what the backward reads
    cur = x2
    for st in plan.steps:
        if st[0] == "conv":
            cv = st[1]
            w = wp[cv.at] = _pack(ts[cv.at], cv.transposed, dt)
            y = e(N, cv.cout, dtype=dt)
            _fwd(cv, cur, w, y, T, bias=ts[cv.at + 1])
            if lens is not None:
                ops.mask_tail(y, T, lens)
            saved.append((cur,))
            cur = y
            continue
        _, ci, cc, rs, ag = st
        C = ci.cin
        w_in, w_rs = _pack(ts[ci.at], True, dt), _pack(ts[rs.at], False, dt)
        wp[ci.at], wp[rs.at] = w_in, w_rs
        seg = {}
        if cc is not None:
            w_cc = wp[cc.at] = _pack(ts[cc.at], False, F32)
            P = e(B * Tc, 2 * C, dtype=F32)  # conv_cond(c) + its bias, one row per conditioning frame
            _fwd(cc, c_low, w_cc, P, Tc, bias=ts[cc.at + 1])
            seg = dict(rowbias=P, rowbias_T=Tc if Tc > 1 else 0)
        u, g, mr = e(N, 2 * C, dtype=dt), e(N, C, dtype=dt), e(B, 2, 2, dtype=F32)
        if lens is not None:  # statistics and apply over each utterance's own rows; g gets a zero tail
            _fwd(ci, cur, w_in, u, T, bias=ts[ci.at + 1], **seg)
            ops.groupnorm_stats_len(u, T, 2, lens, gn_part, mr)
            ops.gn_glu_fwd_len(u, g, T, lens, mr, ts[ag], ts[ag + 1])
        elif T % 128 == 0 and C % 128 == 0:  # GroupNorm statistics from the GEMM's epilogue tiles
            gst = e((N // 128) * (2 * C // 128) * 4, dtype=F32)
            _fwd(ci, cur, w_in, u, T, bias=ts[ci.at + 1], gn_stats=gst, gn_groups=2, **seg)
            ops.gn_glu_fwd_tiles(u, g, T, gst, mr, ts[ag], ts[ag + 1])
        else:
            _fwd(ci, cur, w_in, u, T, bias=ts[ci.at + 1], **seg)
            ops.groupnorm_stats(u, T, 2, gn_part, mr)
            ops.gn_glu_fwd(u, g, T, mr, ts[ag], ts[ag + 1])
        y = e(N, C, dtype=dt)
        _fwd(rs, g, w_rs, y, T, bias=ts[rs.at + 1], res=cur, out2=skip32, split_col=C, out2_accumulate=not first)
        if lens is not None:  # the residual is the next conv_in's operand; its tail holds the bias
            ops.mask_tail(y, T, lens)
        first = False
        saved.append((cur, u, g, mr))
        cur = y
    a_skip, f1 = e(N, plan.S, dtype=dt), e(N, plan.fin1.cout, dtype=dt)
    xhat = e(N, plan.final, dtype=F32)
    ops.scale_act_2d(skip32, a_skip, plan.scale, L.PRO_RELU)
    w1, w2 = _pack(ts[plan.fin1.at], False, dt), _pack(ts[plan.fin2.at], False, dt)
    if lens is not None and plan.fin1.k > 1:
        ops.mask_tail(a_skip, T, lens)
    _fwd(plan.fin1, a_skip, w1, f1, T, bias=ts[plan.fin1.at + 1], act=L.PRO_RELU)
    if lens is not None and plan.fin2.k > 1:
        ops.mask_tail(f1, T, lens)
    _fwd(plan.fin2, f1, w2, xhat, T, bias=ts[plan.fin2.at + 1], out_f32=True)
    if lens is not None:
        ops.mask_tail(xhat, T, lens)
    return xhat, (Tc, c_low, saved, wp, a_skip, f1, w1, w2)


def _decoder_rows_bwd(plan, B, T, Tc, keep, dxhat):
    """The decoder's backward launches on frame-major operands: `keep` =
    (saved, wp, a_skip, f1, c_low, ts) as _decoder_rows left them (wp with the
    final convs' packed weights added), dxhat [B*T, final] the output gradient
    in the compute dtype.  Returns (dx f32 [B*T, C_in], dc f32 [B*Tc, cond] the
    gradient of c_low or None for an unconditioned plan, grads: dL/d(ts) in the
    plan's order)."""
    saved, wp, a_skip, f1, c_low, ts = keep
    dev, dt, S = dxhat.device, plan.dt, plan.S
    N = B * T
    e = functools.partial(torch.empty, device=dev)
    grads = [None] * plan.n_tensors
    Cmax = max(st[1].cin for st in plan.steps if st[0] == "block")
    cs_part = e(64 * max(2 * Cmax, Cmax + S, plan.final, plan.cond, 1024), dtype=F32)
    gnb_part = e(B * 64 * 2, dtype=F32)
    # final layer: ReLU, conv, ReLU, conv on scale * sum(skips)
    f1c, f2c = plan.fin1, plan.fin2
    grads[f2c.at + 1] = _colsum(dxhat, cs_part)
    grads[f2c.at] = _wgrad(f2c, dxhat, f1, T)
    df1 = e(N, f2c.cin, dtype=dt)
    _dgrad(f2c, dxhat, wp[f2c.at], df1, T, mask=f1, mask_slope=0.0)
    grads[f1c.at + 1] = _colsum(df1, cs_part)
    grads[f1c.at] = _wgrad(f1c, df1, a_skip, T)
    # dr: [dL/dx | dL/dskip] of the current block's output, two buffers per width in turn
    bufs = {}

    def dr(C, k):
        if (C, k) not in bufs:
            bufs[(C, k)] = e(N, C + S, dtype=dt)
            if (C, k) != first_key:
                ops.convert_2d(bufs[first_key][:, first_key[0]:], bufs[(C, k)][:, C:])
        return bufs[(C, k)]

    C_last = plan.steps[-1][1].cin
    first_key = (C_last, 0)
    cur = dr(C_last, 0)
    _dgrad(f1c, df1, wp[f1c.at], cur[:, C_last:], T, mask=a_skip, mask_slope=0.0, mask_scale=plan.scale)
    ops.convert_2d(None, cur, cols=C_last)  # dL/dx at the decoder output is 0: the last residual is unused
    k, dc, dx = 0, None, None
    for st, sv in zip(reversed(plan.steps), reversed(saved)):
        if st[0] == "conv":
            cv = st[1]
            cur_x = cur[:, :cv.cout]
            grads[cv.at + 1] = _colsum(cur_x, cs_part)
            grads[cv.at] = _wgrad(cv, cur_x, sv[0], T)
            if sv[0] is saved[0][0]:  # the decoder input
                dx = e(N, cv.cin, dtype=F32)
                _dgrad(cv, cur_x, wp[cv.at], dx, T, out_f32=True)
            else:
                k ^= 1
                nxt = dr(cv.cin, k)
                _dgrad(cv, cur_x, wp[cv.at], nxt[:, :cv.cin], T)
                cur = nxt
            continue
        _, ci, cc, rs, ag = st
        xin, u, g, mr = sv
        C = ci.cin
        grads[rs.at + 1] = _colsum(cur, cs_part)
        grads[rs.at] = _wgrad(rs, cur, g, T)
        dg, du = e(N, C, dtype=dt), e(N, 2 * C, dtype=dt)
        _dgrad(rs, cur, wp[rs.at], dg, T)
        cs_b, dgam_b, dbet_b = (e(B, 2 * C, dtype=F32) for _ in range(3))
        ops.gn_bwd(dg, u, du, T, 2, True, mr, ts[ag], ts[ag + 1], gnb_part, cs_b, dgam_b, dbet_b)
        grads[ci.at + 1] = _colsum(cs_b, cs_part)
        grads[ag], grads[ag + 1] = _colsum(dgam_b, cs_part), _colsum(dbet_b, cs_part)
        # conditioning: dP = the per-segment sums of du, then conv_cond's own gradients at the low rate
        if cc is not None:
            if Tc == 1:
                dP = cs_b
            else:
                dP = e(B * Tc, 2 * C, dtype=F32)
                ops.upsample_cat_bwd([dP], B, T, du)
            grads[cc.at + 1] = grads[ci.at + 1] if Tc == 1 else _colsum(dP, cs_part)
            grads[cc.at] = _wgrad(cc, dP, c_low, Tc)
            dc_new = e(B * Tc, plan.cond, dtype=F32)
            _dgrad(cc, dP, wp[cc.at], dc_new, Tc, **({} if dc is None else dict(res=dc)))
            dc = dc_new
        grads[ci.at] = _wgrad(ci, du, xin, T)
        k ^= 1
        nxt = dr(C, k)
        _dgrad(ci, du, wp[ci.at], nxt[:, :C], T, res=cur[:, :C])
        cur = nxt
    return dx, dc, grads


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, save, T_levels, x, *rest):
        nl = max(1, len(T_levels)) if plan.cond else 0
        cin, ts = rest[:nl], rest[nl:]
        if not x.is_cuda or not all(t.is_cuda for t in rest):
            raise L.VqxError("vqvae2.Decoder runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
        B, _, T = x.shape
        ts = [t.detach().float() for t in ts]
        rows = [_to_rows(z) for z in cin] if plan.cond else None
        x2 = torch.empty(B * T, x.shape[1], device=x.device, dtype=plan.dt)
        ops.nct_to_ntc(x.float().contiguous(), x2)
        xhat, (Tc, c_low, saved, wp, a_skip, f1, w1, w2) = _decoder_rows(plan, x2, B, T, rows, T_levels, ts)
        if save:
            wp[plan.fin1.at], wp[plan.fin2.at] = w1, w2
            ctx.plan, ctx.dims, ctx.T_levels, ctx.Tc = plan, (B, T), T_levels, Tc
            ctx.level_shapes = [tuple(z.shape) for z in cin]
            ctx.keep = (saved, wp, a_skip, f1, c_low, ts)
        return _to_nct(xhat, B, T)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        plan, (B, T), Tc = ctx.plan, ctx.dims, ctx.Tc
        dxhat = torch.empty(B * T, plan.final, device=dout.device, dtype=plan.dt)
        ops.nct_to_ntc(dout.float().contiguous(), dxhat)
        dx, dc, grads = _decoder_rows_bwd(plan, B, T, Tc, ctx.keep, dxhat)
        e = functools.partial(torch.empty, device=dout.device)
        # the conditioning's gradient back to the levels (or to the tensor c)
        if dc is None:
            dcin = []
        elif ctx.T_levels:
            dl = [e(B * Tl, Cl, dtype=F32) for _, Cl, Tl in ctx.level_shapes]
            ops.upsample_cat_bwd(dl, B, Tc, dc)
            dcin = [_to_nct(d, B, s[2]) for d, s in zip(dl, ctx.level_shapes)]
        else:
            dcin = [_to_nct(dc, B, T)]
        ctx.keep = None
        return (None, None, None, _to_nct(dx, B, T), *dcin, *grads)


class Decoder(_Decoder):
    """vqvae2.py:274-371 with `compute_dtype: fp32|bf16`; forward((x, c)) with c a
    (B, cond, T) tensor or a list of levels (B, C_l, T_l), sum C_l == cond.
    With cond_channels 0 / None the blocks own no conv_cond (layers.py:209-212)
    and the call is forward((x, None)): no row bias in the conv_in GEMMs, no
    conv_cond launches or gradients.  A conditioning given to such a decoder, or
    None given to a conditioned one, is a ValueError."""

    def __init__(self, *args, compute_dtype="fp32", **kw):
        scales = kw.get("upsample_scales", args[2] if len(args) > 2 else (1, 1, 1, 1))
        if any(s != 1 for s in scales):
            raise NotImplementedError(f"vqvae2.Decoder: upsample_scales {list(scales)}: resampling stages are not "
                                      "built for the hierarchical decoder (the vae2 recipe has none)")
        if compute_dtype not in _DT:
            raise ValueError(f"compute_dtype {compute_dtype!r} is not fp32 or bf16")
        super().__init__(*args, **kw)
        self.compute_dtype = compute_dtype
        self._plan = None

    def forward(self, input):
        x, c = input
        if x.dim() != 3:
            raise ValueError(f"vqvae2.Decoder: x {tuple(x.shape)} is not (B, C, T)")
        B, _, T = x.shape
        if not self.cond_ch:  # unconditioned (cond_channels 0 / None): forward((x, None))
            if c is not None:
                raise ValueError("vqvae2.Decoder: this decoder is unconditioned (cond_channels 0); it takes (x, None) "
                                 "and would ignore the conditioning it was given")
            if self._plan is None:
                self._plan = _Plan(self)
            ts = _Plan.tensors(self)
            save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, *ts))
            return _DecoderFn.apply(self._plan, save, (), x, *ts)
        if c is None:
            raise ValueError(f"vqvae2.Decoder: the conditioning is None, this decoder has cond_channels {self.cond_ch}")
        levels = [c] if torch.is_tensor(c) else list(c)
        if not levels or any(z.dim() != 3 or z.shape[0] != B for z in levels) \
                or sum(z.shape[1] for z in levels) != self.cond_ch:
            raise ValueError(f"vqvae2.Decoder: the conditioning must be (B, C_l, T_l) levels with sum C_l == "
                             f"{self.cond_ch}")
        if torch.is_tensor(c):
            if c.shape[2] != T:
                raise ValueError(f"vqvae2.Decoder: a tensor c must have x's {T} frames, got {c.shape[2]}")
            T_levels = ()
        else:
            T_levels = tuple(z.shape[2] for z in levels)
            for Tl in T_levels:
                src_index(T, Tl)
        if self._plan is None:
            self._plan = _Plan(self)
        ts = _Plan.tensors(self)
        save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, *levels, *ts))
        return _DecoderFn.apply(self._plan, save, T_levels, x, *levels, *ts)

    def forward_rows(self, x_rows, B, T, cond_rows, lengths=None):
        """forward without gradients on frame-major operands: x_rows [B*T, C] in
        the compute dtype (as vqx_codes_upsample_cat writes it) in place of
        (B, C, T), so the first layout change is skipped; cond_rows the
        conditioning levels as f32 [B*T_l, C_l] rows.  Returns xhat f32
        [B*T, final] rows.  Nothing is kept for a backward.  lengths: host
        ints, utterance b owns rows t < lengths[b] (x_rows zero elsewhere, the
        conditioning one row per utterance or full rate; _decoder_rows)."""
        if lengths is not None:
            lengths = ops.len_array(lengths, B, "vqvae2.Decoder lengths")
            if any(not 1 <= n <= T for n in lengths):
                raise ValueError(f"vqvae2.Decoder: lengths must lie in 1..T = {T}")
        if self._plan is None:
            self._plan = _Plan(self)
        plan = self._plan
        if not x_rows.is_cuda or x_rows.dim() != 2 or x_rows.dtype != plan.dt or x_rows.stride(1) != 1 \
                or x_rows.shape[0] != B * T:
            raise ValueError(f"vqvae2.Decoder: x_rows must be device [{B * T}, C] rows in {plan.dt}")
        if not self.cond_ch:
            if cond_rows is not None:
                raise ValueError("vqvae2.Decoder: this decoder is unconditioned (cond_channels 0); cond_rows must be None")
            with torch.no_grad():
                ts = [t.detach().float() for t in _Plan.tensors(self)]
                return _decoder_rows(plan, x_rows, B, T, None, (), ts, lengths)[0]
        if cond_rows is None or any(r.dim() != 2 or r.dtype != F32 or r.shape[0] % B for r in cond_rows) \
                or sum(r.shape[1] for r in cond_rows) != self.cond_ch:
            raise ValueError(f"vqvae2.Decoder: the conditioning must be f32 [B*T_l, C_l] rows with sum C_l == "
                             f"{self.cond_ch}")
        T_levels = tuple(r.shape[0] // B for r in cond_rows)
        for Tl in T_levels:
            src_index(T, Tl)
        with torch.no_grad():
            ts = [t.detach().float() for t in _Plan.tensors(self)]
            if lengths is not None and T_levels == (T,):
                T_levels = ()  # already at full rate: read in place
            return _decoder_rows(plan, x_rows, B, T, list(cond_rows), T_levels, ts, lengths)[0]


# ------------------------------------------------------------------ encoder
class _EConv:
    """One encoder conv of the plan.  Three slots of the flat tensor list from
    `at`: a stride-1 conv (scale 1) takes (effective weight, bias, None) and
    returns dL/dw in torch's layout; a strided stage conv (scale s, run folded as
    model/resample.py does) takes (weight_v | weight, bias, weight_g | None) and
    returns the parameter gradients of its own weight-norm table."""

    def __init__(self, mod, at):
        self.mod, self.at = mod, at
        self.cin, self.cout, self.k = mod.cin, mod.cout, mod.k
        self.scale = getattr(mod, "scale", 1)
        self.transposed = False
        if self.scale == 1:
            self.dil, self.pad = mod.dilation, mod.padding
            if 2 * self.pad != (mod.k - 1) * mod.dilation:
                raise NotImplementedError("asymmetric padding (the output length would change)")

    def tensors(self):
        m = self.mod
        if self.scale == 1:
            return [m.effective_weight(), m.bias, None]
        return [m.v_param, m.bias, m.g_param]


class _EncPlan:
    """Static description of an Encoder for _EncoderFn (no tensors): per stage
    its conv and blocks; a block = (stack convs, first GroupNorm slots, skip conv)."""

    def __init__(self, enc):
        self.dt = _DT[enc.compute_dtype]
        layers, self.stages, at = list(enc.encode), [], 0
        bounds = list(enc.stage_index) + [len(layers)]
        for lo, hi in zip(bounds, bounds[1:]):
            conv = _EConv(layers[lo], at)
            at += 3
            blocks = []
            for blk in layers[lo + 1:hi - 1]:  # the stage ends with its LeakyReLU
                convs, gn_at = [], []
                for cv, gn in zip(blk.convs, blk.norms):
                    convs.append(_EConv(cv, at))
                    convs[-1].norm = gn
                    gn_at.append(at + 3)
                    at += 5
                blocks.append((convs, gn_at, _EConv(blk.skip_layer, at)))
                at += 3
            self.stages.append((conv, blocks))
        self.z_proj = _EConv(enc.z_proj, at)
        self.n_tensors = at + 3
        self.total_scale = math.prod(cv.scale for cv, _ in self.stages)

    @staticmethod
    def tensors(enc, plan):
        out = []
        for conv, blocks in plan.stages:
            out += conv.tensors()
            for convs, _, skip in blocks:
                for cv in convs:
                    out += cv.tensors() + [cv.norm.weight, cv.norm.bias]
                out += skip.tensors()
        return out + plan.z_proj.tensors()


def _down_splits(cv, n, T, dt):
    tiles = ops.wgrad_tiles(n, T, cv.cout, cv.scale * cv.cin, 3, 1, ops.dt_code(dt))
    return max(1, min(512 // max(1, tiles), n // 512))


def _stage_frames(T_in, s):
    """Output frames of a stage conv (kernel 2s, stride s, padding s//2 + s%2) on T_in frames."""
    return T_in if s == 1 else (T_in + 2 * (s // 2 + s % 2) - 2 * s) // s + 1


def _total_scale(enc):
    """Total down-sampling of an Encoder: the product of its stage convs' strides."""
    return math.prod(getattr(enc.encode[i], "scale", 1) for i in enc.stage_index)


def _encoder_rows(plan, inp, B, T, ts, ragged=False, lengths=None):
    """The encoder's forward launches on the frame-major input `inp` [B*T, C_in]
    in the compute dtype.  Returns z f32 [B*T', z], feat [B*T', C] (the last
    stage's LeakyReLU, compute dtype), T', and what the backward reads (saved, wp).

    ragged (B == 1, nothing kept for a backward): a stage conv whose input length
    J*s + r, 0 < r < s, is no multiple of its stride runs on the input zero-padded
    to (J+1)*s rows, as J+1 folded frames, and its first floor((T_in + 2p - 2s)/s)
    + 1 output rows are kept (J for an even s).  Every kept row reads real frames
    or zeros where the strided conv reads its own padding, so this is exact; the
    layers after it see the kept rows alone.

    lengths (any B, nothing kept for a backward): utterance b owns rows
    t < lengths[b] of the padded T, a multiple of the total stride, and `inp`
    holds zeros in the other rows.  A stage keeps _stage_frames(len, s) frames
    per utterance: the zero tail gives a partial last group the zeros the
    strided conv reads from its own padding (the argument above, for every
    utterance).  The GroupNorm statistics run over the valid rows (the *_len
    kernels, never the GEMM tiles) and every LeakyReLU output a 3-tap conv reads
    is given a zero tail (ops.mask_tail).  z and feat keep the padded T'; the
    tail rows of z are not defined."""
    dev, dt = inp.device, plan.dt
    e = functools.partial(torch.empty, device=dev)
    gn_part = e(B * 2 * 24, dtype=F32)
    wp, saved, T_in = {}, [], T
    lens = None if lengths is None else list(ops.len_array(lengths, B, "vqvae2.Encoder lengths"))
    if lens is not None and T % plan.total_scale:
        raise ValueError(f"vqvae2.Encoder: with lengths the padded T = {T} must be a multiple of {plan.total_scale}")
    for conv, blocks in plan.stages:
        s, C = conv.scale, conv.cout
        Ts = T_in // s
        N = B * Ts
        # every GEMM producing c_j also writes a_j = LeakyReLU(c_j), the operand of the
        # next conv stack / stage conv / z_proj (vqvae2.py:224, layers.py:152)
        if s == 1:
            c, a = e(N, C, dtype=dt), e(N, C, dtype=dt)
            w = wp[conv.at] = _pack(ts[conv.at], False, dt)
            _fwd(conv, inp, w, c, T_in, bias=ts[conv.at + 1], act=L.PRO_LRELU, y2=a)
        else:  # folded: s frames of cin channels as one frame of s*cin, 3 taps
            w, norm = e(C, 3 * s * conv.cin, dtype=dt), e(C, dtype=F32)
            ops.weight_norm_fwd(conv.mod._table(w, norm))
            wp[conv.at] = (w, norm)
            Tf = Ts  # folded frames the GEMM runs on
            if T_in % s:
                if not (ragged and B == 1):
                    raise ValueError(f"vqvae2.Encoder: a stage of {T_in} frames is not a multiple of its stride {s}")
                Tf, Ts = Ts + 1, _stage_frames(T_in, s)
                if Ts < 1:
                    raise ValueError(f"vqvae2.Encoder: T = {T} leaves a stage without a frame")
                N = Ts
                padded = e(Tf * s, conv.cin, dtype=dt)
                ops.convert_2d(inp, padded, rows=T_in)
                ops.zero_(padded[T_in:])
                inp = padded
            c, a = e(B * Tf, C, dtype=dt), e(B * Tf, C, dtype=dt)
            ops.conv_fwd(inp.view(B * Tf, s * conv.cin), w, c, T=Tf, cin=s * conv.cin, cout=C, ntaps=3, pad=1,
                         bias=ts[conv.at + 1], act=L.PRO_LRELU, y2=a)
            c, a = c[:N], a[:N]
        if lens is not None:
            lens = [_stage_frames(n, s) for n in lens]
            ops.mask_tail(a, Ts, lens)
        # GroupNorm statistics from the GEMM's epilogue tiles
        fuse = lens is None and Ts % 128 == 0 and C % 128 == 0
        cs, acts, per_block = [c], [a], []
        for convs, gn_at, skip in blocks:
            src, hs, mrs, gs, gkw = acts[-1], [], [], [], {}
            for l, (cv, ag) in enumerate(zip(convs, gn_at)):
                last = l == len(convs) - 1
                w = wp[cv.at] = _pack(ts[cv.at], False, dt)
                h, mr = e(N, C, dtype=dt), e(B, 2, dtype=F32)
                if fuse:
                    gst = e((N // 128) * (C // 128) * 4, dtype=F32)
                    _fwd(cv, src, w, h, Ts, bias=ts[cv.at + 1], gn_stats=gst, gn_groups=1)
                    if last:
                        gkw = dict(gn_tiles=gst)  # merged inside the skip GEMM
                    else:
                        ops.gn_finalize_tiles(gst, N, Ts, C, 1, mr)
                elif lens is not None:
                    _fwd(cv, src, w, h, Ts, bias=ts[cv.at + 1])
                    ops.groupnorm_stats_len(h, Ts, 1, lens, gn_part, mr)
                else:
                    _fwd(cv, src, w, h, Ts, bias=ts[cv.at + 1])
                    ops.groupnorm_stats(h, Ts, 1, gn_part, mr)
                if not last:  # LeakyReLU(GN(h)): the next conv's operand (layers.py:156-161)
                    g = e(N, C, dtype=dt)
                    if lens is not None:
                        ops.gn_lrelu_fwd_len(h, g, Ts, lens, mr, ts[ag], ts[ag + 1])
                    else:
                        ops.gn_lrelu_fwd(h, g, Ts, mr, ts[ag], ts[ag + 1])
                    gs.append(g)
                    src = g
                hs.append(h)
                mrs.append(mr)
            w = wp[skip.at] = _pack(ts[skip.at], False, dt)
            c, a = e(N, C, dtype=dt), e(N, C, dtype=dt)
            _fwd(skip, cs[-1], w, c, Ts, bias=ts[skip.at + 1], gn_h=hs[-1], gn_mr=mrs[-1], gn_gamma=ts[gn_at[-1]],
                 gn_beta=ts[gn_at[-1] + 1], act=L.PRO_LRELU, y2=a, **gkw)
            if lens is not None:
                ops.mask_tail(a, Ts, lens)
                if skip.k > 1:
                    ops.mask_tail(c, Ts, lens)
            cs.append(c)
            acts.append(a)
            per_block.append((hs, mrs, gs))
        saved.append((inp, T_in, Ts, cs, acts, per_block))
        inp, T_in = acts[-1], Ts
    zp = plan.z_proj
    w = wp[zp.at] = _pack(ts[zp.at], False, dt)
    z = e(B * T_in, zp.cout, dtype=F32)
    _fwd(zp, inp, w, z, T_in, bias=ts[zp.at + 1], out_f32=True)
    return z, inp, T_in, saved, wp


class _EncoderFn(torch.autograd.Function):
    """engine/step.py encoder_fwd / encoder_bwd composed from ops.*, with the
    second output `feat` = the last stage's LeakyReLU and a gradient into it."""

    @staticmethod
    def forward(ctx, plan, save, x, *ts):
        if not x.is_cuda or not all(t.is_cuda for t in ts if t is not None):
            raise L.VqxError("vqvae2.Encoder runs on the MI355X only (libvqx); move it and its input with .cuda()")
        B, _, T = x.shape
        ts = [None if t is None else t.detach().float() for t in ts]
        inp = ops.nct_to_ntc(x.float().contiguous(), torch.empty(B * T, x.shape[1], device=x.device, dtype=plan.dt))
        z, feat, T_out, saved, wp = _encoder_rows(plan, inp, B, T, ts)
        ctx.set_materialize_grads(False)
        if save:
            ctx.plan, ctx.B = plan, B
            ctx.keep = (saved, wp, ts)
        return _to_nct(z, B, T_out), _to_nct(feat, B, T_out)

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, dfeat):
        plan, B = ctx.plan, ctx.B
        saved, wp, ts = ctx.keep
        ctx.keep = None
        grads = [None] * plan.n_tensors
        if dz is None and dfeat is None:
            return (None, None, None, *grads)
        dev, dt = (dz if dz is not None else dfeat).device, plan.dt
        e = functools.partial(torch.empty, device=dev)
        Cmax = max(conv.cout for conv, _ in plan.stages)
        cs_part = e(64 * max(Cmax, plan.z_proj.cout, 1024), dtype=F32)
        gnb_part = e(B * 64 * 2, dtype=F32)
        # the gradient at the last activation a: lrelu'(a) * (W_proj^T dz + dfeat).  The GEMM
        # epilogue applies MASK before RES, so dfeat arrives already masked (vqx_nct_to_ntc_lrelu_bwd)
        _, _, Ts, _, acts, _ = saved[-1]
        a_last, N = acts[-1], B * Ts
        masked = None
        if dfeat is not None:
            masked = ops.nct_to_ntc_lrelu_bwd(dfeat.float().contiguous(), a_last, 0.2, e(N, a_last.shape[1], dtype=dt))
        if dz is not None:
            zp = plan.z_proj
            dzr = ops.nct_to_ntc(dz.float().contiguous(), e(N, zp.cout, dtype=dt))
            grads[zp.at + 1] = _colsum(dzr, cs_part)
            grads[zp.at] = _wgrad(zp, dzr, a_last, Ts)
            cur = e(N, zp.cin, dtype=dt)
            _dgrad(zp, dzr, wp[zp.at], cur, Ts, mask=a_last, mask_slope=0.2,
                   **({} if masked is None else dict(res=masked)))
        else:
            cur = masked
        dx = None
        for si in reversed(range(len(plan.stages))):
            conv, blocks = plan.stages[si]
            inp, T_in, Ts, cs, acts, per_block = saved[si]
            N, C = B * Ts, conv.cout
            for j in reversed(range(len(blocks))):
                convs, gn_at, skip = blocks[j]
                hs, mrs, gs = per_block[j]
                # cur = dL/dc_{j+1}, the gradient w.r.t. block j's output GN(h_L) + skip(c_j)
                dy, tmp = cur, None
                for l in reversed(range(len(convs))):
                    cv, ag = convs[l], gn_at[l]
                    dh = e(N, C, dtype=dt)
                    cs_b, dgam_b, dbet_b = (e(B, C, dtype=F32) for _ in range(3))
                    ops.gn_bwd(dy, hs[l], dh, Ts, 1, False, mrs[l], ts[ag], ts[ag + 1], gnb_part, cs_b, dgam_b, dbet_b)
                    grads[cv.at + 1] = _colsum(cs_b, cs_part)
                    grads[ag], grads[ag + 1] = _colsum(dgam_b, cs_part), _colsum(dbet_b, cs_part)
                    src = acts[j] if l == 0 else gs[l - 1]
                    grads[cv.at] = _wgrad(cv, dh, src, Ts)
                    # into LeakyReLU(.): its derivative from the sign of the stored output
                    dy = tmp = e(N, C, dtype=dt)
                    _dgrad(cv, dh, wp[cv.at], dy, Ts, mask=src, mask_slope=0.2)
                # the skip conv last, adding the stack's data gradient
                grads[skip.at + 1] = _colsum(cur, cs_part)
                grads[skip.at] = _wgrad(skip, cur, cs[j], Ts)
                nxt = e(N, C, dtype=dt)
                _dgrad(skip, cur, wp[skip.at], nxt, Ts, res=tmp)
                cur = nxt
            # cur = dL/dc_0 of the stage (the stage conv's output)
            grads[conv.at + 1] = _colsum(cur, cs_part)
            want_dx = si > 0 or ctx.needs_input_grad[2]
            prev_a = saved[si - 1][4][-1] if si > 0 else None
            mask = {} if si == 0 else dict(mask=prev_a, mask_slope=0.2)
            s = conv.scale
            if s == 1:
                grads[conv.at] = _wgrad(conv, cur, inp, T_in)
                if want_dx:
                    nxt = e(B * T_in, conv.cin, dtype=dt if si else F32)
                    _dgrad(conv, cur, wp[conv.at], nxt, T_in, **(mask if si else dict(out_f32=True)))
            else:
                w, norm = wp[conv.at]
                fold = s * conv.cin
                splits = _down_splits(conv, N, Ts, dt)
                slabs = e(splits, C, 3 * fold, dtype=F32)
                ops.conv_wgrad(cur, inp.view(N, fold), slabs, T=Ts, r_dim=C, c_dim=fold, ntaps=3, pad=1, shift_sign=1,
                               splits=splits)
                dv = torch.empty_like(ts[conv.at])
                dg = torch.empty_like(ts[conv.at + 2]) if ts[conv.at + 2] is not None else None
                ops.weight_norm_bwd(conv.mod._table(w, norm, dv=dv, dg=dg, slabs=slabs, splits=splits))
                grads[conv.at], grads[conv.at + 2] = dv, dg
                if want_dx:
                    nxt = e(B * T_in, conv.cin, dtype=dt if si else F32)
                    if si:
                        mask = dict(mask=prev_a.view(N, fold), mask_slope=0.2)
                    ops.conv_dgrad(cur, w, nxt.view(N, fold), T=Ts, cin=C, cout=fold, ntaps=3, pad=1,
                                   **(mask if si else dict(out_f32=True)))
            if si:
                cur = nxt
            elif want_dx:
                dx = _to_nct(nxt, B, T_in)
        return (None, None, dx, *grads)


class Encoder(_Encoder):
    """vqvae2.py:175-271 with `compute_dtype: fp32|bf16`: forward(x (B, C_in, T))
    -> (z, feat), z = z_proj(feat) (B, z_channels, T'), feat the last stage's
    LeakyReLU output (B, out_channels[-1], T'), T' = T / prod(downsample_scales).
    The reference's module tree: `encode` (without the projection) and `z_proj`."""

    def __init__(self, *args, compute_dtype="fp32", **kw):
        if compute_dtype not in _DT:
            raise ValueError(f"compute_dtype {compute_dtype!r} is not fp32 or bf16")
        super().__init__(*args, **kw)
        layers = list(self.encode)
        self.encode = nn.Sequential(*layers[:-1])
        self.z_proj = layers[-1]
        self.compute_dtype = compute_dtype
        self._plan = None

    def forward(self, x):
        if x.dim() != 3 or x.shape[1] != self.in_ch:
            raise ValueError(f"vqvae2.Encoder: x {tuple(x.shape)} is not (B, {self.in_ch}, T)")
        if self._plan is None:
            self._plan = _EncPlan(self)
        plan = self._plan
        if x.shape[2] % plan.total_scale:
            raise ValueError(f"vqvae2.Encoder: T = {x.shape[2]} is not a multiple of the down-sampling "
                             f"{plan.total_scale}")
        ts = _EncPlan.tensors(self, plan)
        save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, *ts) if t is not None)
        return _EncoderFn.apply(plan, save, x, *ts)

    def forward_rows(self, x_rows, B, T, lengths=None):
        """forward without gradients on the frame-major input x_rows [B*T, C_in]
        in the compute dtype: (z f32 [B*T', z_channels] rows, feat [B*T', C]
        rows in the compute dtype, T').  One utterance (B == 1) may have any
        length that leaves every stage a frame (_encoder_rows states the
        ragged stages); forward itself keeps refusing such a T.  lengths: host
        ints, utterance b owns rows t < lengths[b] of a padded T that is a
        multiple of the down-sampling; x_rows holds zeros elsewhere
        (_encoder_rows)."""
        if self._plan is None:
            self._plan = _EncPlan(self)
        plan = self._plan
        if not x_rows.is_cuda or x_rows.dim() != 2 or x_rows.dtype != plan.dt or x_rows.stride(1) != 1 \
                or tuple(x_rows.shape) != (B * T, self.in_ch):
            raise ValueError(f"vqvae2.Encoder: x_rows must be device [{B * T}, {self.in_ch}] rows in {plan.dt}")
        if lengths is not None:
            lens = list(ops.len_array(lengths, B, "vqvae2.Encoder lengths"))
            if any(not 1 <= n <= T for n in lens):
                raise ValueError(f"vqvae2.Encoder: lengths must lie in 1..T = {T}")
            for conv, _ in plan.stages:
                lens = [_stage_frames(n, conv.scale) for n in lens]
                if min(lens) < 1:
                    raise ValueError(f"vqvae2.Encoder: an utterance of {lengths[lens.index(min(lens))]} frames leaves a "
                                     "stage without a frame")
            with torch.no_grad():
                ts = [None if t is None else t.detach().float() for t in _EncPlan.tensors(self, plan)]
                return _encoder_rows(plan, x_rows, B, T, ts, lengths=lengths)[:3]
        ragged, T_in = False, T
        for conv, _ in plan.stages:
            ragged |= T_in % conv.scale != 0
            T_in = _stage_frames(T_in, conv.scale)
            if T_in < 1:
                raise ValueError(f"vqvae2.Encoder: T = {T} leaves a stage without a frame")
        if ragged and B != 1:
            raise ValueError(f"vqvae2.Encoder: T = {T} is not a multiple of every stage's stride; such lengths are "
                             f"converted one utterance at a time (B == 1), got B = {B}")
        with torch.no_grad():
            ts = [None if t is None else t.detach().float() for t in _EncPlan.tensors(self, plan)]
            return _encoder_rows(plan, x_rows, B, T, ts, ragged=ragged)[:3]


# ------------------------------------------------------------------ model
class _LogLossFn(torch.autograd.Function):
    """log_loss(xhat, x) (layers.py:283-296, 'frame_mean') as vqx_logloss_fwd_bwd:
    the launch that sums the loss also writes d loss / d xhat; the backward is
    its layout change with the upstream gradient folded in (vqx_ntc_to_nct_scale)."""

    @staticmethod
    def forward(ctx, xhat, x):
        B, C, T = x.shape
        rows = _to_rows(xhat)
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


class Model(nn.Module):
    """The reference's hierarchical `Model` (vqvae2.py:11-172) for
    `model_type: vae_npvc_amd.model.vqvae2`: `Model(arch)` with the keys levels,
    use_gst, use_ema, beta, y_num, y_dim, jitter_p, encoder.{i}, decoder.{i},
    quantizer.{i} (+ compute_dtype: fp32|bf16), the reference's module tree
    (encoders, quantizers, decoders, embeds, jitter) and state_dict keys.

    forward((x, y_idx)) restates vqvae2.py:74-127 as a composition of the HIP
    modules under torch autograd, so the reference's trainer (model(input),
    loss.backward(), a stock optimizer) runs it unchanged.  No stretched tensor
    is built for conditioning: each decoder receives its low-rate levels as a
    list; only the input of decoders[0] goes through upsample_cat.  The loss
    dict comes from one readback of the packed scalars at the end.

    Conversion: analyze(x) -> the codes forward picks, synthesize((codes, y))
    -> xhat from codes, convert((x, y)) = the two together = the xhat of
    forward((x, y)).  All three run without gradients and write no parameter
    or buffer; one utterance at a time may have any length, and so may the
    utterances of a padded batch given with its `lengths`.

    Not built (NotImplementedError): use_ema: true (EMAVectorQuantizer.forward
    inside the hierarchy), jitter_p != 0, and encode / decode / infer, whose
    reference versions refer to members the class does not have."""

    def __init__(self, arch):
        super().__init__()
        levels = arch.get("levels", 3)
        use_gst = arch.get("use_gst", True)
        use_ema = arch.get("use_ema", True)
        jitter_p = arch.get("jitter_p", 0.0)
        if use_ema and (levels > 1 or not use_gst):
            raise NotImplementedError("vqvae2.Model: use_ema: true needs EMAVectorQuantizer.forward, which is not "
                                      "built for the hierarchical model; set use_ema: false (the vae2 recipe's value)")
        if jitter_p != 0:
            raise NotImplementedError(f"vqvae2.Model: jitter_p {jitter_p} is not built for the hierarchical model "
                                      "(the vae2 recipe uses 0)")
        dtype = arch.get("compute_dtype", "fp32")
        encoders, quantizers, decoders = [], [], []
        for i in range(levels):
            encoders.append(Encoder(**arch[f"encoder.{i}"], compute_dtype=dtype))
            decoders.append(Decoder(**arch[f"decoder.{i}"], compute_dtype=dtype))
            Quantizer = StyleTokenLayer if use_gst and i == levels - 1 else VectorQuantizer
            quantizers.append(Quantizer(**arch[f"quantizer.{i}"]))
        self.encoders = nn.ModuleList(encoders)
        self.quantizers = nn.ModuleList(quantizers)
        self.decoders = nn.ModuleList(decoders)
        self.embeds = Conditions(arch.get("y_num", 10), arch.get("y_dim", 128), normalize=False)
        self.jitter = Jitter(probability=jitter_p)
        self.beta = arch.get("beta", 0.01)
        self.levels, self.use_gst, self.use_ema = levels, use_gst, use_ema
        self.compute_dtype = dtype
        self._engine = None

    def engine(self, device=None):
        """The optimizer engine of this package's Trainer (engine/autograd_step.py:
        flat parameters and moments, multi-tensor clip + Adam / RAdam), built
        once per device and rebuilt when the parameters were moved."""
        dev = device if device is not None else next(self.parameters()).device
        dev = torch.device(dev)
        if dev.type != "cuda":
            raise RuntimeError("vqvae2.Model runs on the MI355X only (libvqx); move it with .cuda()")
        e = self._engine
        if e is None or e.device != dev or not e.params_intact():
            from ..engine.autograd_step import AutogradEngine
            e = self._engine = AutogradEngine(self, dev)
        return e

    def forward(self, input):
        """(x (B, mel, T), y_idx (B, 1)) -> (xhat (B, mel, T), loss, loss dict)."""
        x, y_idx = input
        if not x.is_cuda:
            raise L.VqxError("vqvae2.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
        x = x.float().contiguous()
        y = self.embeds(y_idx[..., :1]).transpose(1, 2)  # (B, y_dim, 1)
        # hierarchical encode: level i reads level i-1's feature map
        z_levels, feat = [], x
        for enc in self.encoders:
            z, feat = enc(feat)
            z_levels.append(z)
        # quantize and decode from the top; z_vqs holds the quantized levels at their own rates, top first
        z_vqs, level_losses, enc_losses, scalars = [], [], [], []
        z = z_levels.pop()
        for i in reversed(range(self.levels)):
            if self.use_gst and i == self.levels - 1:
                z_vq = self.quantizers[i].pool_forward(z).unsqueeze(-1)
            else:
                z_vq, lvl, _, z_enc, detail = self.quantizers[i](z, loss_weights=(1.0, self.beta))
                level_losses.append(lvl)
                enc_losses.append(z_enc)
                scalars += [detail["entropy"], z_enc]
            z_vqs.append(z_vq)
            if i > 0:
                z = self.decoders[i]((z_levels.pop(), list(z_vqs)))
        xhat = self.decoders[0]((upsample_cat(z_vqs, x.shape[2]), [y]))
        x_loss = _LogLossFn.apply(xhat, x)
        loss = x_loss
        for lvl in level_losses:
            loss = loss + lvl
        vq = enc_losses[0]
        for t in enc_losses[1:]:
            vq = vq + t
        host = torch.stack([loss.detach(), vq, x_loss.detach(), *scalars]).tolist()  # the step's one readback
        losses = {"Total": host[0], "VQ loss": host[1], "X like": host[2]}
        for k in range(len(level_losses)):
            losses[f"entropy.{k}"] = host[3 + 2 * k]
            losses[f"quanti_err.{k}"] = host[4 + 2 * k]
        return xhat, loss, losses

    # ------------------------------------------------------------ conversion
    # The reference defines conversion through forward: xhat of forward((x, y')) is x
    # rendered with speaker y'.  y enters decoders[0] alone, so the codes of every
    # level depend on x only: analyze gives them, synthesize renders them.
    def _is_style(self, i):
        return self.use_gst and i == self.levels - 1

    def level_lengths(self, lengths):
        """Host arithmetic: [[frames of utterance b at level i] for every level i]
        for utterances of `lengths` input frames (level 0 first; the strided
        stage convs floor, _stage_frames).  ValueError when an utterance
        leaves a level without a frame."""
        lengths = lens = list(ops.len_array(lengths, what="vqvae2.Model lengths"))
        out = []
        for i, enc in enumerate(self.encoders):
            for k in enc.stage_index:
                lens = [_stage_frames(n, getattr(enc.encode[k], "scale", 1)) for n in lens]
            if min(lens) < 1:
                b = lens.index(min(lens))
                raise ValueError(f"vqvae2.Model: utterance {b} of {lengths[b]} frames leaves level {i} without a frame")
            out.append(lens)
        return out

    def _batch_lengths(self, lengths, B, who):
        """(lengths as a list, level_lengths, the padded level-0 frame count's granule)."""
        lens = list(ops.len_array(lengths, B, f"{who} lengths"))
        return lens, self.level_lengths(lens), math.prod(_total_scale(enc) for enc in self.encoders)

    def _analyze_lengths(self, x, lengths):
        """analyze for a padded batch: utterance b owns frames t < lengths[b]."""
        who = "vqvae2.Model.analyze"
        B, mel, T = x.shape
        lens, lv, gran = self._batch_lengths(lengths, B, who)
        if max(lens) > T:
            raise ValueError(f"{who}: lengths up to {max(lens)} exceed x's {T} frames")
        with torch.no_grad():
            dt, dev = _DT[self.compute_dtype], x.device
            e = functools.partial(torch.empty, device=dev)
            Tp = -(-T // gran) * gran  # every level's padded length divides exactly
            x = x.float()
            if Tp != T:
                xp = x.new_zeros(B, mel, Tp)
                xp[:, :, :T] = x
                x = xp
            feat = ops.nct_to_ntc(x.contiguous(), e(B * Tp, mel, dtype=dt))
            ops.mask_tail(feat, Tp, lens)  # the input's padding is never trusted
            Ti, zs, lin = Tp, [], lens
            for i, enc in enumerate(self.encoders):
                z, feat, Ti = enc.forward_rows(feat, B, Ti, lengths=lin)
                zs.append((z, Ti))
                lin = lv[i]
            codes, cond, cond_len = [None] * self.levels, [], []  # cond: the levels of codes_upsample_cat_len, top first
            z, Ti = zs.pop()
            for i in reversed(range(self.levels)):
                q = self.quantizers[i]
                if self._is_style(i):
                    mean = ops.segment_mean(z, Ti, lv[i], e(B, z.shape[1], dtype=F32))
                    style = q.pool_rows(mean, 1)
                    codes[i] = style.unsqueeze(-1)
                    cond.append(style)
                    cond_len.append([1] * B)
                else:
                    idx = q.encode(z.view(B, Ti, -1), time_last=False)  # tail entries: whatever the pad rows gave
                    Tm = max(lv[i])
                    keep = (torch.arange(Tm)[None, :] < torch.tensor(lv[i])[:, None]).to(dev)
                    codes[i] = torch.where(keep, idx[:, :Tm], torch.zeros((), dtype=idx.dtype, device=dev))
                    cond.append((idx, q.embeddings.detach(), q.normalize))
                    cond_len.append(lv[i])
                if i > 0:
                    z, Ti = zs.pop()
                    ops.mask_tail(z, Ti, lv[i - 1])  # the encoder's z becomes a decoder's input
                    xin = z if dt == F32 else ops.convert_2d(z, e(z.shape, dtype=dt))
                    dec = self.decoders[i]
                    full = ops.codes_upsample_cat_len(cond, B, Ti, lv[i - 1], cond_len, e(B * Ti, dec.cond_ch, dtype=F32))
                    z = dec.forward_rows(xin, B, Ti, [full], lengths=lv[i - 1])
            return codes

    def analyze(self, x, lengths=None):
        """x (B, mel, T) -> the codes forward would pick, one entry per level in
        level order: int64 indices (B, T_i) of a quantized level, the style
        embedding (B, F, 1) f32 of a style-token top level.  Computed in
        forward's order (top first, decoders[2] and decoders[1] producing the
        lower levels' quantizer inputs) on frame-major rows throughout, under
        no_grad; no parameter or buffer is written (forward renormalises the
        codebooks in place; here they are normalised on the fly).  One utterance
        (B == 1) may have any length that leaves every level a frame.

        lengths (a host sequence or a CPU int tensor, never a device tensor):
        a padded batch, utterance b owning frames t < lengths[b] <= T; whatever
        x holds from lengths[b] on is ignored.  A quantized level comes back
        as int64 (B, max_b len_i[b]) with 0 at the padded positions
        (level_lengths gives len_i), the style level as (B, F, 1).  Each
        utterance gets the codes it would get alone."""
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.encoders[0].in_ch:
            raise ValueError(f"vqvae2.Model.analyze: x must be (B, {self.encoders[0].in_ch}, T)")
        if lengths is not None:  # validated on the host before the device is touched
            lens, _, _ = self._batch_lengths(lengths, x.shape[0], "vqvae2.Model.analyze")
            if max(lens) > x.shape[2]:
                raise ValueError(f"vqvae2.Model.analyze: lengths up to {max(lens)} exceed x's {x.shape[2]} frames")
        if not x.is_cuda:
            raise L.VqxError("vqvae2.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
        if lengths is not None:
            return self._analyze_lengths(x, lengths)
        with torch.no_grad():
            B, _, T = x.shape
            dt = _DT[self.compute_dtype]
            e = functools.partial(torch.empty, device=x.device)
            feat, Ti, zs = ops.nct_to_ntc(x.float().contiguous(), e(B * T, x.shape[1], dtype=dt)), T, []
            for enc in self.encoders:
                z, feat, Ti = enc.forward_rows(feat, B, Ti)
                zs.append((z, Ti))
            codes, cond = [None] * self.levels, []  # cond: the quantized levels as f32 rows, top first
            z, Ti = zs.pop()
            for i in reversed(range(self.levels)):
                q = self.quantizers[i]
                if self._is_style(i):
                    style = q.pool_rows(z, Ti)
                    codes[i] = style.unsqueeze(-1)
                    cond.append(style)
                else:
                    idx = codes[i] = q.encode(z.view(B, Ti, -1), time_last=False)
                    if i > 0:
                        cond.append(ops.codes_upsample_cat([(idx, q.embeddings.detach(), q.normalize)], B, Ti,
                                                           e(B * Ti, q.z_dim, dtype=F32)))
                if i > 0:
                    z, Ti = zs.pop()
                    xin = z if dt == F32 else ops.convert_2d(z, e(z.shape, dtype=dt))
                    z = self.decoders[i].forward_rows(xin, B, Ti, cond)
            return codes

    def _check_codes(self, codes, y_idx, time):
        """synthesize's validation, on the host before any libvqx launch (one
        readback: the extremes of every index tensor, from torch's aminmax).
        Returns (codes as a list, B, T)."""
        who = "vqvae2.Model.synthesize"
        codes = list(codes)
        if len(codes) != self.levels or not all(torch.is_tensor(c) for c in codes):
            raise ValueError(f"{who}: codes must hold one tensor per level ({self.levels})")
        B, width, spans = codes[0].shape[0], 0, []
        for i, c in enumerate(codes):
            q = self.quantizers[i]
            if self._is_style(i):
                if c.dim() != 3 or not c.is_floating_point() or c.shape[1] % 4:
                    raise ValueError(f"{who}: level {i} is a style level: a float (B, F, T_i) tensor, F a multiple of 4")
                width += c.shape[1]
            else:
                if c.dim() != 2 or c.dtype != torch.int64:
                    raise ValueError(f"{who}: level {i} is a quantized level: int64 indices (B, T_i)")
                width += q.z_dim
                if c.numel():
                    spans += list(torch.aminmax(c))
            if c.shape[0] != B:
                raise ValueError(f"{who}: level {i} has batch size {c.shape[0]}, level 0 has {B}")
        if not torch.is_tensor(y_idx) or y_idx.dim() != 2 or y_idx.shape[0] != B:
            raise ValueError(f"{who}: y_idx must be (B, 1) speaker indices with B = {B}")
        if codes[0].dim() != 2 and time is None:
            raise ValueError(f"{who}: give `time` when level 0 is not an index tensor")
        T = int(time) if time is not None else codes[0].shape[1] * _total_scale(self.encoders[0])
        for i, c in enumerate(codes):
            try:
                src_index(T, c.shape[-1])
            except ValueError:
                raise ValueError(f"{who}: level {i} has {c.shape[-1]} frames, which do not stretch to T = {T} "
                                 "(1 <= T_i <= T)") from None
        want = self.decoders[0].layers[0].cin
        if width != want:
            raise ValueError(f"{who}: the levels' channels sum to {width}, decoders[0] takes {want}")
        if spans:
            ext = torch.stack(spans).tolist()  # the one readback
            quantized = [i for i in range(self.levels) if not self._is_style(i) and codes[i].numel()]
            for k, i in enumerate(quantized):
                K = self.quantizers[i].z_num
                if ext[2 * k] < 0 or ext[2 * k + 1] >= K:
                    raise ValueError(f"{who}: level {i} has indices in {ext[2 * k]}..{ext[2 * k + 1]}, the codebook "
                                     f"holds 0..{K - 1}")
        return codes, B, T

    def _synthesize_lengths(self, codes, y_idx, time, lengths):
        """synthesize for a padded batch: utterance b has lengths[b] output frames."""
        who = "vqvae2.Model.synthesize"
        if not torch.is_tensor(y_idx) or y_idx.dim() != 2:
            raise ValueError(f"{who}: y_idx must be (B, 1) speaker indices")
        lens, lv, _ = self._batch_lengths(lengths, y_idx.shape[0], who)
        if time is not None and int(time) != max(lens):
            raise ValueError(f"{who}: with lengths the output has max(lengths) = {max(lens)} frames; time = {time}")
        codes = list(codes)
        for i, c in enumerate(codes[:self.levels]):
            if not torch.is_tensor(c):
                continue  # _check_codes names it
            if self._is_style(i):
                if c.dim() == 3 and c.shape[2] != 1:
                    raise ValueError(f"{who}: with lengths the style level is (B, F, 1), got {tuple(c.shape)}")
            elif c.dim() == 2 and c.shape[1] < max(lv[i]):
                raise ValueError(f"{who}: level {i} holds {c.shape[1]} frames, the lengths need {max(lv[i])}")
        codes, B, T = self._check_codes(codes, y_idx, max(lens))
        if not all(c.is_cuda for c in codes) or not y_idx.is_cuda:
            raise L.VqxError("vqvae2.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
        with torch.no_grad():
            levels, level_len = [], []
            for i in reversed(range(self.levels)):
                c, q = codes[i], self.quantizers[i]
                if self._is_style(i):
                    levels.append(c.float().reshape(B, -1))
                    level_len.append([1] * B)
                else:
                    c = c.contiguous()
                    if c.data_ptr() % 16:  # a slice of a longer index tensor: the kernel reads aligned pointers
                        c = c.clone()
                    levels.append((c, q.embeddings.detach(), q.normalize))
                    level_len.append(lv[i])
            dec = self.decoders[0]
            rows = torch.empty(B * T, dec.layers[0].cin, device=y_idx.device, dtype=_DT[self.compute_dtype])
            ops.codes_upsample_cat_len(levels, B, T, lens, level_len, rows)
            y = self.embeds(y_idx[..., :1]).reshape(B, -1)
            return _to_nct(dec.forward_rows(rows, B, T, [y], lengths=lens), B, T)

    def synthesize(self, input, time=None, lengths=None):
        """((codes, y_idx (B, 1)), time) -> xhat (B, mel, T): decoders[0] on the
        codes of `analyze` (entries may come from different calls, e.g. the style
        of another utterance) with the speaker embedding as conditioning, as
        forward.  One vqx_codes_upsample_cat launch builds the decoder's
        frame-major input from the indices, channels stacked top level first.
        T = `time`, else codes[0]'s frames times encoder 0's down-sampling.
        Under no_grad; writes no parameter or buffer.  Bad codes raise
        ValueError before any libvqx launch.

        lengths (host values, as analyze): the codes of a padded batch as
        analyze(x, lengths) returns them; xhat is (B, mel, max(lengths)) with
        zeros at t >= lengths[b], each utterance rendered as it would be alone
        (its own stretch factors, GroupNorm statistics and conv padding)."""
        codes, y_idx = input
        if lengths is not None:
            return self._synthesize_lengths(codes, y_idx, time, lengths)
        codes, B, T = self._check_codes(codes, y_idx, time)
        if not all(c.is_cuda for c in codes) or not y_idx.is_cuda:
            raise L.VqxError("vqvae2.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
        with torch.no_grad():
            levels = []
            for i in reversed(range(self.levels)):
                c, q = codes[i], self.quantizers[i]
                if self._is_style(i):
                    levels.append(c.float().reshape(B, -1) if c.shape[2] == 1 else _to_rows(c))
                else:
                    c = c.contiguous()
                    if c.data_ptr() % 16:  # a slice of a longer index tensor: the kernel reads aligned pointers
                        c = c.clone()
                    levels.append((c, q.embeddings.detach(), q.normalize))
            dec = self.decoders[0]
            rows = torch.empty(B * T, dec.layers[0].cin, device=y_idx.device, dtype=_DT[self.compute_dtype])
            ops.codes_upsample_cat(levels, B, T, rows)
            y = self.embeds(y_idx[..., :1]).reshape(B, -1)
            return _to_nct(dec.forward_rows(rows, B, T, [y]), B, T)

    def convert(self, input, lengths=None):
        """(x (B, mel, T), y_idx (B, 1)) -> x rendered with speaker y_idx:
        synthesize((analyze(x), y_idx), time=T), the xhat of forward((x, y_idx)).
        lengths: a padded batch (analyze, synthesize); (B, mel, max(lengths))."""
        x, y_idx = input
        if lengths is not None:
            return self.synthesize((self.analyze(x, lengths), y_idx), lengths=lengths)
        return self.synthesize((self.analyze(x), y_idx), time=x.shape[2])

    def encode(self, input):
        raise NotImplementedError("vqvae2.Model.encode: the reference's version reads self.encoder and self.quantizer, "
                                  "which the hierarchical model does not have (vqvae2.py:49-56); no semantics to restate")

    def decode(self, input):
        raise NotImplementedError("vqvae2.Model.decode: the reference's version reads self.quantizer and self.decoder, "
                                  "which the hierarchical model does not have (vqvae2.py:59-64); no semantics to restate")

    def infer(self, input):
        raise NotImplementedError("vqvae2.Model.infer: built on encode / decode, which the reference leaves undefined "
                                  "for the hierarchical model (vqvae2.py:67-71)")

    def remove_weight_norm(self):
        """vqvae2.py:146-156: bake w = g*v/||v|| into a plain `weight` on every conv that has weight norm."""
        for m in self.modules():
            if isinstance(m, (WNConv1d, ResampleConv1d)) and m.has_weight_norm:
                m.remove_weight_norm()
        self._engine = None  # the parameter list changed
