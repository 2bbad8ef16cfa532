"""The decoder of the hierarchical models: conditioning that varies in time
(reference `Decoder`, vqvae2.py:274-371) on the MI355X.

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
decoder_fwd / decoder_bwd composed from `ops.*` calls (`decoder_rows`,
`decoder_rows_bwd`) inside one torch.autograd.Function.  Weight norm goes
through torch autograd on `effective_weight()`: the function receives
w = g*v/||v|| in torch's layout, packs it for the GEMMs and returns dL/dw in
the same layout.  The conditioning GEMMs (conv_cond and its gradients) run in
fp32 in both compute dtypes, as the engine's speaker conditioning does.
"""
import functools
import math
from types import SimpleNamespace

import torch
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .hier_common import DT, F32, choose_tc, colsum, dgrad, fwd, pack, src_index, to_nct, to_rows, wgrad
from .layers import ResSkipBlock, WNConv1d
from .vqvae import Decoder as _Decoder


class _Conv:
    """One conv of the plan: geometry + where its tensors sit in the flat argument list."""

    def __init__(self, mod, at):
        self.transposed, self.k, self.dil = mod.transposed, mod.k, mod.dilation
        self.cin, self.cout = mod.cin, mod.cout
        self.pad = (mod.k - 1) * mod.dilation - mod.padding if mod.transposed else mod.padding
        if 2 * self.pad != (mod.k - 1) * mod.dilation:
            raise NotImplementedError("asymmetric padding (the output length would change)")
        self.at = at  # index of w in the tensor list; bias follows


class Plan:
    """Static description of a Decoder for decoder_rows / decoder_rows_bwd (no tensors)."""

    def __init__(self, dec):
        self.dt = DT[dec.compute_dtype]
        self.steps, at = [], 0  # ("conv", _Conv) | ("block", conv_in, conv_cond | None, res_skip, at of gamma)
        for layer in dec.layers:
            if isinstance(layer, ResSkipBlock):
                n = 0 if layer.conv_cond is None else 2  # unconditioned: 6 tensors per block, else conv_cond's two more
                cc = _Conv(layer.conv_cond, at + 2) if n else None
                rs = _Conv(layer.res_skip_layers, at + 4 + n)
                self.steps.append(("block", _Conv(layer.conv_in, at), cc, rs, at + 2 + n))
                at += 6 + n
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


def decoder_rows(plan, x2, B, T, rows, T_levels, ts, lengths=None):
    """The decoder's forward launches on frame-major operands: x2 [B*T, C] in
    the compute dtype, the conditioning levels `rows` (f32 [B*T_l, C_l]) and the
    flat tensor list `ts`.  Returns (xhat f32 [B*T, final], keep): `keep` holds
    what decoder_rows_bwd reads (Tc, c_low, saved, wp: the packed weights by
    tensor index, a_skip, f1, ts); a caller that wants no backward drops it.
    An unconditioned plan (plan.cond == 0) takes rows = None: no row bias in
    the conv_in GEMMs, no conv_cond launches; Tc and c_low are None.

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
            w = wp[cv.at] = pack(ts[cv.at], cv.transposed, dt)
            y = e(N, cv.cout, dtype=dt)
            fwd(cv, cur, w, y, T, bias=ts[cv.at + 1])
            if lens is not None:
                ops.mask_tail(y, T, lens)
            saved.append((cur,))
            cur = y
            continue
        _, ci, cc, rs, ag = st
        C = ci.cin
        w_in, w_rs = pack(ts[ci.at], True, dt), pack(ts[rs.at], False, dt)
        wp[ci.at], wp[rs.at] = w_in, w_rs
        seg = {}
        if cc is not None:
            w_cc = wp[cc.at] = pack(ts[cc.at], False, F32)
            P = e(B * Tc, 2 * C, dtype=F32)  # conv_cond(c) + its bias, one row per conditioning frame
            fwd(cc, c_low, w_cc, P, Tc, bias=ts[cc.at + 1])
            seg = dict(rowbias=P, rowbias_T=Tc if Tc > 1 else 0)
        u, g, mr = e(N, 2 * C, dtype=dt), e(N, C, dtype=dt), e(B, 2, 2, dtype=F32)
        if lens is not None:  # statistics and apply over each utterance's own rows; g gets a zero tail
            fwd(ci, cur, w_in, u, T, bias=ts[ci.at + 1], **seg)
            ops.groupnorm_stats_len(u, T, 2, lens, gn_part, mr)
            ops.gn_glu_fwd_len(u, g, T, lens, mr, ts[ag], ts[ag + 1])
        elif T % 128 == 0 and C % 128 == 0:  # GroupNorm statistics from the GEMM's epilogue tiles
            gst = e((N // 128) * (2 * C // 128) * 4, dtype=F32)
            fwd(ci, cur, w_in, u, T, bias=ts[ci.at + 1], gn_stats=gst, gn_groups=2, **seg)
            ops.gn_glu_fwd_tiles(u, g, T, gst, mr, ts[ag], ts[ag + 1])
        else:
            fwd(ci, cur, w_in, u, T, bias=ts[ci.at + 1], **seg)
            ops.groupnorm_stats(u, T, 2, gn_part, mr)
            ops.gn_glu_fwd(u, g, T, mr, ts[ag], ts[ag + 1])
        y = e(N, C, dtype=dt)
        fwd(rs, g, w_rs, y, T, bias=ts[rs.at + 1], res=cur, out2=skip32, split_col=C, out2_accumulate=not first)
        if lens is not None:  # the residual is the next conv_in's operand; its tail holds the bias
            ops.mask_tail(y, T, lens)
        first = False
        saved.append((cur, u, g, mr))
        cur = y
    a_skip, f1 = e(N, plan.S, dtype=dt), e(N, plan.fin1.cout, dtype=dt)
    xhat = e(N, plan.final, dtype=F32)
    ops.scale_act_2d(skip32, a_skip, plan.scale, L.PRO_RELU)
    w1 = wp[plan.fin1.at] = pack(ts[plan.fin1.at], False, dt)
    w2 = wp[plan.fin2.at] = pack(ts[plan.fin2.at], False, dt)
    if lens is not None and plan.fin1.k > 1:
        ops.mask_tail(a_skip, T, lens)
    fwd(plan.fin1, a_skip, w1, f1, T, bias=ts[plan.fin1.at + 1], act=L.PRO_RELU)
    if lens is not None and plan.fin2.k > 1:
        ops.mask_tail(f1, T, lens)
    fwd(plan.fin2, f1, w2, xhat, T, bias=ts[plan.fin2.at + 1], out_f32=True)
    if lens is not None:
        ops.mask_tail(xhat, T, lens)
    return xhat, SimpleNamespace(Tc=Tc, c_low=c_low, saved=saved, wp=wp, a_skip=a_skip, f1=f1, ts=ts)


def decoder_rows_bwd(plan, B, T, keep, dxhat):
    """The decoder's backward launches on frame-major operands: `keep` as
    decoder_rows returned it, dxhat [B*T, final] the output gradient in the
    compute dtype.  Returns (dx f32 [B*T, C_in], dc f32 [B*keep.Tc, cond] the
    gradient of c_low or None for an unconditioned plan, grads: dL/d(ts) in the
    plan's order)."""
    Tc, c_low, saved, wp, a_skip, f1, ts = keep.Tc, keep.c_low, keep.saved, keep.wp, keep.a_skip, keep.f1, keep.ts
    dev, dt, S = dxhat.device, plan.dt, plan.S
    N = B * T
    e = functools.partial(torch.empty, device=dev)
    grads = [None] * plan.n_tensors
    Cmax = max(st[1].cin for st in plan.steps if st[0] == "block")
    cs_part = e(64 * max(2 * Cmax, Cmax + S, plan.final, plan.cond, 1024), dtype=F32)
    gnb_part = e(B * 64 * 2, dtype=F32)
    # final layer: ReLU, conv, ReLU, conv on scale * sum(skips)
    f1c, f2c = plan.fin1, plan.fin2
    grads[f2c.at + 1] = colsum(dxhat, cs_part)
    grads[f2c.at] = wgrad(f2c, dxhat, f1, T)
    df1 = e(N, f2c.cin, dtype=dt)
    dgrad(f2c, dxhat, wp[f2c.at], df1, T, mask=f1, mask_slope=0.0)
    grads[f1c.at + 1] = colsum(df1, cs_part)
    grads[f1c.at] = wgrad(f1c, df1, a_skip, T)
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
    dgrad(f1c, df1, wp[f1c.at], cur[:, C_last:], T, mask=a_skip, mask_slope=0.0, mask_scale=plan.scale)
    ops.convert_2d(None, cur, cols=C_last)  # dL/dx at the decoder output is 0: the last residual is unused
    k, dc, dx = 0, None, None
    for st, sv in zip(reversed(plan.steps), reversed(saved)):
        if st[0] == "conv":
            cv = st[1]
            cur_x = cur[:, :cv.cout]
            grads[cv.at + 1] = colsum(cur_x, cs_part)
            grads[cv.at] = wgrad(cv, cur_x, sv[0], T)
            if sv[0] is saved[0][0]:  # the decoder input
                dx = e(N, cv.cin, dtype=F32)
                dgrad(cv, cur_x, wp[cv.at], dx, T, out_f32=True)
            else:
                k ^= 1
                nxt = dr(cv.cin, k)
                dgrad(cv, cur_x, wp[cv.at], nxt[:, :cv.cin], T)
                cur = nxt
            continue
        _, ci, cc, rs, ag = st
        xin, u, g, mr = sv
        C = ci.cin
        grads[rs.at + 1] = colsum(cur, cs_part)
        grads[rs.at] = wgrad(rs, cur, g, T)
        dg, du = e(N, C, dtype=dt), e(N, 2 * C, dtype=dt)
        dgrad(rs, cur, wp[rs.at], dg, T)
        cs_b, dgam_b, dbet_b = (e(B, 2 * C, dtype=F32) for _ in range(3))
        ops.gn_bwd(dg, u, du, T, 2, True, mr, ts[ag], ts[ag + 1], gnb_part, cs_b, dgam_b, dbet_b)
        grads[ci.at + 1] = colsum(cs_b, cs_part)
        grads[ag], grads[ag + 1] = colsum(dgam_b, cs_part), colsum(dbet_b, cs_part)
        # conditioning: dP = the per-segment sums of du, then conv_cond's own gradients at the low rate
        if cc is not None:
            if Tc == 1:
                dP = cs_b
            else:
                dP = e(B * Tc, 2 * C, dtype=F32)
                ops.upsample_cat_bwd([dP], B, T, du)
            grads[cc.at + 1] = grads[ci.at + 1] if Tc == 1 else colsum(dP, cs_part)
            grads[cc.at] = wgrad(cc, dP, c_low, Tc)
            dc_new = e(B * Tc, plan.cond, dtype=F32)
            dgrad(cc, dP, wp[cc.at], dc_new, Tc, **({} if dc is None else dict(res=dc)))
            dc = dc_new
        grads[ci.at] = wgrad(ci, du, xin, T)
        k ^= 1
        nxt = dr(C, k)
        dgrad(ci, du, wp[ci.at], nxt[:, :C], T, res=cur[:, :C])
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
        rows = [to_rows(z) for z in cin] if plan.cond else None
        x2 = ops.nct_to_ntc(x.float().contiguous(), torch.empty(B * T, x.shape[1], device=x.device, dtype=plan.dt))
        xhat, keep = decoder_rows(plan, x2, B, T, rows, T_levels, ts)
        if save:
            ctx.plan, ctx.dims, ctx.T_levels, ctx.keep = plan, (B, T), T_levels, keep
            ctx.level_shapes = [tuple(z.shape) for z in cin]
        return to_nct(xhat, B, T)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        plan, (B, T), Tc = ctx.plan, ctx.dims, ctx.keep.Tc
        e = functools.partial(torch.empty, device=dout.device)
        dxhat = ops.nct_to_ntc(dout.float().contiguous(), e(B * T, plan.final, dtype=plan.dt))
        dx, dc, grads = decoder_rows_bwd(plan, B, T, ctx.keep, dxhat)
        # the conditioning's gradient back to the levels (or to the tensor c)
        if dc is None:
            dcin = []
        elif ctx.T_levels:
            dl = [e(B * Tl, Cl, dtype=F32) for _, Cl, Tl in ctx.level_shapes]
            ops.upsample_cat_bwd(dl, B, Tc, dc)
            dcin = [to_nct(d, B, s[2]) for d, s in zip(dl, ctx.level_shapes)]
        else:
            dcin = [to_nct(dc, B, T)]
        ctx.keep = None
        return (None, None, None, to_nct(dx, B, T), *dcin, *grads)


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
        if compute_dtype not in DT:
            raise ValueError(f"compute_dtype {compute_dtype!r} is not fp32 or bf16")
        super().__init__(*args, **kw)
        self.compute_dtype = compute_dtype
        self._plan = None

    @property
    def plan(self):
        """The module tree's Plan, built on first use."""
        if self._plan is None:
            self._plan = Plan(self)
        return self._plan

    def forward(self, input):
        x, c = input
        if x.dim() != 3:
            raise ValueError(f"vqvae2.Decoder: x {tuple(x.shape)} is not (B, C, T)")
        B, _, T = x.shape
        levels, T_levels = [], ()  # unconditioned (cond_channels 0 / None), forward((x, None)): no levels
        if not self.cond_ch:
            if c is not None:
                raise ValueError("vqvae2.Decoder: this decoder is unconditioned (cond_channels 0); it takes (x, None) "
                                 "and would ignore the conditioning it was given")
        elif c is None:
            raise ValueError(f"vqvae2.Decoder: the conditioning is None, this decoder has cond_channels {self.cond_ch}")
        else:
            levels = [c] if torch.is_tensor(c) else list(c)
            if not levels or any(z.dim() != 3 or z.shape[0] != B for z in levels) \
                    or sum(z.shape[1] for z in levels) != self.cond_ch:
                raise ValueError(f"vqvae2.Decoder: the conditioning must be (B, C_l, T_l) levels with sum C_l == "
                                 f"{self.cond_ch}")
            if torch.is_tensor(c):
                if c.shape[2] != T:
                    raise ValueError(f"vqvae2.Decoder: a tensor c must have x's {T} frames, got {c.shape[2]}")
            else:
                T_levels = tuple(z.shape[2] for z in levels)
                for Tl in T_levels:
                    src_index(T, Tl)
        plan, ts = self.plan, Plan.tensors(self)
        save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, *levels, *ts))
        return _DecoderFn.apply(plan, save, T_levels, x, *levels, *ts)

    def forward_rows(self, x_rows, B, T, cond_rows, lengths=None):
        """forward without gradients on frame-major operands: x_rows [B*T, C] in
        the compute dtype (as vqx_codes_upsample_cat writes it) in place of
        (B, C, T), so the first layout change is skipped; cond_rows the
        conditioning levels as f32 [B*T_l, C_l] rows.  Returns xhat f32
        [B*T, final] rows.  Nothing is kept for a backward.  lengths: host
        ints, utterance b owns rows t < lengths[b] (x_rows zero elsewhere, the
        conditioning one row per utterance or full rate; decoder_rows)."""
        if lengths is not None:
            lengths = ops.len_array(lengths, B, "vqvae2.Decoder lengths")
            if any(not 1 <= n <= T for n in lengths):
                raise ValueError(f"vqvae2.Decoder: lengths must lie in 1..T = {T}")
        plan = self.plan
        if not x_rows.is_cuda or x_rows.dim() != 2 or x_rows.dtype != plan.dt or x_rows.stride(1) != 1 \
                or x_rows.shape[0] != B * T:
            raise ValueError(f"vqvae2.Decoder: x_rows must be device [{B * T}, C] rows in {plan.dt}")
        rows, T_levels = None, ()
        if not self.cond_ch:
            if cond_rows is not None:
                raise ValueError("vqvae2.Decoder: this decoder is unconditioned (cond_channels 0); cond_rows must be None")
        elif cond_rows is None or any(r.dim() != 2 or r.dtype != F32 or r.shape[0] % B for r in cond_rows) \
                or sum(r.shape[1] for r in cond_rows) != self.cond_ch:
            raise ValueError(f"vqvae2.Decoder: the conditioning must be f32 [B*T_l, C_l] rows with sum C_l == "
                             f"{self.cond_ch}")
        else:
            rows, T_levels = list(cond_rows), tuple(r.shape[0] // B for r in cond_rows)
            for Tl in T_levels:
                src_index(T, Tl)
            if lengths is not None and T_levels == (T,):
                T_levels = ()  # already at full rate: read in place
        with torch.no_grad():
            ts = [t.detach().float() for t in Plan.tensors(self)]
            return decoder_rows(plan, x_rows, B, T, rows, T_levels, ts, lengths)[0]
