"""The encoder of the hierarchical models (reference `Encoder`,
vqvae2.py:175-271) on the MI355X: two outputs, the projected z and the feature
map the next level's encoder reads.

`Encoder` has the reference's constructor arguments, module tree, parameter
order and state_dict keys plus `compute_dtype: fp32|bf16`.  Its forward
(`_encoder_rows`) and backward are the launch sequences of engine/step.py
encoder_fwd / encoder_bwd composed from `ops.*` calls inside one
torch.autograd.Function.  `forward_rows` is the forward alone on frame-major
rows; it also takes one utterance of any length or a padded batch with `lengths`.
"""
import functools
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .hier_common import DT, F32, colsum, dgrad, fwd, pack, to_nct, wgrad
from .vqvae import Encoder as _Encoder


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
        self.dt = DT[enc.compute_dtype]
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


def stage_frames(T_in, s):
    """Output frames of a stage conv (kernel 2s, stride s, padding s//2 + s%2) on T_in frames."""
    return T_in if s == 1 else (T_in + 2 * (s // 2 + s % 2) - 2 * s) // s + 1


def total_scale(enc):
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
    holds zeros in the other rows.  A stage keeps stage_frames(len, s) frames
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
            w = wp[conv.at] = pack(ts[conv.at], False, dt)
            fwd(conv, inp, w, c, T_in, bias=ts[conv.at + 1], act=L.PRO_LRELU, y2=a)
        else:  # folded: s frames of cin channels as one frame of s*cin, 3 taps
            w, norm = e(C, 3 * s * conv.cin, dtype=dt), e(C, dtype=F32)
            ops.weight_norm_fwd(conv.mod._table(w, norm))
            wp[conv.at] = (w, norm)
            Tf = Ts  # folded frames the GEMM runs on
            if T_in % s:
                if not (ragged and B == 1):
                    raise ValueError(f"vqvae2.Encoder: a stage of {T_in} frames is not a multiple of its stride {s}")
                Tf, Ts = Ts + 1, stage_frames(T_in, s)
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
            lens = [stage_frames(n, s) for n in lens]
            ops.mask_tail(a, Ts, lens)
        # GroupNorm statistics from the GEMM's epilogue tiles
        fuse = lens is None and Ts % 128 == 0 and C % 128 == 0
        cs, acts, per_block = [c], [a], []
        for convs, gn_at, skip in blocks:
            src, hs, mrs, gs, gkw = acts[-1], [], [], [], {}
            for l, (cv, ag) in enumerate(zip(convs, gn_at)):
                last = l == len(convs) - 1
                w = wp[cv.at] = pack(ts[cv.at], False, dt)
                h, mr = e(N, C, dtype=dt), e(B, 2, dtype=F32)
                if fuse:
                    gst = e((N // 128) * (C // 128) * 4, dtype=F32)
                    fwd(cv, src, w, h, Ts, bias=ts[cv.at + 1], gn_stats=gst, gn_groups=1)
                    if last:
                        gkw = dict(gn_tiles=gst)  # merged inside the skip GEMM
                    else:
                        ops.gn_finalize_tiles(gst, N, Ts, C, 1, mr)
                elif lens is not None:
                    fwd(cv, src, w, h, Ts, bias=ts[cv.at + 1])
                    ops.groupnorm_stats_len(h, Ts, 1, lens, gn_part, mr)
                else:
                    fwd(cv, src, w, h, Ts, bias=ts[cv.at + 1])
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
            w = wp[skip.at] = pack(ts[skip.at], False, dt)
            c, a = e(N, C, dtype=dt), e(N, C, dtype=dt)
            fwd(skip, cs[-1], w, c, Ts, bias=ts[skip.at + 1], gn_h=hs[-1], gn_mr=mrs[-1], gn_gamma=ts[gn_at[-1]],
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
    w = wp[zp.at] = pack(ts[zp.at], False, dt)
    z = e(B * T_in, zp.cout, dtype=F32)
    fwd(zp, inp, w, z, T_in, bias=ts[zp.at + 1], out_f32=True)
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
        return to_nct(z, B, T_out), to_nct(feat, B, T_out)

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
            grads[zp.at + 1] = colsum(dzr, cs_part)
            grads[zp.at] = wgrad(zp, dzr, a_last, Ts)
            cur = e(N, zp.cin, dtype=dt)
            dgrad(zp, dzr, wp[zp.at], cur, Ts, mask=a_last, mask_slope=0.2,
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
                    grads[cv.at + 1] = colsum(cs_b, cs_part)
                    grads[ag], grads[ag + 1] = colsum(dgam_b, cs_part), colsum(dbet_b, cs_part)
                    src = acts[j] if l == 0 else gs[l - 1]
                    grads[cv.at] = wgrad(cv, dh, src, Ts)
                    # into LeakyReLU(.): its derivative from the sign of the stored output
                    dy = tmp = e(N, C, dtype=dt)
                    dgrad(cv, dh, wp[cv.at], dy, Ts, mask=src, mask_slope=0.2)
                # the skip conv last, adding the stack's data gradient
                grads[skip.at + 1] = colsum(cur, cs_part)
                grads[skip.at] = wgrad(skip, cur, cs[j], Ts)
                nxt = e(N, C, dtype=dt)
                dgrad(skip, cur, wp[skip.at], nxt, Ts, res=tmp)
                cur = nxt
            # cur = dL/dc_0 of the stage (the stage conv's output)
            grads[conv.at + 1] = colsum(cur, cs_part)
            want_dx = si > 0 or ctx.needs_input_grad[2]
            prev_a = saved[si - 1][4][-1] if si > 0 else None
            mask = {} if si == 0 else dict(mask=prev_a, mask_slope=0.2)
            s = conv.scale
            if s == 1:
                grads[conv.at] = wgrad(conv, cur, inp, T_in)
                if want_dx:
                    nxt = e(B * T_in, conv.cin, dtype=dt if si else F32)
                    dgrad(conv, cur, wp[conv.at], nxt, T_in, **(mask if si else dict(out_f32=True)))
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
                dx = to_nct(nxt, B, T_in)
        return (None, None, dx, *grads)


class Encoder(_Encoder):
    """vqvae2.py:175-271 with `compute_dtype: fp32|bf16`: forward(x (B, C_in, T))
    -> (z, feat), z = z_proj(feat) (B, z_channels, T'), feat the last stage's
    LeakyReLU output (B, out_channels[-1], T'), T' = T / prod(downsample_scales).
    The reference's module tree: `encode` (without the projection) and `z_proj`."""

    def __init__(self, *args, compute_dtype="fp32", **kw):
        if compute_dtype not in DT:
            raise ValueError(f"compute_dtype {compute_dtype!r} is not fp32 or bf16")
        super().__init__(*args, **kw)
        layers = list(self.encode)
        self.encode = nn.Sequential(*layers[:-1])
        self.z_proj = layers[-1]
        self.compute_dtype = compute_dtype
        self._plan = None

    @property
    def plan(self):
        """The module tree's _EncPlan, built on first use."""
        if self._plan is None:
            self._plan = _EncPlan(self)
        return self._plan

    def forward(self, x):
        if x.dim() != 3 or x.shape[1] != self.in_ch:
            raise ValueError(f"vqvae2.Encoder: x {tuple(x.shape)} is not (B, {self.in_ch}, T)")
        plan = self.plan
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
        plan = self.plan
        if not x_rows.is_cuda or x_rows.dim() != 2 or x_rows.dtype != plan.dt or x_rows.stride(1) != 1 \
                or tuple(x_rows.shape) != (B * T, self.in_ch):
            raise ValueError(f"vqvae2.Encoder: x_rows must be device [{B * T}, {self.in_ch}] rows in {plan.dt}")
        ragged, T_in = False, T
        if lengths is not None:
            lens = list(ops.len_array(lengths, B, "vqvae2.Encoder lengths"))
            if any(not 1 <= n <= T for n in lens):
                raise ValueError(f"vqvae2.Encoder: lengths must lie in 1..T = {T}")
            for conv, _ in plan.stages:
                lens = [stage_frames(n, conv.scale) for n in lens]
                if min(lens) < 1:
                    raise ValueError(f"vqvae2.Encoder: an utterance of {lengths[lens.index(min(lens))]} frames leaves a "
                                     "stage without a frame")
        else:
            for conv, _ in plan.stages:
                ragged |= T_in % conv.scale != 0
                T_in = stage_frames(T_in, conv.scale)
                if T_in < 1:
                    raise ValueError(f"vqvae2.Encoder: T = {T} leaves a stage without a frame")
            if ragged and B != 1:
                raise ValueError(f"vqvae2.Encoder: T = {T} is not a multiple of every stage's stride; such lengths are "
                                 f"converted one utterance at a time (B == 1), got B = {B}")
        with torch.no_grad():
            ts = [None if t is None else t.detach().float() for t in _EncPlan.tensors(self, plan)]
            return _encoder_rows(plan, x_rows, B, T, ts, ragged=ragged, lengths=lengths)[:3]
