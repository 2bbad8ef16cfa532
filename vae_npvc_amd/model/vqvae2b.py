"""The hierarchical model with parallel level decoders (reference
model/vqvae2b.py:11-165) on the MI355X, for
`model_type: vae_npvc_amd.model.vqvae2b`.

Every level quantizes its own encoder's output, as vqvae2a does, but the
decoders are not chained: level i has its own decoder, conditioned on its own
speaker embedding; the L outputs are stretched to the input's length, stacked
on channels and rendered by `final_decoder`, an unconditioned decoder
(`cond_channels: 0`, called as `final_decoder((z, None))`).  `decode` and
`infer` take one speaker per level.

The decode side is one torch.autograd.Function (`_DecodeSideFn`) over the flat
tensor lists of the L + 1 decoder plans.  Between the level inputs' rows and
xhat's rows everything is frame-major: a level decoder's output rows go into
the join (`vqx_upsample_cat_fwd`, which also stretches and rounds to the
compute dtype) and from there into the final decoder; backwards the final
decoder's fp32 input gradient is split, summed over each level's segments and
rounded once to the compute dtype by `vqx_upsample_cat_bwd_to`.  The launches
that compute are those of `vqvae2.Decoder` modules composed with
`upsample_cat`; only exact layout copies are gone, so the two give equal bits.
There is no CPU path.
"""
import functools

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .hier_base import HierModelBase
from .hier_common import DT, F32, mean_pool, src_index, to_nct, to_rows
from .hier_decoder import Decoder, Plan, decoder_rows, decoder_rows_bwd
from .hier_encoder import Encoder
from .layers import Conditions
from .layers_gst import StyleTokenLayer
from .layers_vq import EMAVectorQuantizer, Jitter, VectorQuantizer


class _DecodeSideFn(torch.autograd.Function):
    """forward(cfg, save, z_vq_0 .. z_vq_{L-1} (B, C_i, T_i), y_0 .. y_{L-1}
    (B, y_dim) speaker rows, the tensors of the L level plans, the tensors of
    the final plan) -> xhat (B, final, time).  cfg = (plans: L level plans and
    the final one, upsample_last, time)."""

    @staticmethod
    def forward(ctx, cfg, save, *rest):
        plans, upsample_last, time = cfg
        nl = len(plans) - 1
        zs, ys, flat = rest[:nl], rest[nl:2 * nl], rest[2 * nl:]
        if not all(t.is_cuda for t in rest):
            raise L.VqxError("vqvae2b.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
        dev, dt = zs[0].device, plans[0].dt
        B = zs[0].shape[0]
        e = functools.partial(torch.empty, device=dev)
        ts, at = [], 0
        for p in plans:
            ts.append([t.detach().float() for t in flat[at:at + p.n_tensors]])
            at += p.n_tensors
        outs, keeps, dims = [], [], []
        for i in range(nl):
            z = zs[i]
            C, Ti = z.shape[1], z.shape[2]
            Td = Ti if upsample_last else time
            if Td == Ti:  # the level at the decoder's own rate: the one layout change, into the compute dtype
                x2 = ops.nct_to_ntc(z.float().contiguous(), e(B * Ti, C, dtype=dt))
            else:
                x2 = ops.upsample_cat_fwd([to_rows(z)], B, Td, e(B * Td, C, dtype=dt))
            y = ys[i].detach().float().contiguous()
            xh, keep = decoder_rows(plans[i], x2, B, Td, [y], (1,), ts[i])
            outs.append(xh)
            keeps.append(keep if save else None)
            dims.append((Ti, Td, C))
        # the join: stretch the shorter levels, stack on channels, round once to the compute dtype
        joined = ops.upsample_cat_fwd(outs, B, time, e(B * time, sum(o.shape[1] for o in outs), dtype=dt))
        xhat, keep = decoder_rows(plans[nl], joined, B, time, None, (), ts[nl])
        if save:
            keeps.append(keep)
            ctx.cfg, ctx.B, ctx.dims, ctx.keeps = cfg, B, dims, keeps
        return to_nct(xhat, B, time)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        plans, upsample_last, time = ctx.cfg
        B, dims, keeps = ctx.B, ctx.dims, ctx.keeps
        ctx.keeps = None
        nl = len(plans) - 1
        fin, dt = plans[nl], plans[nl].dt
        e = functools.partial(torch.empty, device=dout.device)
        dxhat = ops.nct_to_ntc(dout.float().contiguous(), e(B * time, fin.final, dtype=dt))
        dx, _, g_fin = decoder_rows_bwd(fin, B, time, keeps[nl], dxhat)
        # every level decoder's output gradient: the fp32 sums over its segments, stored in the compute dtype
        dl = [e(B * Td, plans[i].final, dtype=dt) for i, (_, Td, _) in enumerate(dims)]
        ops.upsample_cat_bwd_to(dl, B, time, dx)
        dzs, dys, grads = [], [], []
        for i in range(nl):
            Ti, Td, C = dims[i]
            dxi, dc, g = decoder_rows_bwd(plans[i], B, Td, keeps[i], dl[i])
            grads += g
            dys.append(dc if ctx.needs_input_grad[2 + nl + i] else None)  # Tc == 1: dc is the speaker rows' gradient
            if not ctx.needs_input_grad[2 + i]:
                dzs.append(None)
            elif Td == Ti:
                dzs.append(to_nct(dxi, B, Ti))
            else:
                dz = ops.upsample_cat_bwd([e(B * Ti, C, dtype=F32)], B, Td, dxi)[0]
                dzs.append(to_nct(dz, B, Ti))
        return (None, None, *dzs, *dys, *grads, *g_fin)


def decode_side(decoders, final_decoder, z_vqs, ys, time, upsample_last):
    """The decode side of vqvae2b (vqvae2b.py:125-135): decoders[i] on z_vqs[i]
    (B, C_i, T_i) with the speaker rows ys[i] (B, y_dim), stretched before the
    decoder (upsample_last false) or after it, the outputs stacked and rendered
    by final_decoder.  Returns xhat (B, final, time)."""
    if len(z_vqs) != len(decoders) or len(ys) != len(decoders):
        raise ValueError("decode_side: one z_vq and one speaker row tensor per level decoder")
    B = z_vqs[0].shape[0]
    if final_decoder.cond_ch:
        raise ValueError("decode_side: final_decoder must be unconditioned (cond_channels 0)")
    for d, z, y in zip(decoders, z_vqs, ys):
        if z.dim() != 3 or z.shape[0] != B or z.shape[1] != d.layers[0].cin:
            raise ValueError(f"decode_side: a level {tuple(z.shape)} is not (B, {d.layers[0].cin}, T_i)")
        if y.dim() != 2 or y.shape[0] != B or y.shape[1] != d.cond_ch:
            raise ValueError(f"decode_side: speaker rows {tuple(y.shape)} are not ({B}, {d.cond_ch})")
        src_index(time, z.shape[2])
    if sum(d.final_ch for d in decoders) != final_decoder.layers[0].cin:
        raise ValueError(f"decode_side: the level decoders' final_channels sum to {sum(d.final_ch for d in decoders)}, "
                         f"final_decoder takes {final_decoder.layers[0].cin}")
    mods = [*decoders, final_decoder]
    if len({d.compute_dtype for d in mods}) != 1:
        raise ValueError("decode_side: the decoders must share one compute_dtype")
    plans = tuple(d.plan for d in mods)
    flat = [t for d in mods for t in Plan.tensors(d)]
    save = torch.is_grad_enabled() and any(t.requires_grad for t in (*z_vqs, *ys, *flat))
    cfg = (plans, bool(upsample_last), int(time))
    return _DecodeSideFn.apply(cfg, save, *z_vqs, *ys, *flat)


class Model(HierModelBase):
    """`Model(arch)` with the reference's keys: levels (1..3), use_gst (false
    at levels == 1), use_ema, y_num, y_dim, jitter_p, beta, pooling_last,
    upsample_last, encoder.{i}, decoder.{i}, quantizer.{i}, final_decoder
    (+ compute_dtype: fp32|bf16).  The module tree (encoders, quantizers,
    decoders, embeds, final_decoder, jitter), the parameter order and the
    state_dict keys are the reference's.

    forward((x, y_idx)) restates vqvae2b.py:99-149 (every level uses
    y_idx[..., :1]): xhat, loss, loss dict from one readback at the end.
    encode(x) restates :52-70; decode((zs, ys), time) restates :73-90 with ys
    (B, levels), level i rendered with speaker ys[:, i]; infer((x, ys)) is the
    two together.  convert((x, y_idx)) is the xhat of the eval-mode forward
    (encode and convert are HierModelBase's).  encode, decode, infer and
    convert run without gradients and write no parameter or buffer.  All four
    take `lengths=` (host ints): a padded batch of utterances of different
    lengths, each rendered as it would be alone (`_render_lengths`).

    Refused at construction: jitter_p != 0 with a mean-pooled quantized top
    level (one frame has no neighbour), use_gst with pooling_last: false (the
    reference hands the style layer a 3-D tensor there and fails), and
    whatever vqvae2.Encoder / vqvae2.Decoder refuse."""
    name = "vqvae2b.Model"

    def __init__(self, arch):
        super().__init__()
        levels = arch.get("levels", 3)
        if levels not in (1, 2, 3):
            raise ValueError(f"vqvae2b.Model: levels {levels} not in 1..3")
        use_gst = arch.get("use_gst", True) if levels > 1 else False
        use_ema = arch.get("use_ema", True)
        y_num, y_dim = arch.get("y_num", 10), arch.get("y_dim", 128)
        jitter_p = arch.get("jitter_p", 0.0)
        pooling_last = arch.get("pooling_last", True)
        if use_gst and not pooling_last:
            raise NotImplementedError("vqvae2b.Model: use_gst with pooling_last: false: the reference hands the style "
                                      "layer the un-pooled 3-D level there (vqvae2b.py:116-117) and fails")
        if jitter_p != 0 and pooling_last and not use_gst:
            raise NotImplementedError(f"vqvae2b.Model: jitter_p {jitter_p} with a mean-pooled quantized top level: its "
                                      "one frame has no neighbour (the reference indexes out of range, layers_vq.py:367)")
        dtype = arch.get("compute_dtype", "fp32")
        plain = EMAVectorQuantizer if use_ema else VectorQuantizer
        self.encoders = nn.ModuleList([Encoder(**arch[f"encoder.{i}"], compute_dtype=dtype) for i in range(levels)])
        self.quantizers = nn.ModuleList([
            (StyleTokenLayer if use_gst and i == levels - 1 else plain)(**arch[f"quantizer.{i}"])
            for i in range(levels)])
        self.decoders = nn.ModuleList([Decoder(**arch[f"decoder.{i}"], compute_dtype=dtype) for i in range(levels)])
        self.embeds = nn.ModuleList([Conditions(y_num, y_dim, normalize=False) for _ in range(levels)])
        self.final_decoder = Decoder(**arch["final_decoder"], compute_dtype=dtype)
        self.jitter = Jitter(probability=jitter_p)
        if self.final_decoder.cond_ch:
            raise ValueError(f"vqvae2b.Model: final_decoder has cond_channels {self.final_decoder.cond_ch}; the model "
                             "calls it without conditioning (vqvae2b.py:135), set cond_channels: 0")
        if any(not d.cond_ch for d in self.decoders):
            raise ValueError("vqvae2b.Model: every level decoder is conditioned on its speaker embedding; "
                             "cond_channels must equal y_dim")
        width = sum(d.final_ch for d in self.decoders)
        if width != self.final_decoder.layers[0].cin:
            raise ValueError(f"vqvae2b.Model: the level decoders' final_channels sum to {width}, final_decoder's first "
                             f"in_channels is {self.final_decoder.layers[0].cin}")
        self.beta = arch.get("beta", 0.01)
        self.pooling_last = pooling_last
        self.upsample_last = arch.get("upsample_last", False)
        self.levels, self.use_gst, self.use_ema = levels, use_gst, use_ema
        self.compute_dtype = dtype

    def forward(self, input):
        """(x (B, mel, T), y_idx (B, 1)) -> (xhat (B, mel, T), loss, loss dict).
        The loss is x_loss + sum z_qut + beta * sum z_enc; the dict holds Total,
        VQ loss, X like, then per quantized level k (bottom-up) the quantizer's
        detail and quanti_err.k, as vqvae2a.Model.forward."""
        x, y_idx = input
        x = self._check(x)
        z_vqs, ys, level_losses, enc_losses, named = [], [], [], [], []
        feat = x
        for i in range(self.levels):
            z, feat = self.encoders[i](feat)
            q = self.quantizers[i]
            if self._is_style(i):  # pooling_last holds: the fused pool + attention
                z_vq = q.pool_forward(z).unsqueeze(-1)
            else:
                if self._pooled(i):
                    z = mean_pool(z)
                z_vq, lvl, _, z_enc, detail = q(z, loss_weights=(1.0, self.beta), src_t=self.jitter.draw(z.shape[2]))
                named += self._detail_scalars(len(level_losses), detail, z_enc)
                level_losses.append(lvl)
                enc_losses.append(z_enc)
            z_vqs.append(z_vq)
            ys.append(self.embeds[i](y_idx[..., :1]).reshape(x.shape[0], -1))  # (B, y_dim): one frame, never stretched
        xhat = decode_side(self.decoders, self.final_decoder, z_vqs, ys, x.shape[2], self.upsample_last)
        loss, losses = self._loss(xhat, x, level_losses, enc_losses, named)
        return xhat, loss, losses

    def _check_decode(self, zs, ys, time):
        """decode's validation on the host, before any libvqx launch of its own
        (one readback: the extremes of every index tensor).  Returns (zs, B, T)."""
        who = "vqvae2b.Model.decode"
        zs = list(zs)
        if len(zs) != self.levels or not all(torch.is_tensor(z) for z in zs):
            raise ValueError(f"{who}: zs must hold one tensor per level ({self.levels})")
        B = zs[0].shape[0]
        for i, z in enumerate(zs):
            if self._is_style(i):
                if z.dim() != 3 or not z.is_floating_point() or z.shape[1] != self.decoders[i].layers[0].cin:
                    raise ValueError(f"{who}: level {i} is a style level: a float (B, "
                                     f"{self.decoders[i].layers[0].cin}, T_i) tensor")
            elif z.dim() != 2 or z.dtype != torch.int64:
                raise ValueError(f"{who}: level {i} is a quantized level: int64 indices (B, T_i)")
            if z.shape[0] != B or z.shape[-1] < 1:
                raise ValueError(f"{who}: level {i} has shape {tuple(z.shape)}; level 0 has batch size {B}")
        if not torch.is_tensor(ys) or ys.dim() != 2 or tuple(ys.shape) != (B, self.levels) or ys.dtype != torch.int64:
            raise ValueError(f"{who}: ys must be int64 (B, levels) = ({B}, {self.levels}) speaker indices, one column "
                             "per level")
        T = int(time) if time else max(z.shape[-1] for z in zs)
        for i, z in enumerate(zs):
            try:
                src_index(T, z.shape[-1])
            except ValueError:
                raise ValueError(f"{who}: level {i} has {z.shape[-1]} frames, which do not stretch to T = {T} "
                                 "(1 <= T_i <= T)") from None
        lo, hi = self._check_index_ranges(who, zs, ys)
        y_num = self.embeds[0].cond_num
        if lo < 0 or hi >= y_num:
            raise ValueError(f"{who}: ys has speakers in {lo}..{hi}, the model has 0..{y_num - 1}")
        return zs, B, T

    def _render_lengths(self, levels, ys, B, lens, lv):
        """decode's launches for a padded batch: every level decoder's input
        from one vqx_codes_upsample_cat_len launch (at the level's own rate
        with upsample_last, else at x's), the join one such launch over the L
        f32 outputs, the final decoder and the output layout change, each
        utterance with its own stretch factors."""
        dt, dev = DT[self.compute_dtype], ys[0].device
        outs, out_lens, T = [], [], max(lens)
        for i in range(self.levels):
            run = lv[i] if self.upsample_last else lens
            Td, dec = max(run), self.decoders[i]
            rows = torch.empty(B * Td, dec.layers[0].cin, device=dev, dtype=dt)
            ops.codes_upsample_cat_len([levels[i]], B, Td, run, [lv[i]], rows)
            outs.append(dec.forward_rows(rows, B, Td, [ys[i]], lengths=run))
            out_lens.append(run)
        joined = torch.empty(B * T, sum(o.shape[1] for o in outs), device=dev, dtype=dt)
        ops.codes_upsample_cat_len(outs, B, T, lens, out_lens, joined)
        xhat = self.final_decoder.forward_rows(joined, B, T, None, lengths=lens)
        return ops.ntc_to_nct_len(xhat, T, lens, torch.empty(B, xhat.shape[1], T, device=dev, dtype=F32))

    def _decode_lengths(self, zs, ys, time, lengths):
        """decode for a padded batch: utterance b has lengths[b] output frames."""
        who = "vqvae2b.Model.decode"
        if not torch.is_tensor(ys) or ys.dim() != 2:
            raise ValueError(f"{who}: ys must be int64 (B, levels) speaker indices")
        lens = list(ops.len_array(lengths, ys.shape[0], f"{who} lengths"))
        if min(lens) < 1:
            raise ValueError(f"{who}: lengths[{lens.index(min(lens))}] = {min(lens)} is not a frame count")
        lv = self.level_lengths(lens)
        if time is not None and int(time) != max(lens):
            raise ValueError(f"{who}: with lengths the output has max(lengths) = {max(lens)} frames; time = {time}")
        zs = list(zs)
        for i, z in enumerate(zs[:self.levels]):
            if torch.is_tensor(z) and z.dim() >= 2 and z.shape[-1] != max(lv[i]):
                raise ValueError(f"{who}: level {i} holds {z.shape[-1]} frames, encode(x, lengths) gives {max(lv[i])}")
        zs, B, T = self._check_decode(zs, ys, max(lens))
        if not all(z.is_cuda for z in zs) or not ys.is_cuda:
            raise self._off_device()
        with torch.no_grad():
            levels = [zs[i].float().reshape(B, -1) if self._is_style(i) else self._index_level(i, zs[i])
                      for i in range(self.levels)]
            return self._render_lengths(levels, self._speaker_rows(ys), B, lens, lv)

    def decode(self, input, time=None, lengths=None):
        """((zs, ys (B, levels)), time) -> xhat (B, mel, T) (vqvae2b.py:73-90):
        zs as `encode` returns them, level i rendered by decoders[i] with the
        speaker ys[:, i].  T = `time`, else the longest level.  A quantized
        level goes from its indices to its decoder's frame-major input in one
        vqx_codes_upsample_cat launch (a normalised codebook is normalised on
        the fly); everything up to xhat stays frame-major.  Under no_grad;
        writes no parameter or buffer.  Bad arguments raise ValueError.

        lengths (host values, as encode): zs are the codes of a padded batch
        as encode(x, lengths) returns them; xhat is (B, mel, max(lengths)) with
        zeros at t >= lengths[b], each utterance rendered as it would be alone;
        `time`, if given, must equal max(lengths)."""
        zs, ys = input
        if lengths is not None:
            return self._decode_lengths(zs, ys, time, lengths)
        zs, B, T = self._check_decode(zs, ys, time)
        if not all(z.is_cuda for z in zs) or not ys.is_cuda:
            raise self._off_device()
        dt = DT[self.compute_dtype]
        with torch.no_grad():
            outs = []
            for i in range(self.levels):
                z, dec = zs[i], self.decoders[i]
                Td = z.shape[-1] if self.upsample_last else T
                if self._is_style(i):
                    level = z.float().reshape(B, -1) if z.shape[2] == 1 else to_rows(z)
                else:
                    level = self._index_level(i, z)
                rows = torch.empty(B * Td, dec.layers[0].cin, device=ys.device, dtype=dt)
                ops.codes_upsample_cat([level], B, Td, rows)
                y = self.embeds[i](ys[:, i:i + 1]).reshape(B, -1)
                outs.append(dec.forward_rows(rows, B, Td, [y]))
            joined = torch.empty(B * T, sum(o.shape[1] for o in outs), device=ys.device, dtype=dt)
            ops.upsample_cat_fwd(outs, B, T, joined)
            return to_nct(self.final_decoder.forward_rows(joined, B, T, None), B, T)

    def infer(self, input, lengths=None):
        """(x, ys (B, levels)) -> decode((encode(x), ys)) (vqvae2b.py:93-97);
        with lengths, decode((encode(x, lengths), ys), lengths=lengths)."""
        x, ys = input
        if lengths is not None:
            B = x.shape[0] if torch.is_tensor(x) and x.dim() == 3 else None
            if not torch.is_tensor(ys) or ys.dim() != 2 or tuple(ys.shape) != (B, self.levels) or ys.dtype != torch.int64:
                raise ValueError(f"vqvae2b.Model.infer: ys must be int64 (B, levels) = ({B}, {self.levels}) speaker "
                                 "indices, one column per level")
            return self.decode((self.encode(x, lengths), ys), lengths=lengths)
        return self.decode((self.encode(x), ys))
