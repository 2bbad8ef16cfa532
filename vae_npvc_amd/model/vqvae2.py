"""The hierarchical model (reference model/vqvae2.py, recipe egs/vcc20/vae2) on
the MI355X, for `model_type: vae_npvc_amd.model.vqvae2`: `Model`, with
training and conversion.

Its blocks live in one module per topic and are re-exported here: `Encoder`
(hier_encoder.py), `Decoder` (hier_decoder.py), level upsampling and its
concatenation `upsample`, `upsample_cat`, `src_index`, `choose_tc`
(hier_common.py, with the fused log-loss).  What `Model` shares with
vqvae2a.Model and vqvae2b.Model is `HierModelBase` (hier_base.py).  There is
no CPU path.
"""
import functools
import math

import torch
import torch.nn as nn

from .. import ops
from .hier_base import HierModelBase
from .hier_common import DT, F32, choose_tc, src_index, to_nct, to_rows, upsample, upsample_cat
from .hier_decoder import Decoder
from .hier_encoder import Encoder, stage_frames, total_scale
from .layers import Conditions
from .layers_gst import StyleTokenLayer
from .layers_vq import Jitter, VectorQuantizer

__all__ = ["Model", "Encoder", "Decoder", "upsample", "upsample_cat", "src_index", "choose_tc"]


class Model(HierModelBase):
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
    name = "vqvae2.Model"

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

    def forward(self, input):
        """(x (B, mel, T), y_idx (B, 1)) -> (xhat (B, mel, T), loss, loss dict:
        Total, VQ loss, X like, then entropy.k and quanti_err.k per quantized
        level k in the order the levels run, top-down)."""
        x, y_idx = input
        if not x.is_cuda:
            raise self._off_device()
        x = x.float().contiguous()
        y = self.embeds(y_idx[..., :1]).transpose(1, 2)  # (B, y_dim, 1)
        # hierarchical encode: level i reads level i-1's feature map
        z_levels, feat = [], x
        for enc in self.encoders:
            z, feat = enc(feat)
            z_levels.append(z)
        # quantize and decode from the top; z_vqs holds the quantized levels at their own rates, top first
        z_vqs, level_losses, enc_losses, named = [], [], [], []
        z = z_levels.pop()
        for i in reversed(range(self.levels)):
            if self._is_style(i):
                z_vq = self.quantizers[i].pool_forward(z).unsqueeze(-1)
            else:
                z_vq, lvl, _, z_enc, detail = self.quantizers[i](z, loss_weights=(1.0, self.beta))
                k = len(level_losses)
                level_losses.append(lvl)
                enc_losses.append(z_enc)
                named += [(f"entropy.{k}", detail["entropy"]), (f"quanti_err.{k}", z_enc)]
            z_vqs.append(z_vq)
            if i > 0:
                z = self.decoders[i]((z_levels.pop(), list(z_vqs)))
        xhat = self.decoders[0]((upsample_cat(z_vqs, x.shape[2]), [y]))
        loss, losses = self._loss(xhat, x, level_losses, enc_losses, named)
        return xhat, loss, losses

    # ------------------------------------------------------------ conversion
    # The reference defines conversion through forward: xhat of forward((x, y')) is x
    # rendered with speaker y'.  y enters decoders[0] alone, so the codes of every
    # level depend on x only: analyze gives them, synthesize renders them.
    def level_lengths(self, lengths):
        """Host arithmetic: [[frames of utterance b at level i] for every level i]
        for utterances of `lengths` input frames (level 0 first; the strided
        stage convs floor, stage_frames).  ValueError when an utterance
        leaves a level without a frame."""
        lengths = lens = list(ops.len_array(lengths, what="vqvae2.Model lengths"))
        out = []
        for i, enc in enumerate(self.encoders):
            for k in enc.stage_index:
                lens = [stage_frames(n, getattr(enc.encode[k], "scale", 1)) for n in lens]
            if min(lens) < 1:
                b = lens.index(min(lens))
                raise ValueError(f"vqvae2.Model: utterance {b} of {lengths[b]} frames leaves level {i} without a frame")
            out.append(lens)
        return out

    def _batch_lengths(self, lengths, B, who):
        """(lengths as a list, level_lengths, the padded level-0 frame count's granule)."""
        lens = list(ops.len_array(lengths, B, f"{who} lengths"))
        return lens, self.level_lengths(lens), math.prod(total_scale(enc) for enc in self.encoders)

    def _render(self, rows, y_idx, B, T, lengths=None):
        """decoders[0] on its frame-major input `rows` with the speaker row as conditioning -> xhat (B, mel, T)."""
        y = self.embeds(y_idx[..., :1]).reshape(B, -1)
        return to_nct(self.decoders[0].forward_rows(rows, B, T, [y], lengths=lengths), B, T)

    def _analyze_lengths(self, x, lens, lv, gran):
        """analyze for a padded batch: utterance b owns frames t < lens[b]
        (lens, lv, gran: _batch_lengths, validated by analyze)."""
        B, mel, T = x.shape
        with torch.no_grad():
            dt, dev = DT[self.compute_dtype], x.device
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
                    cond.append(self._index_level(i, idx))
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
            batch = self._batch_lengths(lengths, x.shape[0], "vqvae2.Model.analyze")
            if max(batch[0]) > x.shape[2]:
                raise ValueError(f"vqvae2.Model.analyze: lengths up to {max(batch[0])} exceed x's {x.shape[2]} frames")
        if not x.is_cuda:
            raise self._off_device()
        if lengths is not None:
            return self._analyze_lengths(x, *batch)
        with torch.no_grad():
            B, _, T = x.shape
            dt = DT[self.compute_dtype]
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
                        cond.append(ops.codes_upsample_cat([self._index_level(i, idx)], B, Ti,
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
        B, width = codes[0].shape[0], 0
        for i, c in enumerate(codes):
            if self._is_style(i):
                if c.dim() != 3 or not c.is_floating_point() or c.shape[1] % 4:
                    raise ValueError(f"{who}: level {i} is a style level: a float (B, F, T_i) tensor, F a multiple of 4")
                width += c.shape[1]
            else:
                if c.dim() != 2 or c.dtype != torch.int64:
                    raise ValueError(f"{who}: level {i} is a quantized level: int64 indices (B, T_i)")
                width += self.quantizers[i].z_dim
            if c.shape[0] != B:
                raise ValueError(f"{who}: level {i} has batch size {c.shape[0]}, level 0 has {B}")
        if not torch.is_tensor(y_idx) or y_idx.dim() != 2 or y_idx.shape[0] != B:
            raise ValueError(f"{who}: y_idx must be (B, 1) speaker indices with B = {B}")
        if codes[0].dim() != 2 and time is None:
            raise ValueError(f"{who}: give `time` when level 0 is not an index tensor")
        T = int(time) if time is not None else codes[0].shape[1] * total_scale(self.encoders[0])
        for i, c in enumerate(codes):
            try:
                src_index(T, c.shape[-1])
            except ValueError:
                raise ValueError(f"{who}: level {i} has {c.shape[-1]} frames, which do not stretch to T = {T} "
                                 "(1 <= T_i <= T)") from None
        want = self.decoders[0].layers[0].cin
        if width != want:
            raise ValueError(f"{who}: the levels' channels sum to {width}, decoders[0] takes {want}")
        self._check_index_ranges(who, codes)
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
            raise self._off_device()
        with torch.no_grad():
            levels, level_len = [], []
            for i in reversed(range(self.levels)):
                if self._is_style(i):
                    levels.append(codes[i].float().reshape(B, -1))
                    level_len.append([1] * B)
                else:
                    levels.append(self._index_level(i, codes[i]))
                    level_len.append(lv[i])
            rows = torch.empty(B * T, self.decoders[0].layers[0].cin, device=y_idx.device, dtype=DT[self.compute_dtype])
            ops.codes_upsample_cat_len(levels, B, T, lens, level_len, rows)
            return self._render(rows, y_idx, B, T, lengths=lens)

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
            raise self._off_device()
        with torch.no_grad():
            levels = []
            for i in reversed(range(self.levels)):
                c = codes[i]
                if self._is_style(i):
                    levels.append(c.float().reshape(B, -1) if c.shape[2] == 1 else to_rows(c))
                else:
                    levels.append(self._index_level(i, c))
            rows = torch.empty(B * T, self.decoders[0].layers[0].cin, device=y_idx.device, dtype=DT[self.compute_dtype])
            ops.codes_upsample_cat(levels, B, T, rows)
            return self._render(rows, y_idx, B, T)

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
