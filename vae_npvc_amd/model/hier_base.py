"""What the three hierarchical models (vqvae2, vqvae2a, vqvae2b `Model`) share.

`HierModelBase` registers no submodule and sets no parameter: every `Model`
assigns its own ModuleLists, in the reference's order, which is the order of
its parameters and state_dict keys.  The base reads `levels`, `use_gst`,
`encoders`, `quantizers` (through the `_quantizer` hook) and, for `encode`,
`pooling_last`; `name` prefixes the messages.

vqvae2a and vqvae2b convert a padded batch of utterances of different lengths
(`lengths=`) on frame-major rows from the input's layout change to the
output's: `_encode_lengths` here, `_render_lengths` in each model.  The lengths
are host values and travel in kernel arguments (csrc/vqx_varlen.hip).
"""
import functools
import math

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from .hier_common import DT, F32, LogLossFn, mean_pool
from .hier_encoder import stage_frames, total_scale
from .layers import WNConv1d
from .layers_vq import VectorQuantizer
from .resample import ResampleConv1d


class HierModelBase(nn.Module):
    name = "HierModelBase"  # "vqvae2.Model", ...: the prefix of the messages

    def __init__(self):
        super().__init__()
        self._engine = None

    def engine(self, device=None):
        """The optimizer engine of this package's Trainer (engine/autograd_step.py:
        flat parameters and moments, multi-tensor clip + Adam / RAdam; data
        parallel over a parallel.ddp.Comm through its attach_comm), built once
        per device and rebuilt when the parameters were moved."""
        dev = device if device is not None else next(self.parameters()).device
        dev = torch.device(dev)
        if dev.type != "cuda":
            raise RuntimeError(f"{self.name} runs on the MI355X only (libvqx); move it with .cuda()")
        e = self._engine
        if e is None or e.device != dev or not e.params_intact():
            from ..engine.autograd_step import AutogradEngine
            e = self._engine = AutogradEngine(self, dev)
        return e

    def remove_weight_norm(self):
        """vqvae2.py:146-156: bake w = g*v/||v|| into a plain `weight` on every conv that has weight norm."""
        for m in self.modules():
            if isinstance(m, (WNConv1d, ResampleConv1d)) and m.has_weight_norm:
                m.remove_weight_norm()
        self._engine = None  # the parameter list changed

    # ------------------------------------------------------------ hooks
    def _quantizer(self, i):
        return self.quantizers[i]

    def _is_style(self, i):
        return self.use_gst and i == self.levels - 1

    def _pooled(self, i):
        return self.pooling_last and i == self.levels - 1

    def _attend(self, i, z):
        """Level i's encoder output z (B, C, T_i) as its pool / quantizer reads it (vqvae2a: attention.{i})."""
        return z

    def _attend_rows(self, i, z, B, T, lens):
        """_attend on frame-major f32 rows z [B*T, C] of a padded batch whose
        utterance b owns rows t < lens[b]; the other rows are undefined."""
        return z

    # ------------------------------------------------------------ shared pieces
    def _off_device(self):
        return L.VqxError(f"{self.name} runs on the MI355X only (libvqx); move it and its inputs with .cuda()")

    def _check(self, x):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.encoders[0].in_ch:
            raise ValueError(f"{self.name}: x must be (B, {self.encoders[0].in_ch}, T)")
        if not x.is_cuda:
            raise self._off_device()
        return x.float().contiguous()

    @staticmethod
    def _detail_scalars(k, detail, z_enc):
        """Quantized level k's entries of the loss dict: the quantizer's whole detail, then quanti_err.k."""
        return [(f"{key}.{k}", val) for key, val in dict(detail, quanti_err=z_enc).items()]

    def _loss(self, xhat, x, level_losses, enc_losses, named):
        """The loss x_loss + sum of the level losses and the loss dict: Total,
        VQ loss (the sum of enc_losses), X like, then `named` = [(key, scalar)]
        in order, from one readback of the stacked scalars."""
        x_loss = LogLossFn.apply(xhat, x)
        loss = x_loss
        for lvl in level_losses:
            loss = loss + lvl
        vq = enc_losses[0]
        for t in enc_losses[1:]:
            vq = vq + t
        named = [("Total", loss), ("VQ loss", vq), ("X like", x_loss), *named]
        host = torch.stack([s.detach().reshape(()) for _, s in named]).tolist()  # the step's one readback
        return loss, dict(zip([n for n, _ in named], host))

    def _index_level(self, i, idx):
        """Level i's int64 indices as a level of vqx_codes_upsample_cat:
        (indices, codebook, normalise on the fly)."""
        idx = idx.contiguous()
        if idx.data_ptr() % 16:  # a slice of a longer index tensor: the kernel reads aligned pointers
            idx = idx.clone()
        q = self._quantizer(i)
        return idx, q.embeddings.detach(), bool(getattr(q, "normalize", False))

    def _check_index_ranges(self, who, codes, *more):
        """ValueError unless every quantized level of `codes` holds indices of
        its codebook: one aminmax per index tensor, one stacked readback, which
        also brings the extremes of the tensors in `more`: returned as
        [min, max, ...]."""
        quantized = [i for i in range(self.levels) if not self._is_style(i) and codes[i].numel()]
        spans = [v for t in (*[codes[i] for i in quantized], *more) for v in torch.aminmax(t)]
        if not spans:
            return []
        ext = torch.stack(spans).tolist()  # the one readback
        for k, i in enumerate(quantized):
            K = self._quantizer(i).z_num
            if ext[2 * k] < 0 or ext[2 * k + 1] >= K:
                raise ValueError(f"{who}: level {i} has indices in {ext[2 * k]}..{ext[2 * k + 1]}, the codebook "
                                 f"holds 0..{K - 1}")
        return ext[2 * len(quantized):]

    # ------------------------------------------------------------ vqvae2a and vqvae2b
    def _enc_lengths(self, lengths):
        """[[frames of utterance b that encoders[i] gives] for every level i], before a top level is pooled."""
        lengths = lens = list(ops.len_array(lengths, what=f"{self.name} lengths"))
        out = []
        for i, enc in enumerate(self.encoders):
            for k in enc.stage_index:
                lens = [stage_frames(n, getattr(enc.encode[k], "scale", 1)) for n in lens]
            if min(lens) < 1:
                b = lens.index(min(lens))
                raise ValueError(f"{self.name}: utterance {b} of {lengths[b]} frames leaves level {i} without a frame")
            out.append(lens)
        return out

    def level_lengths(self, lengths):
        """Host arithmetic: [[frames of utterance b at level i] for every level i]
        for utterances of `lengths` input frames (level 0 first; the strided
        stage convs floor, stage_frames; a mean-pooled or style top level has
        one frame).  ValueError when an utterance leaves a level without a frame."""
        lv = self._enc_lengths(lengths)
        top = self.levels - 1
        if self._is_style(top) or self._pooled(top):
            lv[top] = [1] * len(lv[top])
        return lv

    def _batch_lengths(self, lengths, x, who):
        """The host checks of a padded batch x (B, mel, T) with `lengths`:
        (lengths as a list, level_lengths, the encoders' own lengths)."""
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.encoders[0].in_ch:
            raise ValueError(f"{who}: x must be (B, {self.encoders[0].in_ch}, T)")
        lens = list(ops.len_array(lengths, x.shape[0], f"{who} lengths"))
        if min(lens) < 1 or max(lens) > x.shape[2]:
            b = next(b for b, n in enumerate(lens) if not 1 <= n <= x.shape[2])
            raise ValueError(f"{who}: lengths[{b}] = {lens[b]} outside 1..T = {x.shape[2]}")
        return lens, self.level_lengths(lens), self._enc_lengths(lens)

    def _encode_lengths(self, x, lens, lv, enc_len):
        """encode for a padded batch (under no_grad; lens, lv, enc_len:
        _batch_lengths): (codes as encode returns them, the levels as
        vqx_codes_upsample_cat_len takes them: the indices with their codebook,
        or the style rows (B, F))."""
        B, mel, T = x.shape
        dt, dev = DT[self.compute_dtype], x.device
        e = functools.partial(torch.empty, device=dev)
        gran = math.prod(total_scale(enc) for enc in self.encoders)
        Tp = -(-max(lens) // gran) * gran  # every level's padded length divides exactly
        if T > Tp:
            x = x[:, :, :max(lens)]
        # the one input layout change: zeros from each utterance's end, x's padding never read
        feat = ops.nct_to_ntc_pad_len(x.float().contiguous(), Tp, lens, e(B * Tp, mel, dtype=dt))
        codes, levels, Ti, lin = [], [], Tp, lens
        for i in range(self.levels):
            z, feat, Ti = self.encoders[i].forward_rows(feat, B, Ti, lengths=lin)
            lin = enc_len[i]
            z = self._attend_rows(i, z, B, Ti, lin)
            q = self._quantizer(i)
            if self._is_style(i):
                style = q.pool_rows(ops.segment_mean(z, Ti, lin, e(B, z.shape[1], dtype=F32)), 1)
                codes.append(style.unsqueeze(-1))
                levels.append(style)
            elif self._pooled(i):
                mean = ops.segment_mean(z, Ti, lin, e(B, z.shape[1], dtype=F32))
                idx = q.encode(mean.view(B, 1, -1), time_last=False)
                codes.append(idx)
                levels.append(self._index_level(i, idx))
            else:
                idx = q.encode(z.view(B, Ti, -1), time_last=False)  # tail entries: whatever the pad rows gave
                codes.append(ops.index_mask_len(idx, lin, e(B, max(lin), dtype=torch.int64)))
                levels.append(self._index_level(i, codes[-1]))  # max(lin) frames: no longer than a decoder's rows
        return codes, levels

    def _embed(self, i):
        """Level i's speaker embedding."""
        return self.embeds[i]

    def _speaker_rows(self, ys):
        """ys (B, levels) speaker indices -> [the (B, y_dim) speaker rows of level i]."""
        return [self._embed(i)(ys[:, i:i + 1]).reshape(ys.shape[0], -1) for i in range(self.levels)]

    def _render_lengths(self, levels, ys, B, lens, lv):
        """The decode side of a padded batch, under no_grad: `levels` as
        _encode_lengths gives them, ys the speaker rows per level -> xhat
        (B, mel, max(lens)), zeros from each utterance's end."""
        raise NotImplementedError

    def encode(self, input, lengths=None):
        """One entry per level (vqvae2a.py:72-91, vqvae2b.py:52-70): int64
        indices (B, T_i) of a quantized level, the style embedding (B, F, 1) of
        a style-token top.  Without gradients; writes nothing (a normalised
        codebook is normalised on the fly).

        lengths (a host sequence of ints or a 1-D CPU int tensor, never a
        device tensor): a padded batch, utterance b owning frames
        t < lengths[b] <= T; whatever x holds from lengths[b] on is ignored,
        NaN included.  A quantized level comes back as int64
        (B, max_b len_i[b]) with 0 at the padded positions (level_lengths gives
        len_i), a mean-pooled one as (B, 1), the style level as (B, F, 1).
        Each utterance gets the codes it would get alone."""
        x = input[0] if isinstance(input, (list, tuple)) else input
        if lengths is not None:  # validated on the host before the device is touched
            batch = self._batch_lengths(lengths, x, f"{self.name}.encode")
            if not x.is_cuda:
                raise self._off_device()
            with torch.no_grad():
                return self._encode_lengths(x, *batch)[0]
        x = self._check(x)
        zs = []
        with torch.no_grad():
            for i in range(self.levels):
                z, x = self.encoders[i](x)
                z = self._attend(i, z)
                q = self._quantizer(i)
                if self._is_style(i):
                    zs.append(q.pool_forward(z).unsqueeze(-1))
                else:
                    if self._pooled(i):
                        z = mean_pool(z)
                    zs.append(q.encode(z))
        return zs

    def convert(self, input, lengths=None):
        """(x (B, mel, T), y_idx (B, 1)) -> the xhat of the eval-mode forward,
        without gradients.  A normalised codebook, which every forward
        renormalises in place, gets its bits back, so no parameter or buffer
        changes (an EMA codebook is neither initialised nor updated in eval mode).

        lengths (host values, as encode): a padded batch -> (B, mel,
        max(lengths)) f32 with exact zeros at t >= lengths[b], every utterance
        rendered as the eval-mode forward would render it alone (its own
        GroupNorm statistics, conv padding, pools and stretch factors), on
        frame-major rows throughout; nothing is written, whatever the model's
        mode."""
        if lengths is not None:
            who = f"{self.name}.convert"
            x, y_idx = input
            batch = self._batch_lengths(lengths, x, who)
            if not torch.is_tensor(y_idx) or y_idx.dim() != 2 or y_idx.shape[0] != x.shape[0] or y_idx.shape[1] < 1 \
                    or y_idx.dtype != torch.int64:
                raise ValueError(f"{who}: y_idx must be int64 (B, 1) speaker indices with B = {x.shape[0]}")
            if not x.is_cuda or not y_idx.is_cuda:
                raise self._off_device()
            with torch.no_grad():
                _, levels = self._encode_lengths(x, *batch)
                ys = self._speaker_rows(y_idx[:, :1].expand(-1, self.levels))
                return self._render_lengths(levels, ys, x.shape[0], batch[0], batch[1])
        mutated = [q.embeddings for q in self.modules() if isinstance(q, VectorQuantizer) and q.normalize]
        saved = [e.detach().clone() for e in mutated]
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                xhat = self.forward(input)[0]
                for e, s in zip(mutated, saved):
                    e.copy_(s)
        finally:
            self.train(was_training)
        return xhat
