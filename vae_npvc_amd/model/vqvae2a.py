"""The reworked hierarchical model (reference model/vqvae2a.py:11-238) on the
MI355X, for `model_type: vae_npvc_amd.model.vqvae2a`.

Every level quantizes its own encoder's output directly (an EMA codebook by
default, jitter on the quantized frames), the decoders are chained top-down,
each level has its own speaker embedding, and one quantizer / one embedding
may be shared by all levels.  The blocks are this package's: the `Encoder`
and `Decoder` of the hierarchical models, `upsample_cat`, `mean_pool`,
`StyleTokenLayer`, the two quantizers of layers_vq.py, `Conditions` and the
fused log-loss, composed under torch autograd as `vqvae2.Model` composes
them; what the three models share is `HierModelBase`.  There is no CPU path.
"""
import torch
import torch.nn as nn

from .. import ops
from .hier_base import HierModelBase
from .hier_common import DT, F32, mean_pool, upsample_cat
from .hier_decoder import Decoder
from .hier_encoder import Encoder
from .layers import Conditions
from .layers_attn import SelfAttention
from .layers_gst import StyleTokenLayer
from .layers_vq import EMAVectorQuantizer, Jitter, VectorQuantizer

__all__ = ["Model", "mean_pool"]


class Model(HierModelBase):
    """`Model(arch)` with the reference's keys: levels (1..3), use_gst (forced
    false at levels == 1), use_ema, use_quantizers (false: one shared
    `quantizer`), use_embeds (false: one shared `embed`), pooling_last,
    upsample_last, jitter_p, beta, y_num, y_dim, encoder.{i}, decoder.{i},
    quantizer.{i} or quantizer (+ compute_dtype: fp32|bf16).  The module tree
    (encoders, decoders, quantizers | quantizer, embeds | embed, jitter), the
    parameter order and the state_dict keys are the reference's.

    This package's addition: `attention.{i}: {n_head: H}` puts a residual
    self-attention over level i's frames (layers_attn.SelfAttention, n_feat =
    encoder.{i}'s z_channels) between that level's encoder and its pool /
    quantizer: z = z + attention(z).  The layers are `attentions` (keys
    attentions.{i}.mha.linear_{q,k,v,out}.{weight,bias}), registered after every
    other module so that the order of the existing parameters does not move;
    without such a key `attentions` does not exist.

    forward((x, y_idx)) restates vqvae2a.py:131-193: xhat, loss, loss dict
    (one readback, at the end).  encode(x) restates :72-91.  convert((x, y_idx))
    is the xhat of the eval-mode forward, without gradients and without writing
    a parameter or buffer: the package's definition of conversion, which
    `decoder_type: vae_npvc_amd.decoder.hier` drives.  Both are HierModelBase's,
    and both take `lengths=` (host ints): a padded batch of utterances of
    different lengths, each converted as it would be alone, on frame-major rows
    throughout (`_render_lengths` is this model's decode side of it).

    Refused at construction: jitter_p != 0 with a mean-pooled quantized top
    level (one frame has no neighbour), a style-token top with a shared
    quantizer (the reference's forward hands the shared codebook a 2-D tensor
    there and fails), and whatever vqvae2.Encoder / vqvae2.Decoder refuse
    (resampling decoder stages among them)."""
    name = "vqvae2a.Model"

    def __init__(self, arch):
        super().__init__()
        levels = arch.get("levels", 3)
        if levels not in (1, 2, 3):
            raise ValueError(f"vqvae2a.Model: levels {levels} not in 1..3")
        use_gst = arch.get("use_gst", True) if levels > 1 else False
        use_ema = arch.get("use_ema", True)
        use_quantizers = arch.get("use_quantizers", True)
        use_embeds = arch.get("use_embeds", True)
        y_num, y_dim = arch.get("y_num", 10), arch.get("y_dim", 128)
        jitter_p = arch.get("jitter_p", 0.0)
        if levels > 1:
            pooling_last = True if use_gst else arch.get("pooling_last", True)
        else:
            pooling_last = False
        if use_gst and not use_quantizers:
            raise NotImplementedError("vqvae2a.Model: use_gst with use_quantizers: false: the reference calls the shared "
                                      "codebook on the pooled 2-D vector there (vqvae2a.py:148-150) and fails")
        if jitter_p != 0 and pooling_last and not use_gst:
            raise NotImplementedError(f"vqvae2a.Model: jitter_p {jitter_p} with a mean-pooled quantized top level: its "
                                      "one frame has no neighbour (the reference indexes out of range, layers_vq.py:367)")
        dtype = arch.get("compute_dtype", "fp32")
        self.encoders = nn.ModuleList([Encoder(**arch[f"encoder.{i}"], compute_dtype=dtype) for i in range(levels)])
        self.decoders = nn.ModuleList([Decoder(**arch[f"decoder.{i}"], compute_dtype=dtype) for i in range(levels)])
        plain = EMAVectorQuantizer if use_ema else VectorQuantizer
        if use_quantizers:
            self.quantizers = nn.ModuleList([
                (StyleTokenLayer if use_gst and i == levels - 1 else plain)(**arch[f"quantizer.{i}"])
                for i in range(levels)])
        else:
            self.quantizer = plain(**arch["quantizer"])
        if use_embeds:
            self.embeds = nn.ModuleList([Conditions(y_num, y_dim, normalize=False) for _ in range(levels)])
        else:
            self.embed = Conditions(y_num, y_dim, normalize=False)
        self.jitter = Jitter(probability=jitter_p)
        for key in arch:
            if str(key).startswith("attention.") and key not in [f"attention.{i}" for i in range(levels)]:
                raise ValueError(f"vqvae2a.Model: {key!r} names no level of 0..{levels - 1}")
        attentions = {}
        for i in range(levels):
            if f"attention.{i}" in arch:
                cfg = dict(arch[f"attention.{i}"])
                if set(cfg) - {"n_head", "dropout_rate"} or "n_head" not in cfg:
                    raise ValueError(f"vqvae2a.Model: attention.{i} takes n_head (and dropout_rate: 0), got {sorted(cfg)}")
                attentions[str(i)] = SelfAttention(self.encoders[i].z_proj.cout, compute_dtype=dtype, **cfg)
        if attentions:  # last: the order of the parameters above stays what it is without the key
            self.attentions = nn.ModuleDict(attentions)
        self.beta = arch.get("beta", 0.01)
        self.pooling_last = pooling_last
        self.upsample_last = arch.get("upsample_last", False)
        self.use_quantizers, self.use_embeds = use_quantizers, use_embeds
        self.levels, self.use_gst, self.use_ema = levels, use_gst, use_ema
        self.compute_dtype = dtype

    def _quantizer(self, i):
        return self.quantizers[i] if self.use_quantizers else self.quantizer

    def _attention(self, i):
        att = getattr(self, "attentions", None)
        return att[str(i)] if att is not None and str(i) in att else None

    def _attend(self, i, z):
        att = self._attention(i)
        return z if att is None else att(z, residual=True)

    def _attend_rows(self, i, z, B, T, lens):
        att = self._attention(i)
        return z if att is None else att.forward_rows(z, B, T, lengths=lens, residual=True)

    def forward(self, input):
        """(x (B, mel, T), y_idx (B, 1)) -> (xhat (B, mel, T), loss, loss dict).
        The loss is x_loss + sum z_qut + beta * sum z_enc; the dict holds Total,
        VQ loss, X like, then per quantized level k in the order they run
        (bottom-up) the quantizer's detail (entropy.k, used_curr.k, usage.k,
        diff_emb.k for an EMA codebook in training, entropy.k for a plain one)
        and quanti_err.k."""
        x, y_idx = input
        x = self._check(x)
        # encode bottom-up: level i reads level i-1's feature map and is quantized at once
        z_vqs, level_losses, enc_losses, named = [], [], [], []
        feat = x
        for i in range(self.levels):
            z, feat = self.encoders[i](feat)
            z = self._attend(i, z)
            q = self._quantizer(i)
            if self._is_style(i):  # pooling_last is forced: the fused pool + attention
                z_vq = q.pool_forward(z).unsqueeze(-1)
            else:
                if self._pooled(i):
                    z = mean_pool(z)
                z_vq, lvl, _, z_enc, detail = q(z, loss_weights=(1.0, self.beta), src_t=self.jitter.draw(z.shape[2]))
                named += self._detail_scalars(len(level_losses), detail, z_enc)
                level_losses.append(lvl)
                enc_losses.append(z_enc)
            z_vqs.append(z_vq)
        # decode top-down (vqvae2a.py:160-179)
        xhat = None
        for i in reversed(range(self.levels)):
            cat = [z_vqs[i]] if xhat is None else [z_vqs[i], xhat]
            # the level below's frames, x's at the bottom (levels == 1: index -1 is the level itself, as in the reference)
            time = x.shape[-1] if i == 0 and self.levels > 1 else z_vqs[i - 1].shape[-1]
            embed = self.embeds[i] if self.use_embeds else self.embed
            y = embed(y_idx[..., :1]).transpose(1, 2)  # (B, y_dim, 1): a one-frame conditioning level, never stretched
            if self.upsample_last:
                xhat = self.decoders[i]((upsample_cat(cat, z_vqs[i].shape[-1]), [y]))
                if xhat.shape[-1] != time:
                    xhat = upsample_cat([xhat], time)
            else:
                xhat = self.decoders[i]((upsample_cat(cat, time), [y]))
        loss, losses = self._loss(xhat, x, level_losses, enc_losses, named)
        return xhat, loss, losses

    def _embed(self, i):
        return self.embeds[i] if self.use_embeds else self.embed

    def _render_lengths(self, levels, ys, B, lens, lv):
        """forward's top-down chain for a padded batch: decoder i's frame-major
        input is one vqx_codes_upsample_cat_len launch over [level i's indices
        (or the style rows), the upper decoder's f32 output rows], each
        utterance stretched by its own factors; upsample_last leaves a
        decoder's output at its own rate, and the launch that reads it next
        stretches it (the bottom one by a launch of its own)."""
        dt, dev = DT[self.compute_dtype], ys[0].device
        out, out_len = None, None
        for i in reversed(range(self.levels)):
            # the frames the reference calls `time`: the level below's, x's at the bottom (levels == 1: the level's own)
            time = lens if i == 0 and self.levels > 1 else lv[i - 1]
            run = lv[i] if self.upsample_last else time
            cat, cat_len = ([levels[i]], [lv[i]]) if out is None else ([levels[i], out], [lv[i], out_len])
            Td, dec = max(run), self.decoders[i]
            rows = torch.empty(B * Td, dec.layers[0].cin, device=dev, dtype=dt)
            ops.codes_upsample_cat_len(cat, B, Td, run, cat_len, rows)
            out, out_len = dec.forward_rows(rows, B, Td, [ys[i]], lengths=run), run
        T = max(time)
        if out_len != time:  # upsample_last: the bottom decoder's output, stretched to x's frames
            out = ops.codes_upsample_cat_len([out], B, T, time, [out_len],
                                             torch.empty(B * T, out.shape[1], device=dev, dtype=F32))
        return ops.ntc_to_nct_len(out, T, time, torch.empty(B, out.shape[1], T, device=dev, dtype=F32))

    def decode(self, input, time=None):
        raise NotImplementedError("vqvae2a.Model.decode: the reference's version reads an undefined `x` at level 0 "
                                  "(vqvae2a.py:107); no semantics to restate.  Use convert((x, y_idx))")

    def infer(self, input):
        raise NotImplementedError("vqvae2a.Model.infer: built on decode, which reads an undefined `x` in the reference "
                                  "(vqvae2a.py:107,125-129).  Use convert((x, y_idx))")
