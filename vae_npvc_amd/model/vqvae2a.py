"""The reworked hierarchical model (reference model/vqvae2a.py:11-238) on the
MI355X, for `model_type: vae_npvc_amd.model.vqvae2a`.

Every level quantizes its own encoder's output directly (an EMA codebook by
default, jitter on the quantized frames), the decoders are chained top-down,
each level has its own speaker embedding, and one quantizer / one embedding
may be shared by all levels.  The blocks are this package's: `vqvae2.Encoder`,
`vqvae2.Decoder`, `upsample_cat`, `StyleTokenLayer`, the two quantizers of
layers_vq.py, `Conditions` and the fused log-loss, composed under torch
autograd as `vqvae2.Model` composes them.  There is no CPU path.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .layers import Conditions
from .layers_gst import StyleTokenLayer
from .layers_vq import EMAVectorQuantizer, Jitter, VectorQuantizer
from .vqvae2 import F32, Decoder, Encoder, _LogLossFn, _to_nct, _to_rows, upsample_cat
from .vqvae2 import Model as _Vqvae2Model

_EMA_KEYS = ("entropy", "used_curr", "usage", "diff_emb")


class _MeanPoolFn(torch.autograd.Function):
    """torch.mean(z, dim=-1, keepdim=True) of z (B, C, T) (vqvae2a.py:145-146):
    the per-utterance column sums of vqx_upsample_cat_bwd (one level of one
    frame) times 1/T; the backward stretches g/T back over the T frames."""

    @staticmethod
    def forward(ctx, z):
        B, C, T = z.shape
        total = torch.empty(B, C, device=z.device, dtype=F32)
        ops.upsample_cat_bwd([total], B, T, _to_rows(z))
        ctx.dims = (B, C, T)
        return ops.scale_act_2d(total, torch.empty_like(total), 1.0 / T, L.PRO_NONE).view(B, C, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        B, C, T = ctx.dims
        rows = g.float().reshape(B, C).contiguous()
        rows = ops.scale_act_2d(rows, torch.empty_like(rows), 1.0 / T, L.PRO_NONE)
        out = ops.upsample_cat_fwd([rows], B, T, torch.empty(B * T, C, device=g.device, dtype=F32))
        return _to_nct(out, B, T)


def mean_pool(z):
    if not z.is_cuda:
        raise L.VqxError("vqvae2a.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
    return _MeanPoolFn.apply(z)


class Model(nn.Module):
    """`Model(arch)` with the reference's keys: levels (1..3), use_gst (forced
    false at levels == 1), use_ema, use_quantizers (false: one shared
    `quantizer`), use_embeds (false: one shared `embed`), pooling_last,
    upsample_last, jitter_p, beta, y_num, y_dim, encoder.{i}, decoder.{i},
    quantizer.{i} or quantizer (+ compute_dtype: fp32|bf16).  The module tree
    (encoders, decoders, quantizers | quantizer, embeds | embed, jitter), the
    parameter order and the state_dict keys are the reference's.

    forward((x, y_idx)) restates vqvae2a.py:131-193: xhat, loss, loss dict
    (one readback, at the end).  encode(x) restates :72-91.  convert((x, y_idx))
    is the xhat of the eval-mode forward, without gradients and without writing
    a parameter or buffer: the package's definition of conversion, which
    `decoder_type: vae_npvc_amd.decoder.hier` drives.

    Refused at construction: jitter_p != 0 with a mean-pooled quantized top
    level (one frame has no neighbour), a style-token top with a shared
    quantizer (the reference's forward hands the shared codebook a 2-D tensor
    there and fails), and whatever vqvae2.Encoder / vqvae2.Decoder refuse
    (resampling decoder stages among them)."""

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
        self.beta = arch.get("beta", 0.01)
        self.pooling_last = pooling_last
        self.upsample_last = arch.get("upsample_last", False)
        self.use_quantizers, self.use_embeds = use_quantizers, use_embeds
        self.levels, self.use_gst, self.use_ema = levels, use_gst, use_ema
        self.compute_dtype = dtype
        self._engine = None

    # the optimizer engine (flat parameters, multi-tensor clip + Adam / RAdam; data
    # parallel refused) and the weight-norm removal are vqvae2.Model's
    engine = _Vqvae2Model.engine
    remove_weight_norm = _Vqvae2Model.remove_weight_norm

    def _quantizer(self, i):
        return self.quantizers[i] if self.use_quantizers else self.quantizer

    def _is_style(self, i):
        return self.use_gst and i == self.levels - 1

    def _check(self, x):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.encoders[0].in_ch:
            raise ValueError(f"vqvae2a.Model: x must be (B, {self.encoders[0].in_ch}, T)")
        if not x.is_cuda:
            raise L.VqxError("vqvae2a.Model runs on the MI355X only (libvqx); move it and its inputs with .cuda()")
        return x.float().contiguous()

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
        z_vqs, level_losses, enc_losses, details = [], [], [], []
        feat = x
        for i in range(self.levels):
            z, feat = self.encoders[i](feat)
            q = self._quantizer(i)
            if self._is_style(i):  # pooling_last is forced: the fused pool + attention
                z_vq = q.pool_forward(z).unsqueeze(-1)
            else:
                if self.pooling_last and i == self.levels - 1:
                    z = mean_pool(z)
                z_vq, lvl, _, z_enc, detail = q(z, loss_weights=(1.0, self.beta), src_t=self.jitter.draw(z.shape[2]))
                level_losses.append(lvl)
                enc_losses.append(z_enc)
                details.append(dict(detail, quanti_err=z_enc))
            z_vqs.append(z_vq)
        # decode top-down (vqvae2a.py:160-179)
        xhat = None
        for i in reversed(range(self.levels)):
            cat = [z_vqs[i]] if xhat is None else [z_vqs[i], xhat]
            if i == self.levels - 1:
                time = z_vqs[i - 1].shape[-1]  # levels == 1: index -1 is the level itself, as in the reference
            elif i == 0:
                time = x.shape[-1]
            else:
                time = z_vqs[i - 1].shape[-1]
            embed = self.embeds[i] if self.use_embeds else self.embed
            y = embed(y_idx[..., :1]).transpose(1, 2)  # (B, y_dim, 1): a one-frame conditioning level, never stretched
            if self.upsample_last:
                xhat = self.decoders[i]((upsample_cat(cat, z_vqs[i].shape[-1]), [y]))
                if xhat.shape[-1] != time:
                    xhat = upsample_cat([xhat], time)
            else:
                xhat = self.decoders[i]((upsample_cat(cat, time), [y]))
        x_loss = _LogLossFn.apply(xhat, x)
        loss = x_loss
        for lvl in level_losses:
            loss = loss + lvl
        vq = enc_losses[0]
        for t in enc_losses[1:]:
            vq = vq + t
        names, scalars = ["Total", "VQ loss", "X like"], [loss.detach(), vq, x_loss.detach()]
        for k, d in enumerate(details):
            for key, val in d.items():
                names.append(f"{key}.{k}")
                scalars.append(val.detach())
        host = torch.stack([s.reshape(()) for s in scalars]).tolist()  # the step's one readback
        return xhat, loss, dict(zip(names, host))

    def encode(self, input):
        """vqvae2a.py:72-91: one entry per level, int64 indices (B, T_i) of a
        quantized level, the style embedding (B, F, 1) of a style-token top.
        Without gradients; writes nothing (a normalised codebook is normalised
        on the fly)."""
        x = input[0] if isinstance(input, (list, tuple)) else input
        x = self._check(x)
        zs = []
        with torch.no_grad():
            for i in range(self.levels):
                z, x = self.encoders[i](x)
                q = self._quantizer(i)
                if self._is_style(i):
                    zs.append(q.pool_forward(z).unsqueeze(-1))
                else:
                    if self.pooling_last and i == self.levels - 1:
                        z = mean_pool(z)
                    zs.append(q.encode(z))
        return zs

    def convert(self, input):
        """(x (B, mel, T), y_idx (B, 1)) -> the xhat of the eval-mode forward,
        without gradients.  A normalised codebook, which every forward
        renormalises in place, gets its bits back, so no parameter or buffer
        changes (an EMA codebook is neither initialised nor updated in eval mode)."""
        mutated = [q.embeddings for q in self.modules()
                   if isinstance(q, VectorQuantizer) and q.normalize]
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

    def decode(self, input, time=None):
        raise NotImplementedError("vqvae2a.Model.decode: the reference's version reads an undefined `x` at level 0 "
                                  "(vqvae2a.py:107); no semantics to restate.  Use convert((x, y_idx))")

    def infer(self, input):
        raise NotImplementedError("vqvae2a.Model.infer: built on decode, which reads an undefined `x` in the reference "
                                  "(vqvae2a.py:107,125-129).  Use convert((x, y_idx))")
