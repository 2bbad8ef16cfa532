"""What the three hierarchical models (vqvae2, vqvae2a, vqvae2b `Model`) share.

`HierModelBase` registers no submodule and sets no parameter: every `Model`
assigns its own ModuleLists, in the reference's order, which is the order of
its parameters and state_dict keys.  The base reads `levels`, `use_gst`,
`encoders`, `quantizers` (through the `_quantizer` hook) and, for `encode`,
`pooling_last`; `name` prefixes the messages.
"""
import torch
import torch.nn as nn

from .. import _lib as L
from .hier_common import LogLossFn, mean_pool
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
        parallel refused), built once per device and rebuilt when the
        parameters were moved."""
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
    def encode(self, input):
        """One entry per level (vqvae2a.py:72-91, vqvae2b.py:52-70): int64
        indices (B, T_i) of a quantized level, the style embedding (B, F, 1) of
        a style-token top.  Without gradients; writes nothing (a normalised
        codebook is normalised on the fly)."""
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
                    if self._pooled(i):
                        z = mean_pool(z)
                    zs.append(q.encode(z))
        return zs

    def convert(self, input):
        """(x (B, mel, T), y_idx (B, 1)) -> the xhat of the eval-mode forward,
        without gradients.  A normalised codebook, which every forward
        renormalises in place, gets its bits back, so no parameter or buffer
        changes (an EMA codebook is neither initialised nor updated in eval mode)."""
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
