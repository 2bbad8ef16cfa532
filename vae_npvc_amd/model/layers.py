"""Parameter containers of the VQ-VAE with the reference's module tree and
state_dict keys (vae_npvc/model/layers.py, vqvae.py).

These modules only own parameters: the arithmetic of the whole training step
runs in the HIP engine (vae_npvc_amd/engine/step.py).  Registration order is
bias -> weight_g -> weight_v for every weight-normed conv, the order
nn.utils.weight_norm leaves in the reference (so model.parameters() order,
and therefore optimizer state_dicts, line up with reference checkpoints).
"""
import math

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops


class WNConv1d(nn.Module):
    """Weight-normed stride-1 Conv1d (kind 0, v [cout, cin, k], g [cout,1,1]) or
    ConvTranspose1d (kind 1, v [cin, cout, k], g [cin,1,1]); nn.utils.weight_norm
    with dim=0 as applied at vqvae.py:203-208,329-334."""

    def __init__(self, cin, cout, k, transposed=False, padding=None, dilation=1, weight_norm=True):
        super().__init__()
        self.cin, self.cout, self.k, self.transposed = cin, cout, k, transposed
        self.dilation = dilation
        self.padding = (k - 1) // 2 * dilation if padding is None else padding
        bound = 1.0 / math.sqrt((cout if transposed else cin) * k)
        vshape = (cin, cout, k) if transposed else (cout, cin, k)
        v = torch.empty(vshape).uniform_(-bound, bound)
        if not weight_norm:  # use_weight_norm: false -> a plain nn.Conv1d / ConvTranspose1d (weight, bias)
            # reset_parameters (vqvae.py:210-217, 336-343) re-draws every conv
            # weight N(0, 2/fan_in), torch's fan_in = weight.size(1) * k; with
            # weight norm on it is a no-op (it writes the recomputed .weight)
            nn.init.kaiming_normal_(v, nonlinearity="relu")
            self.weight = nn.Parameter(v)
            self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
            self.has_weight_norm = False
            return
        self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(vshape[0], 1, 1))
        self.weight_v = nn.Parameter(v)
        self.has_weight_norm = True

    @property
    def kind(self):
        return 1 if self.transposed else 0

    def effective_weight(self):
        """w = g * v/||v|| in the reference's (torch) layout, for export/inspection."""
        if not self.has_weight_norm:
            return self.weight
        return torch._weight_norm(self.weight_v, self.weight_g, 0)

    def remove_weight_norm(self):
        """Bake w into a plain `weight` parameter (torch.nn.utils.remove_weight_norm)."""
        if not self.has_weight_norm:
            raise ValueError("weight_norm not present")
        w = self.effective_weight().detach()
        del self.weight_g
        del self.weight_v
        self.weight = nn.Parameter(w)
        self.has_weight_norm = False

    def extra_repr(self):
        return (f"{self.cin}, {self.cout}, kernel_size={self.k}, padding={self.padding}, dilation={self.dilation}, "
                f"transposed={self.transposed}")


class ResidualBlock(nn.Module):
    """Conv1d_Layernorm_LRelu_Residual (layers.py:129-178):
    out = stack(c) + Conv_1(c), stack = [LReLU0.2, Conv_k(dilation), GN(1, C)]
    followed by (layers - 1) x [LReLU0.2, Conv_k, GN(1, C)] (layers.py:151-161)."""

    def __init__(self, channels, kernel_size=3, layers=1, dilation=1, weight_norm=True):
        super().__init__()
        if (kernel_size - 1) % 2:
            raise ValueError("Not support even number kernel size.")  # layers.py:142
        wn = weight_norm
        stack = [nn.LeakyReLU(0.2), WNConv1d(channels, channels, kernel_size, dilation=dilation, weight_norm=wn),
                 nn.GroupNorm(1, channels, eps=1e-5, affine=True)]
        for _ in range(layers - 1):
            stack += [nn.LeakyReLU(0.2), WNConv1d(channels, channels, kernel_size, weight_norm=wn),
                      nn.GroupNorm(1, channels, eps=1e-5, affine=True)]
        self.stack = nn.Sequential(*stack)
        self.skip_layer = WNConv1d(channels, channels, 1, weight_norm=wn)
        self.layers, self.dilation = layers, dilation

    @property
    def convs(self):
        return [self.stack[3 * l + 1] for l in range(self.layers)]

    @property
    def norms(self):
        return [self.stack[3 * l + 2] for l in range(self.layers)]


class ResSkipBlock(nn.Module):
    """DeConv1d_Layernorm_GLU_ResSkip (layers.py:181-249): h = GN(2, 2C)(ConvT(x) +
    Conv_1(c)) with ConvT of dilation d and padding (k-1)//2*d (layers.py:198-200);
    g = tanh(h[:C])*sigmoid(h[C:]); r = Conv_1(g); x' = r[:C] + x; skip = r[C:]."""

    def __init__(self, channels, cond_channels, skip_channels, kernel_size=3, dilation=1, weight_norm=True):
        super().__init__()
        if (kernel_size - 1) % 2:
            raise ValueError("Not support even number kernel size.")  # layers.py:197
        wn = weight_norm
        self.conv_in = WNConv1d(channels, 2 * channels, kernel_size, transposed=True,
                                padding=(kernel_size - 1) // 2 * dilation, dilation=dilation, weight_norm=wn)
        self.norm_layer = nn.GroupNorm(2, 2 * channels, eps=1e-5, affine=True)
        # cond_channels 0 / None: an unconditioned block, no conv_cond and no state_dict keys for it (layers.py:209-212)
        self.conv_cond = WNConv1d(cond_channels, 2 * channels, 1, weight_norm=wn) if cond_channels else None
        self.res_skip_layers = WNConv1d(channels, channels + skip_channels, 1, weight_norm=wn)
        self.in_channels = channels
        self.dilation = dilation


class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, weight):
        if not (ids.is_cuda and weight.is_cuda):
            raise L.VqxError("Conditions runs on the MI355X only (libvqx); move it and its ids with .cuda()")
        flat = ids.reshape(-1).to(torch.int64).contiguous()
        w = weight.detach().float().contiguous()
        out = torch.empty(flat.numel(), w.shape[1], device=w.device, dtype=torch.float32)
        ops.embedding_fwd(w, flat, out)
        ctx.rows = w.shape[0]
        ctx.save_for_backward(flat)
        return out.view(*ids.shape, w.shape[1])

    @staticmethod
    def backward(ctx, dout):
        flat, = ctx.saved_tensors
        d = dout.reshape(flat.numel(), -1).float().contiguous()
        dweight = torch.empty(ctx.rows, d.shape[1], device=d.device, dtype=torch.float32)
        ops.embedding_bwd_rows(d, flat, dweight)
        return None, dweight


class Conditions(nn.Module):
    """Speaker embedding (layers.py:12-60, normalize=False => nn.Embedding);
    forward(ids) -> ids.shape + (cond_dim,) through vqx_embedding_fwd /
    vqx_embedding_bwd_rows.  The normalised table (normalize=True) is not built."""

    def __init__(self, cond_num, cond_dim, normalize=False):
        super().__init__()
        if normalize:
            raise NotImplementedError("Conditions: normalize=True is not built on the HIP path (no model uses it)")
        self._embedding = nn.Embedding(cond_num, cond_dim)
        self.cond_num = cond_num
        self.normalize = False

    def forward(self, ids):
        return _EmbeddingFn.apply(ids, self._embedding.weight)


LOG_2PI = math.log(2.0 * math.pi)
