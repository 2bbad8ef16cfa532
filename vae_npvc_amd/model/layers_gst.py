"""Style-token (GST) layer of the hierarchical model's top-level quantizer
(reference model/layers_gst.py:10-147, used with `use_gst: true` as
`layer(z.mean(dim=-1))`, vqvae2.py:97) on the MI355X.

A 1-query x `gst_tokens` multi-head attention over tanh(gst_embs) with
q/k/v/out linears.  libvqx computes it in two launches forward and three
backward (include/vqx.h vqx_gst_fwd / vqx_gst_bwd), the time pooling
included: `pool_forward(z)` is the fused `layer(z.mean(dim=-1))`.

Constructor, parameter tree and state_dict keys are the reference's
(`gst_embs`, `mha.linear_{q,k,v,out}.{weight,bias}`), so its checkpoints load
unchanged; initialisation draws the same random numbers in the same order.
Not built: dropout (the recipe uses 0) and the masked attention branch, which
no model reaches.  There is no CPU path.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops

F32 = torch.float32


class MultiHeadedAttention(nn.Module):
    """The parameter tree of the reference's attention (layers_gst.py:63-80);
    StyleTokenLayer computes with it."""

    def __init__(self, q_dim, k_dim, v_dim, n_head, n_feat, dropout_rate=0.0):
        super().__init__()
        if n_feat % n_head:
            raise ValueError(f"n_feat {n_feat} is not a multiple of n_head {n_head}")
        if k_dim != v_dim:
            raise ValueError("keys and values are the same tokens: k_dim must equal v_dim")
        if dropout_rate != 0.0:
            raise NotImplementedError("attention dropout is not built on the HIP path (the recipe uses 0)")
        self.d_k = n_feat // n_head
        self.h = n_head
        self.linear_q = nn.Linear(q_dim, n_feat)
        self.linear_k = nn.Linear(k_dim, n_feat)
        self.linear_v = nn.Linear(v_dim, n_feat)
        self.linear_out = nn.Linear(n_feat, n_feat)


class StyleTokenLayer(nn.Module):
    """forward(ref_embs (B, ref_embed_dim)) -> (B, gst_token_dim);
    pool_forward(z (B, ref_embed_dim, T)) = forward(z.mean(dim=-1)), fused."""

    def __init__(self, ref_embed_dim: int = 128, gst_tokens: int = 10, gst_token_dim: int = 256, gst_heads: int = 4,
                 dropout_rate: float = 0.0):
        super().__init__()
        if dropout_rate != 0.0:
            raise NotImplementedError("StyleTokenLayer: dropout_rate != 0 is not built on the HIP path "
                                      "(the recipe uses 0)")
        self.ref_embed_dim, self.gst_heads = ref_embed_dim, gst_heads
        self.gst_embs = nn.Parameter(torch.randn(gst_tokens, gst_token_dim // gst_heads))
        self.mha = MultiHeadedAttention(q_dim=ref_embed_dim, k_dim=gst_token_dim // gst_heads,
                                        v_dim=gst_token_dim // gst_heads, n_head=gst_heads, n_feat=gst_token_dim,
                                        dropout_rate=dropout_rate)

    def _params(self):
        m = self.mha
        return (self.gst_embs, m.linear_q.weight, m.linear_q.bias, m.linear_k.weight, m.linear_k.bias,
                m.linear_v.weight, m.linear_v.bias, m.linear_out.weight, m.linear_out.bias)

    def _apply_fn(self, x):
        params = self._params()
        save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _GstFn.apply(self.gst_heads, save, x, *params)

    def forward(self, ref_embs):
        if ref_embs.dim() != 2 or ref_embs.shape[1] != self.ref_embed_dim:
            raise ValueError(f"StyleTokenLayer: ref_embs {tuple(ref_embs.shape)} is not (B, {self.ref_embed_dim})")
        return self._apply_fn(ref_embs)

    def pool_forward(self, z):
        if z.dim() != 3 or z.shape[1] != self.ref_embed_dim:
            raise ValueError(f"StyleTokenLayer: z {tuple(z.shape)} is not (B, {self.ref_embed_dim}, T)")
        return self._apply_fn(z)

    def pool_rows(self, z_rows, T):
        """pool_forward without gradients on frame-major f32 rows z_rows [B*T, ref_embed_dim]
        (no layout change): the style embedding [B, gst_token_dim]."""
        if z_rows.dim() != 2 or z_rows.shape[1] != self.ref_embed_dim or z_rows.shape[0] % T:
            raise ValueError(f"StyleTokenLayer: z_rows {tuple(z_rows.shape)} is not [B*{T}, {self.ref_embed_dim}]")
        if not z_rows.is_cuda:
            raise L.VqxError("StyleTokenLayer runs on the MI355X only (libvqx); move it and its input with .cuda()")
        with torch.no_grad():
            params = tuple(p.detach().float().contiguous() for p in self._params())
            return _gst_rows(self.gst_heads, z_rows, T, params)[0]


def _gst_rows(heads, z, T, params):
    """vqx_gst_fwd on frame-major rows z [B*T, R] (T = 1: reference embeddings) with
    the nine contiguous f32 parameters: (style [B, F], the workspace the backward reads)."""
    B, R = z.shape[0] // T, z.shape[1]
    (N, E), Fd = params[0].shape, params[1].shape[0]
    ws = torch.empty(ops.gst_workspace(B, N, Fd, heads, R, E), device=z.device, dtype=F32)
    style = torch.empty(B, Fd, device=z.device, dtype=F32)
    ops.gst_fwd(z, T, params, heads, style, ws)
    return style, ws


class _GstFn(torch.autograd.Function):
    """x is (B, R) reference embeddings or (B, R, T) frames to pool."""

    @staticmethod
    def forward(ctx, heads, save, x, *params):
        if not x.is_cuda or not all(p.is_cuda for p in params):
            raise L.VqxError("StyleTokenLayer runs on the MI355X only (libvqx); move it and its input with .cuda()")
        dev = x.device
        if x.dim() == 3:  # (B, R, T) -> frame-major rows
            B, R, T = x.shape
            z = torch.empty(B * T, R, device=dev, dtype=F32)
            ops.nct_to_ntc(x.float().contiguous(), z)
        else:
            (B, R), T = x.shape, 1
            z = x.float()
            if z.stride(1) != 1 or z.stride(0) < R:  # rows of a wider buffer are read in place
                z = z.contiguous()
        params = tuple(p.detach().float().contiguous() for p in params)
        style, ws = _gst_rows(heads, z, T, params)
        if save:
            ctx.heads, ctx.T, ctx.xshape = heads, T, tuple(x.shape)
            ctx.save_for_backward(z, ws, *params)
        return style

    @staticmethod
    @once_differentiable
    def backward(ctx, d_style):
        z, ws, *params = ctx.saved_tensors
        T, dev = ctx.T, d_style.device
        dz = torch.empty(z.shape[0], z.shape[1], device=dev, dtype=F32)
        grads = tuple(torch.empty_like(p) for p in params)
        ops.gst_bwd(z, T, tuple(params), ctx.heads, d_style.float().contiguous(), ws, dz, grads)
        if len(ctx.xshape) == 3:
            dx = torch.empty(ctx.xshape, device=dev, dtype=F32)
            ops.ntc_to_nct(dz, dx)
        else:
            dx = dz
        return (None, None, dx, *grads)
