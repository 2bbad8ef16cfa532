"""Self-attention over the frames of a latent (the reference's
`MultiHeadedAttention`, model/layers_gst.py:63-147, called as
`mha(x^T, x^T, x^T, key mask)^T`) on the MI355X.

Launches of a forward (include/vqx.h vqx_attn_*): the layout change in, one
1x1 GEMM with the concatenated [3F][F] weight writing the packed q | k | v rows
in the compute dtype, the fused MFMA attention (keys streamed with an online
softmax, nothing T x T stored), the output linear as a 1x1 GEMM with f32
output, the layout change out.  The backward mirrors it: the output linear's
data and weight gradients, vqx_attn_bwd (3 launches, P recomputed from the
saved log-sum-exp, no atomics), the q/k/v GEMM's data and weight gradients.

`SelfAttention.mha` is the parameter tree of layers_gst.py, so a reference
`MultiHeadedAttention` state_dict loads into it unchanged and initialisation
draws the reference's numbers in its order.  Not built: dropout, cross
attention, causal masks, fp8 operands.  There is no CPU path.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .hier_common import DT, F32, colsum, wgrad
from .layers_gst import MultiHeadedAttention

D_K = (32, 64)  # head widths the kernels are built for (csrc/vqx_attn.hip)


class _Lin:
    """A linear as the 1x1 conv the helpers of hier_common.py take."""
    transposed, k, dil, pad = False, 1, 1, 0

    def __init__(self, cin, cout):
        self.cin, self.cout = cin, cout


def _pack(params, dt):
    """(wq, bq, wk, bk, wv, bv, wo, bo) -> the GEMMs' operands: the
    concatenated [3F, F] weight and wo in the compute dtype, the biases f32."""
    wq, bq, wk, bk, wv, bv, wo, bo = (p.detach() for p in params)
    return (torch.cat([wq, wk, wv]).to(dt).contiguous(), torch.cat([bq, bk, bv]).float().contiguous(),
            wo.to(dt).contiguous(), bo.float().contiguous())


def _attend(xr, B, T, H, lens, packed):
    """The three launches between the layout changes on rows xr [B*T, F] of the
    compute dtype: (out f32 [B*T, F], qkv, ctx, lse).  Rows t >= lens[b] of
    `out` hold the output bias (ctx is zero there); the callers cut them."""
    wqkv, bqkv, wo, bo = packed
    N, F = xr.shape
    e = lambda *s, dtype: torch.empty(*s, device=xr.device, dtype=dtype)  # noqa: E731
    qkv = ops.conv_fwd(xr, wqkv, e(N, 3 * F, dtype=xr.dtype), T=T, cin=F, cout=3 * F, ntaps=1, pad=0, bias=bqkv)
    ctx, lse = e(N, F, dtype=xr.dtype), e(B * H * T, dtype=F32)
    ops.attn_fwd(qkv, ctx, lse, B, T, H, lens)
    out = ops.conv_fwd(ctx, wo, e(N, F, dtype=F32), T=T, cin=F, cout=F, ntaps=1, pad=0, bias=bo, out_f32=True)
    return out, qkv, ctx, lse


def _rows_in(x, lens, dt):
    """(B, F, T) f32 -> (frame-major f32 rows, the same rows in the compute
    dtype): the one layout change in; with lens the tail is zeros, x's never read."""
    B, F, T = x.shape
    r32 = torch.empty(B * T, F, device=x.device, dtype=F32)
    if lens is None:
        ops.nct_to_ntc(x, r32)
    else:
        ops.nct_to_ntc_len(x, lens, r32)
    return r32, (r32 if dt == F32 else ops.convert_2d(r32, torch.empty_like(r32, dtype=dt)))


def _rows_out(rows, B, T, lens):
    x = torch.empty(B, rows.shape[1], T, device=rows.device, dtype=F32)
    return ops.ntc_to_nct(rows, x) if lens is None else ops.ntc_to_nct_len(rows, T, lens, x)


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, dt, lens, residual, save, x, *params):
        B, F, T = x.shape
        x32, xr = _rows_in(x.float().contiguous(), lens, dt)
        packed = _pack(params, dt)
        out, qkv, c, lse = _attend(xr, B, T, H, lens, packed)
        if residual:
            out.add_(x32)
        if save:
            ctx.cfg = (B, T, H, lens, residual)
            ctx.save_for_backward(xr, qkv, c, lse, packed[0], packed[2])
        return _rows_out(out, B, T, lens)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xr, qkv, c, lse, wqkv, wo = ctx.saved_tensors
        B, T, H, lens, residual = ctx.cfg
        N, F = xr.shape
        dt, dev = xr.dtype, xr.device
        e = lambda *s, dtype: torch.empty(*s, device=dev, dtype=dtype)  # noqa: E731
        g32, gr = _rows_in(g.float().contiguous(), lens, dt)  # the gradient into padded frames is ignored
        part = e(64 * max(3 * F, 1024), dtype=F32)
        lo, lqkv = _Lin(F, F), _Lin(F, 3 * F)
        dbo = colsum(gr, part)
        dwo = wgrad(lo, gr, c, T).reshape(F, F)
        d_ctx = ops.conv_dgrad(gr, wo, e(N, F, dtype=dt), T=T, cin=F, cout=F, ntaps=1, pad=0)
        d_qkv = e(N, 3 * F, dtype=dt)
        ops.attn_bwd(qkv, c, lse, d_ctx, d_qkv, e(ops.attn_workspace(B, T, F, H, dt), dtype=F32), B, T, H, lens)
        db = colsum(d_qkv, part)
        dw = wgrad(lqkv, d_qkv, xr, T).reshape(3 * F, F)
        dx = ops.conv_dgrad(d_qkv, wqkv, e(N, F, dtype=F32), T=T, cin=3 * F, cout=F, ntaps=1, pad=0, out_f32=True)
        if residual:
            dx.add_(g32)
        # d linear_k.bias is zero: the softmax ignores a per-query constant (as vqx_gst_bwd writes it)
        return (None, None, None, None, None, _rows_out(dx, B, T, lens),
                dw[:F], db[:F], dw[F:2 * F], torch.zeros_like(db[:F]), dw[2 * F:], db[2 * F:], dwo, dbo)


class SelfAttention(nn.Module):
    """forward(x (B, n_feat, T), lengths=None, residual=False) -> (B, n_feat, T) f32:
    mha(x^T, x^T, x^T, mask)^T (+ x with `residual`), the mask keeping the keys
    t2 < lengths[b].  With lengths (host ints, as ops.len_array takes them) the
    output frames t >= lengths[b] are exact zeros, whatever x holds there, and
    the gradient into them is ignored.

    forward_rows(rows f32 [B*T, n_feat], B, T, lengths=None, residual=False):
    the same bits on frame-major rows without gradients, keeping nothing."""

    def __init__(self, n_feat, n_head, dropout_rate=0.0, compute_dtype="fp32"):
        super().__init__()
        if dropout_rate != 0.0:
            raise NotImplementedError("SelfAttention: dropout_rate != 0 is not built on the HIP path")
        if n_head < 1 or n_feat % n_head:
            raise ValueError(f"SelfAttention: n_feat {n_feat} is not a multiple of n_head {n_head}")
        if n_feat // n_head not in D_K:
            raise NotImplementedError(f"SelfAttention: d_k = n_feat / n_head = {n_feat // n_head} is not built on the "
                                      f"HIP path (the kernels take {D_K[0]} or {D_K[1]})")
        if compute_dtype not in DT:
            raise ValueError(f"SelfAttention: compute_dtype {compute_dtype!r} not in {sorted(DT)}")
        self.n_feat, self.n_head, self.compute_dtype = n_feat, n_head, compute_dtype
        self.mha = MultiHeadedAttention(n_feat, n_feat, n_feat, n_head, n_feat)

    def _params(self):
        m = self.mha
        return (m.linear_q.weight, m.linear_q.bias, m.linear_k.weight, m.linear_k.bias, m.linear_v.weight,
                m.linear_v.bias, m.linear_out.weight, m.linear_out.bias)

    def _off_device(self):
        return L.VqxError("SelfAttention runs on the MI355X only (libvqx); move it and its input with .cuda()")

    def forward(self, x, lengths=None, residual=False):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.n_feat:
            raise ValueError(f"SelfAttention: x must be (B, {self.n_feat}, T)")
        lens = None if lengths is None else _lens(lengths, x.shape[0], x.shape[2])
        params = self._params()
        if not x.is_cuda or not all(p.is_cuda for p in params):
            raise self._off_device()
        save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _AttnFn.apply(self.n_head, DT[self.compute_dtype], lens, bool(residual), save, x, *params)

    def forward_rows(self, rows, B, T, lengths=None, residual=False):
        if not torch.is_tensor(rows) or rows.dim() != 2 or tuple(rows.shape) != (B * T, self.n_feat) \
                or rows.dtype != F32 or rows.stride(1) != 1:
            raise ValueError(f"SelfAttention: rows must be f32 [{B}*{T}, {self.n_feat}]")
        lens = None if lengths is None else _lens(lengths, B, T)
        params = self._params()
        if not rows.is_cuda or not all(p.is_cuda for p in params):
            raise self._off_device()
        dt = DT[self.compute_dtype]
        with torch.no_grad():
            if rows.stride(0) != self.n_feat or dt != F32:
                xr = ops.convert_2d(rows, torch.empty(B * T, self.n_feat, device=rows.device, dtype=dt))
            else:
                xr = rows
            out = _attend(xr, B, T, self.n_head, lens, _pack(params, dt))[0]
            if residual:
                out.add_(rows)
            return out if lens is None else ops.mask_tail(out, T, lens)


def _lens(lengths, B, T):
    """lengths as a host list of B ints in 1..T; ValueError before any launch."""
    lens = list(ops.len_array(lengths, B, "SelfAttention lengths"))
    if min(lens) < 1 or max(lens) > T:
        b = next(b for b, n in enumerate(lens) if not 1 <= n <= T)
        raise ValueError(f"SelfAttention: lengths[{b}] = {lens[b]} outside 1..T = {T}")
    return lens
