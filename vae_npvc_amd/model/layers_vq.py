"""Quantizer and jitter modules (buffers + API of vae_npvc/model/layers_vq.py).

The arithmetic (distance / argmin / gather / EMA update) is libvqx's fused HIP
kernels; these modules hold the state with the reference's buffer names so
checkpoints load both ways.  The flat model's engine drives the kernels itself
(engine/step.py); the forwards here compose them under torch autograd for the
hierarchical family.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops

F32 = torch.float32


def draw_code_rows(zf, K, comm=None, summed=False):
    """The rows `_tile(z)[torch.randperm(len)][:K]` of init_emb / update_emb
    (layers_vq.py:183-190,197,213) for the frames zf [N, D], drawn from torch's
    CPU generator exactly as the reference draws them: `randn_like` when N < K,
    then `randperm`.  Returns (perm, None) with perm a host int32 [K] tensor of
    row numbers of zf when N >= K (zf's values are not read: no
    synchronisation), else (None, rows) with rows the K tiled noisy rows as a
    host f32 tensor (zf is copied to the host; rare).

    comm (data parallel; anything with world, rank and all_gather_cat): zf is
    this rank's equal shard of a global batch of N * world frames, rank r
    owning the global rows [r * N, (r + 1) * N), and the generator is consumed
    exactly as one process on the global batch consumes it, identically on
    every rank.  With N * world >= K, perm holds this rank's local row numbers
    and -1 for a row another rank owns (ops.gather_rows_host gives zero rows
    there), so the SUM over ranks of the gathers is the global batch's rows.
    Otherwise the tiling runs on the all_gather_cat of the ranks' frames and
    every rank gets the same K rows; with `summed` (the rows go through a SUM
    all-reduce) every rank but 0 gets zeros instead.  Needs no device."""
    N, D = zf.shape
    world = 1 if comm is None else comm.world
    if N * world >= K:
        perm = torch.randperm(N * world)[:K]
        if comm is not None:
            from ..parallel.ddp import owned_rows
            perm = owned_rows(perm, comm.rank * N, N)
        return perm.to(torch.int32), None
    z = zf.detach().float()
    if comm is not None:
        z = comm.all_gather_cat(z)
    z = z.cpu()
    n = z.shape[0]
    zt = z.repeat((K + n - 1) // n, 1)
    zt = zt + torch.randn_like(zt) * (0.01 / np.sqrt(D))
    rows = zt[torch.randperm(zt.shape[0])][:K].contiguous()
    if summed and comm is not None and comm.rank != 0:
        rows.zero_()
    return None, rows


def map_to_device(src_t, device):
    """A host int32 neighbour map (Jitter.draw) on `device`: a pinned,
    non-blocking copy (nothing waits for it on the host)."""
    return torch.from_numpy(np.ascontiguousarray(src_t, dtype=np.int32)).pin_memory().to(device, non_blocking=True)


class EMAVectorQuantizer(nn.Module):
    """EMA codebook (layers_vq.py:166-334).  Buffers emb_init (bool),
    emb_sum [K, D], emb_elem [K], embeddings [K, D] (layers_vq.py:170-173)."""

    def __init__(self, z_num, z_dim, mu, threshold=1.0, reduction="frame_mean"):
        super().__init__()
        if reduction != "frame_mean":
            raise NotImplementedError("only reduction='frame_mean' (the reference Model's setting, vqvae.py:24)")
        self.register_buffer("emb_init", torch.tensor(0).bool())
        self.register_buffer("emb_sum", torch.zeros(z_num, z_dim))
        self.register_buffer("emb_elem", torch.ones(z_num))
        self.register_buffer("embeddings", torch.zeros(z_num, z_dim))
        self.mu, self.z_num, self.z_dim, self.threshold = mu, z_num, z_dim, threshold
        self.reduction = reduction
        self.quantize = True
        self.update = True
        self._init_host = None  # host mirror of emb_init (avoids a device sync per step)
        self.last_indices = None
        self.comm = None  # data parallel: attach_comm

    @property
    def initialized(self):
        if self._init_host is None:
            self._init_host = bool(self.emb_init.item())
        return self._init_host

    def mark_initialized(self):
        self.emb_init.fill_(True)
        self._init_host = True

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._init_host = None

    def attach_comm(self, comm):
        """Data parallel (parallel/ddp.py Comm, or None to detach): a training
        forward that initialises or updates the codebook then uses the GLOBAL
        batch, every rank holding an equal shard of it: init_emb's rows are
        SUM-reduced into `embeddings`, and bsum | bcnt | rand_rows travel in
        one SUM all-reduce per call between the lookup and the EMA update, so
        the buffers, entropy, used_curr, usage and diff_emb are global and
        equal on every rank.  The commitment loss stays the rank's own (the
        mean over ranks is the global value).  An eval-mode forward, encode and
        decode issue no collective."""
        self.comm = comm

    def encode(self, z, time_last=True):
        """Nearest-code indices of z (B, D, T) (layers_vq.py:236-252) on the HIP VQ kernel."""
        if time_last:
            B, D, T = z.shape
            zf = z.transpose(1, 2).reshape(-1, D).float().contiguous()
        else:
            B, T, D = z.shape
            zf = z.reshape(-1, D).float().contiguous()
        n = zf.shape[0]
        idx = torch.empty(n, dtype=torch.int64, device=z.device)
        ops.vq_forward(zf, self.embeddings.contiguous(), idx, None, None, None)
        return idx.view(B, T)

    def decode(self, z_id, time_last=True):
        """Codebook gather (layers_vq.py:255-265)."""
        B, T = z_id.shape
        out = torch.empty(B * T, self.z_dim, device=z_id.device)
        ops.gather_rows(self.embeddings.contiguous(), z_id.reshape(-1).contiguous(), out)
        out = out.view(B, T, -1)
        return out.transpose(1, 2).contiguous() if time_last else out

    def forward(self, z, time_last=True, loss_weights=None, src_t=None):
        """layers_vq.py:268-323 for reduction 'frame_mean' on the HIP kernels:
        (z_vq, 0.0, z_enc_loss, detail).  z is (B, D, T) ((B, T, D) with
        time_last=False); z_enc_loss is a 0-dim device tensor.  In training
        mode (with `update`) the codebook buffers are updated in place after
        the lookup and `detail` holds entropy, used_curr, usage and diff_emb as
        0-dim device tensors the caller reads; otherwise it is empty.  The
        first training call initialises the codebook from z (init_emb).

        loss_weights=(w_qut, w_enc): returns (z_vq, loss, 0.0, z_enc_loss,
        detail) with loss = w_enc * z_enc_loss the level's one differentiable
        scalar (z_enc_loss is then not differentiable), as VectorQuantizer.forward.

        z_vq carries NO gradient: in the reference the straight-through line
        `z_vq = z + (z_vq - z).detach()` is indented under reduction == 'none'
        (layers_vq.py:310-315), so with 'frame_mean' z_vq is the detached
        gather.  dL/dz is the commitment term alone, one vqx_vq_commit_bwd_g
        launch with the upstream gradient read on the device.

        src_t: a host int32 neighbour map (Jitter.draw) applied to z_vq inside
        its layout change (vqx_ntc_to_nct_gather), or None.

        The CPU generator is consumed exactly as the reference does: init draws
        randn_like (when B*T < K) then randperm, the update the same pair again.
        A steady-state training call (B*T >= K, initialised) does not
        synchronise with the host.  `last_indices` holds the int64 (B, T)
        indices of the last call (a device tensor nothing waits for)."""
        if not self.quantize:  # the reference's early exit (:269-271)
            tensor_0 = torch.tensor(0.0, dtype=torch.float, device=z.device)
            return z, tensor_0, tensor_0, tensor_0
        if self.z_dim not in (64, 128, 256):
            raise NotImplementedError(f"z_dim {self.z_dim}: the HIP quantizer is built for z_dim 64, 128 or 256")
        if self.z_num % 16 or self.z_num > 2048:
            raise NotImplementedError(f"z_num {self.z_num}: the HIP quantizer takes K % 16 == 0, K <= 2048")
        if z.dim() != 3 or z.shape[1 if time_last else 2] != self.z_dim:
            raise ValueError(f"EMAVectorQuantizer: z {tuple(z.shape)} does not carry {self.z_dim} channels")
        if src_t is not None and not time_last:
            raise NotImplementedError("EMAVectorQuantizer: a jitter map needs time_last=True")
        if not (z.is_cuda and self.embeddings.is_cuda):
            raise L.VqxError("EMAVectorQuantizer.forward runs on the MI355X only (libvqx); move it and z with .cuda()")
        w_enc = None if loss_weights is None else float(loss_weights[1])
        save = torch.is_grad_enabled() and z.requires_grad
        src = None if src_t is None else map_to_device(src_t, z.device)
        z_vq, loss, enc, diag, self.last_indices = _EMAQuantizeFn.apply(self, time_last, w_enc, save, src, z)
        detail = {}
        if diag is not None:
            detail = {k: diag[i] for i, k in enumerate(("entropy", "used_curr", "usage", "diff_emb"))}
        if w_enc is None:
            return z_vq, 0.0, enc, detail
        return z_vq, loss, 0.0, enc, detail

    def _workspace(self, dev):
        """vqx_vq_ema_update's workspace (its arrival counter stays zero between calls)."""
        ws = getattr(self, "_ema_ws", None)
        if ws is None or ws.device != dev:
            ws = self._ema_ws = torch.zeros(ops.ema_workspace(self.z_num, self.z_dim), device=dev, dtype=F32)
        return ws

    def extra_repr(self):
        return f"{self.z_num}, {self.z_dim}, mu={self.mu}, threshold={self.threshold}"


class _EMAQuantizeFn(torch.autograd.Function):
    """EMAVectorQuantizer.forward: [init_emb] vqx_vq_forward (with the EMA
    statistics when the codebook is updated), vqx_vq_ema_update*, the layout
    change; one vqx_vq_commit_bwd_g backward.  Outputs (z_vq, weighted loss,
    z_enc_loss, diag [4] or None, indices)."""

    @staticmethod
    def forward(ctx, q, time_last, w_enc, save, src, z):
        dev = z.device
        e = lambda *shape: torch.empty(*shape, device=dev, dtype=F32)  # noqa: E731
        if time_last:
            B, D, T = z.shape
            zf = ops.nct_to_ntc(z.detach().float().contiguous(), e(B * T, D))
        else:
            B, T, D = z.shape
            zf = z.detach().reshape(B * T, D).float().contiguous()
        N, K = B * T, q.z_num
        E = q.embeddings
        if E.dtype != F32 or not E.is_contiguous():
            raise ValueError("EMAVectorQuantizer: the codebook buffer must be a contiguous f32 tensor")
        comm = q.comm
        if q.training and not q.initialized:  # init_emb (:192-201)
            perm, rows = draw_code_rows(zf, K, comm)
            if perm is not None:
                ops.gather_rows_host(zf, perm, E)
                if comm is not None:  # each rank filled the rows it owns
                    comm.all_reduce_sum(E)
            else:
                E.copy_(rows)
            ops.convert_2d(E, q.emb_sum)
            q.emb_elem.fill_(1.0)
            q.mark_initialized()
        update = q.training and q.update
        idx = torch.empty(N, device=dev, dtype=torch.int64)
        zq, sq = e(N, D), e(1)
        diag = None
        if update and comm is not None:
            # the global batch's statistics: bsum | bcnt | rand_rows in one bundle, one SUM
            # all-reduce between the lookup and the update (on RCCL the wait is a stream wait)
            bundle = ops.zero_(e(1, 2 * K * D + K)).view(-1)
            bsum, bcnt = bundle[:K * D].view(K, D), bundle[K * D:K * D + K]
            rand = bundle[K * D + K:].view(K, D)
            ops.vq_forward(zf, E, idx, zq, None, sq, None, bsum, bcnt)
            perm, rows = draw_code_rows(zf, K, comm, summed=True)  # update_emb's dead-code rows (:212-213)
            if perm is not None:
                ops.gather_rows_host(zf, perm, rand)
            else:
                rand.copy_(rows)
            work = comm.all_reduce_sum(bundle, async_op=True)
            diag = e(4)
            comm.wait(work, "ema")
            ops.vq_ema_update(q.emb_sum, q.emb_elem, E, bsum, bcnt, rand, q.mu, q.threshold, diag, q._workspace(dev))
        elif update:
            counts = ops.zero_(e(1, K * D + K)).view(-1)
            bsum, bcnt = counts[:K * D].view(K, D), counts[K * D:]
            ops.vq_forward(zf, E, idx, zq, None, sq, None, bsum, bcnt)
            perm, rows = draw_code_rows(zf, K)  # update_emb's dead-code rows (:212-213)
            diag = e(4)
            args = (q.emb_sum, q.emb_elem, E, bsum, bcnt)
            if perm is not None and K <= 512:  # the rows are read from zf inside the update launch
                ops.vq_ema_update(*args, None, q.mu, q.threshold, diag, q._workspace(dev), clear=True, rows=(zf, perm))
            else:
                rand = ops.gather_rows_host(zf, perm, e(K, D)) if perm is not None else rows.to(dev)
                ops.vq_ema_update(*args, rand, q.mu, q.threshold, diag, q._workspace(dev))
        else:
            ops.vq_forward(zf, E, idx, zq, None, sq, None, None, None)
        enc = sq[0] / N  # frame_mean: the sum over frames and channels / (B*T) (:308-309)
        loss = w_enc * enc if w_enc is not None else None
        if time_last:
            z_vq = e(B, D, T)
            if src is not None:
                ops.ntc_to_nct_gather(zq, src, z_vq)
            else:
                ops.ntc_to_nct(zq, z_vq)
        else:
            z_vq = zq.view(B, T, D)
        idx = idx.view(B, T)
        ctx.mark_non_differentiable(z_vq, idx, *(() if diag is None else (diag,)), *((enc,) if w_enc is not None else ()))
        ctx.set_materialize_grads(False)
        if save:
            ctx.cfg = (time_last, w_enc, (B, D, T))
            ctx.keep = (zf, zq)
        return z_vq, loss, enc, diag, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, dzvq, dloss, denc, ddiag, didx):
        time_last, w_enc, (B, D, T) = ctx.cfg
        zf, zq = ctx.keep
        ctx.keep = None
        g, w = (dloss, w_enc) if w_enc is not None else (denc, 1.0)
        if g is None:
            return None, None, None, None, None, None
        dz = torch.empty((B, D, T) if time_last else (B * T, D), device=zf.device, dtype=F32)
        ops.vq_commit_bwd_g(zf, zq, B, T, 2.0 * w / (B * T), g.detach().float().reshape(1).contiguous(), dz)
        return None, None, None, None, None, dz if time_last else dz.view(B, T, D)


class VectorQuantizer(nn.Module):
    """Straight-through codebook (layers_vq.py:9-163): the codebook is the
    parameter `embeddings` [K, D] (randn, normalised at construction when
    `normalize`, :13-20).  Training runs in the engine (vqx_vq_normalize /
    vqx_vq_forward / vqx_vq_plain_bwd); encode / decode here run the same HIP
    kernels without the in-place renormalisation, as the reference's do."""

    def __init__(self, z_num, z_dim, normalize=False, reduction="frame_mean"):
        super().__init__()
        if reduction != "frame_mean":
            raise NotImplementedError("only reduction='frame_mean' (the reference Model's setting, vqvae.py:31)")
        self.target_norm = 1.0 if normalize else None
        self.embeddings = nn.Parameter(torch.randn(z_num, z_dim, requires_grad=True))
        self.embed_norm()
        self.z_num, self.z_dim, self.normalize, self.reduction = z_num, z_dim, normalize, reduction
        self.quantize = True

    def embed_norm(self):
        """In-place row renormalisation of the codebook (layers_vq.py:28-33)."""
        if self.target_norm:
            with torch.no_grad():
                self.embeddings.mul_(self.target_norm / self.embeddings.norm(dim=1, keepdim=True))

    def _codebook(self):
        E = self.embeddings.detach().float().contiguous()
        if not self.normalize:
            return E
        K = E.shape[0]
        Ew = E.clone()
        emb = torch.empty_like(E)
        elen = torch.empty(K, device=E.device)
        zdummy = torch.zeros(1, E.shape[1], device=E.device)
        ops.vq_normalize(zdummy, Ew, torch.empty_like(zdummy), torch.empty(1, device=E.device), emb, elen,
                         torch.empty(2, device=E.device))
        # Ew was renormalised (not written back: encode/decode do not call embed_norm);
        # emb = Ew/||Ew|| == the reference's target_norm * E / ||E|| up to rounding
        return emb

    def encode(self, z, time_last=True):
        """Nearest-code indices (layers_vq.py:36-58) on the HIP VQ kernel."""
        if time_last:
            B, D, T = z.shape
            zf = z.transpose(1, 2).reshape(-1, D).float().contiguous()
        else:
            B, T, D = z.shape
            zf = z.reshape(-1, D).float().contiguous()
        n = zf.shape[0]
        emb = self._codebook()
        if self.normalize:
            zn, zl = torch.empty_like(zf), torch.empty(n, device=z.device)
            ops.vq_normalize(zf, emb.clone(), zn, zl, torch.empty_like(emb), torch.empty(emb.shape[0], device=z.device),
                             torch.empty(n // 4 + 2, device=z.device))
            zf = zn
        idx = torch.empty(n, dtype=torch.int64, device=z.device)
        ops.vq_forward(zf, emb, idx, None, None, None)
        return idx.view(B, T)

    def decode(self, z_id, time_last=True):
        """Codebook gather (layers_vq.py:61-76)."""
        B, T = z_id.shape
        out = torch.empty(B * T, self.z_dim, device=z_id.device)
        ops.gather_rows(self._codebook(), z_id.reshape(-1).contiguous(), out)
        out = out.view(B, T, -1)
        return out.transpose(1, 2).contiguous() if time_last else out

    def forward(self, z, time_last=True, loss_weights=None, src_t=None):
        """layers_vq.py:79-150 for reduction 'frame_mean' on the HIP kernels:
        (z_vq, z_qut_loss, z_enc_loss, {'entropy': perplexity}).  z is (B, D, T)
        ((B, T, D) with time_last=False); z_vq carries the gathered codes and
        passes its gradient straight through to z; both losses are 0-dim device
        tensors, and `entropy` stays one until the caller reads it.  With
        `normalize` the codebook parameter is renormalised in place first
        (embed_norm(), :96).

        loss_weights=(w_qut, w_enc): returns (z_vq, loss, z_qut_loss,
        z_enc_loss, detail) where loss = w_qut * z_qut_loss + w_enc * z_enc_loss
        is the level's one differentiable scalar and the two parts are not
        differentiable (vqvae2.Model's call: w_qut = 1, w_enc = beta).

        Either way one vqx_vq_plain_bwd_g launch gives dL/dz and dL/dE; the
        upstream gradients of the scalars are read on the device.

        src_t: a host int32 neighbour map (Jitter.draw) for the jitter the
        reference applies to z_vq afterwards (vqvae2a.py:157): z_vq leaves
        through vqx_ntc_to_nct_gather and its gradient comes back through
        vqx_nct_to_ntc_keep (a replaced frame passes none).  None: today's
        launches and bits."""
        if not self.quantize:  # the reference's early exit (:80-82)
            tensor_0 = torch.tensor(0.0, dtype=torch.float, device=z.device)
            return z, tensor_0, tensor_0, tensor_0
        if self.z_dim not in (64, 128, 256):
            raise NotImplementedError(f"z_dim {self.z_dim}: the HIP quantizer is built for z_dim 64, 128 or 256")
        if z.dim() != 3 or z.shape[1 if time_last else 2] != self.z_dim:
            raise ValueError(f"VectorQuantizer: z {tuple(z.shape)} does not carry {self.z_dim} channels")
        if src_t is not None and not time_last:
            raise NotImplementedError("VectorQuantizer: a jitter map needs time_last=True")
        weights = None if loss_weights is None else (float(loss_weights[0]), float(loss_weights[1]))
        save = torch.is_grad_enabled() and (z.requires_grad or self.embeddings.requires_grad)
        src = None if src_t is None or not z.is_cuda else map_to_device(src_t, z.device)
        z_vq, loss, qut, enc, perp, _ = _QuantizeFn.apply(self.normalize, time_last, weights, save, src, z,
                                                          self.embeddings)
        if weights is None:
            return z_vq, qut, enc, {"entropy": perp}
        return z_vq, loss, qut, enc, {"entropy": perp}

    def forward_indices(self, z, time_last=True):
        """forward's nearest-code indices (B, T) alone, from the same launches
        (the codebook renormalised in place as forward does)."""
        with torch.no_grad():
            return _QuantizeFn.apply(self.normalize, time_last, None, False, None, z, self.embeddings)[5]

    def extra_repr(self):
        return f"{self.z_num}, {self.z_dim}" + (", normalize=True" if self.normalize else "")


class _QuantizeFn(torch.autograd.Function):
    """VectorQuantizer.forward: vqx_vq_normalize (when `normalize`), vqx_vq_forward
    and vqx_vq_perplexity forward, one vqx_vq_plain_bwd_g backward.  Outputs
    (z_vq, weighted loss, z_qut_loss, z_enc_loss, perplexity, indices); with
    `weights` the weighted loss is the differentiable scalar, else the two parts."""

    @staticmethod
    def forward(ctx, normalize, time_last, weights, save, src, z, E):
        if not (z.is_cuda and E.is_cuda):
            raise L.VqxError("VectorQuantizer.forward runs on the MI355X only (libvqx); move it and z with .cuda()")
        dev = z.device
        e = lambda *shape: torch.empty(*shape, device=dev, dtype=F32)  # noqa: E731
        if time_last:
            B, D, T = z.shape
            zf = ops.nct_to_ntc(z.float().contiguous(), e(B * T, D))
        else:
            B, T, D = z.shape
            zf = z.reshape(B * T, D).float().contiguous()
        N, K = B * T, E.shape[0]
        if E.dtype != F32 or not E.is_contiguous():
            raise ValueError("VectorQuantizer: the codebook parameter must be a contiguous f32 tensor")
        stats = e(3)  # sum ||z_vq - z_norm||^2, sum ||z_norm - z||^2, perplexity
        counts = ops.zero_(e(1, K * D + K)).view(-1)
        bsum, bcnt = counts[:K * D].view(K, D), counts[K * D:]
        if normalize:
            zn, zl, emb, el = e(N, D), e(N), e(K, D), e(K)
            ops.vq_normalize(zf, E.detach(), zn, zl, emb, el, e(N // 4 + 2), stats[1:2])
        else:
            zn, zl, emb, el = zf, None, E.detach(), None
        idx = torch.empty(N, device=dev, dtype=torch.int64)
        zq = e(N, D)
        ops.vq_forward(zn, emb, idx, zq, None, stats[0:1], None, bsum, bcnt)
        ops.vq_perplexity(bcnt, N, stats[2:3])
        qut = stats[0] / N  # frame_mean: the sum over frames and channels / (B*T) (:133-134)
        enc = (stats[0] + stats[1]) / N if normalize else stats[0] / N
        loss = weights[0] * qut + weights[1] * enc if weights is not None else qut + enc
        if time_last and src is not None:
            z_vq = ops.ntc_to_nct_gather(zq, src, e(B, D, T))
        elif time_last:
            z_vq = ops.ntc_to_nct(zq, e(B, D, T))
        else:
            z_vq = zq.view(B, T, D)
        idx = idx.view(B, T)
        perp = stats[2].clone()
        ctx.mark_non_differentiable(idx, perp, *((qut, enc) if weights is not None else (loss,)))
        ctx.set_materialize_grads(False)
        if save:
            ctx.cfg = (normalize, time_last, weights, (B, D, T))
            ctx.keep = (zf, zn, zl, zq, bsum, bcnt, emb, el, src)
        return z_vq, loss, qut, enc, perp, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, dzvq, dloss, dqut, denc, dperp, didx):
        normalize, time_last, weights, (B, D, T) = ctx.cfg
        zf, zn, zl, zq, bsum, bcnt, emb, el, src = ctx.keep
        dev, N = zq.device, B * T
        if dzvq is None:
            dzq = None
        elif time_last and src is not None:
            dzq = ops.nct_to_ntc_keep(dzvq.float().contiguous(), src, torch.empty(N, D, device=dev, dtype=F32))
        elif time_last:
            dzq = ops.nct_to_ntc(dzvq.float().contiguous(), torch.empty(N, D, device=dev, dtype=F32))
        else:
            dzq = dzvq.reshape(N, D).float().contiguous()
        if weights is not None:
            w_qut, w_enc, g_qut, g_enc = weights[0], weights[1], dloss, dloss
        else:
            w_qut, w_enc, g_qut, g_enc = 1.0, 1.0, dqut, denc
        # a scalar nothing depends on: its term is dropped (weight 0), its gradient not read
        s_qut = 2.0 * w_qut / N if g_qut is not None else 0.0
        s_enc = 2.0 * w_enc / N if g_enc is not None else 0.0
        g = [None if t is None else t.detach().float().reshape(1).contiguous() for t in (g_qut, g_enc)]
        dz, dE = torch.empty(N, D, device=dev, dtype=F32), torch.empty_like(emb)
        ops.vq_plain_bwd_g(zf, zn, zl, zq, dzq, T, normalize, s_qut, s_enc, g[0], g[1], dz, bsum, bcnt, emb, el, dE)
        ctx.keep = None
        if time_last:
            dz = ops.ntc_to_nct(dz, torch.empty(B, D, T, device=dev, dtype=F32))
        else:
            dz = dz.view(B, T, D)
        return None, None, None, None, None, dz, dE


class Jitter(nn.Module):
    """Jitter (layers_vq.py:337-383).  The neighbour map is drawn on the host
    numpy stream exactly as the reference does (so seeded runs match): `draw`
    gives it to a quantizer's forward, which folds the gather into its layout
    change (the flat model's engine draws its own, engine/step.py); `forward`
    applies one to a stand-alone tensor.  Note the reference's indexing
    replaces a frame with probability 1-p (layers_vq.py:365)."""

    def __init__(self, probability=0.12):
        super().__init__()
        self.probability = probability

    def draw(self, T):
        """The neighbour map of one forward over T frames (layers_vq.py:353-379):
        a host int32 array, frame t showing frame map[t]; None when p == 0 or
        not training (the reference's early return, no draw).  The global numpy
        stream is consumed exactly as np.random.choice does, one uniform per
        choice: one per frame, a second for a replaced inner frame.  A frame is
        replaced with probability 1 - p (the reference's indexing, :364).
        T == 1 raises: the reference indexes frame 1 of 1 there."""
        p = self.probability
        if p == 0.0 or not self.training:
            return None
        if T == 1:
            raise ValueError("Jitter: one frame has no neighbour (the reference indexes out of range at T == 1)")
        src = np.arange(T, dtype=np.int32)
        cdf = np.cumsum([p, 1 - p])
        keep_below = (cdf / cdf[-1])[0]
        rs = np.random.random_sample
        for i in range(T):
            if rs() < keep_below:  # np.random.choice([1, 0], p=[p, 1-p]) == 1 -> [True, False][1]: keep
                continue
            if i == 0:
                src[i] = 1
            elif i == T - 1:
                src[i] = T - 2
            else:
                src[i] = i + (-1 if rs() < 0.5 else 1)
        return src

    def forward(self, x):
        """Jitter of a stand-alone (B, C, T) device tensor: draws a map and
        gathers the frames (vqx_ntc_to_nct_gather); the backward passes the
        gradient of the frames that kept themselves (vqx_nct_to_ntc_keep)."""
        if x.dim() != 3:
            raise ValueError(f"Jitter: x {tuple(x.shape)} is not (B, C, T)")
        src = self.draw(x.shape[2])
        if src is None:
            return x
        if not x.is_cuda:
            raise L.VqxError("Jitter.forward runs on the MI355X only (libvqx); move x with .cuda()")
        return _JitterFn.apply(map_to_device(src, x.device), x)

    def extra_repr(self):
        return f"jitter_prob={self.probability}"


class _JitterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, x):
        B, C, T = x.shape
        rows = ops.nct_to_ntc(x.float().contiguous(), torch.empty(B * T, C, device=x.device, dtype=F32))
        ctx.src = src
        return ops.ntc_to_nct_gather(rows, src, torch.empty(B, C, T, device=x.device, dtype=F32))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        B, C, T = g.shape
        rows = ops.nct_to_ntc_keep(g.float().contiguous(), ctx.src, torch.empty(B * T, C, device=g.device, dtype=F32))
        return None, ops.ntc_to_nct(rows, torch.empty(B, C, T, device=g.device, dtype=F32))
