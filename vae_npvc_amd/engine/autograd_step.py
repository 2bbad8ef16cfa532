"""Optimizer engine for a model whose forward and backward run under torch
autograd (vqvae2.Model): the parameters and Adam's moments live in flat
buffers like VQVAEEngine's, the gradients are whatever tensors autograd hands
over, and the global-norm clip, Adam or RAdam and StepLR run as the
multi-tensor HIP launches (vqx_multi_sq_norm, vqx_sq_norm_finish[_adam],
vqx_multi_adam_step) with every per-step scalar on the device.

It shows `Trainer` and `FusedOptimState` (trainer/basic.py) the surface of
VQVAEEngine: params, flat_p, exp_avg, exp_avg_sq, opt_step, hyper, sumsq, lr0,
sched_step, sched_gamma, betas, eps, opt_kind, device, init_optimizer,
params_intact, invalidate_packed, attach_comm, train_step, optimizer_step.

Data parallel (attach_comm with a parallel.ddp.Comm): after the backward the
gradient tensors are packed into one flat buffer (vqx_multi_pack, zeros where
a parameter has no gradient), mean all-reduced in the Comm's buckets, and
every parameter that had a gradient gets its view of the buffer as .grad, so
the clip and Adam run on the averaged gradient unchanged.  Autograd gives no
per-group completion point, so both `grad_sync` values reduce after the
backward: a reduction overlapped with the backward is not built (and nothing
on a one-GPU box could measure it).  The EMA quantizer levels reduce their own
statistics (model/layers_vq.py).
"""
import torch

from .. import ops

F32 = torch.float32


class AutogradEngine:
    fused_forward = False  # Trainer.train_step: the step returns the model's loss dict, not a workspace
    data_parallel = True   # Trainer._setup_engine: attach_comm takes a parallel.ddp.Comm
    world, rank = 1, 0

    def __init__(self, model, device):
        self.m = model
        self.device = torch.device(device)
        self.comm = None
        self.opt_ready = False
        self._flatten()

    # ------------------------------------------------------------ parameters
    def _flatten(self):
        """Every parameter becomes a view of one dense flat buffer, in
        model.parameters() order with no padding (FusedOptimState walks the
        moments with the same offsets); in-place writes such as the
        quantizer's embed_norm() and load_state_dict keep working on the views."""
        params = list(self.m.parameters())
        for p in params:
            if p.dtype != F32 or p.device != self.device:
                raise ValueError("AutogradEngine: every parameter must be a float32 tensor on " + str(self.device))
        self.params = params
        numels = [p.numel() for p in params]
        self._p_off, _, _ = ops.multi_layout(numels)
        self.n_params = sum(numels)
        self.flat_p = torch.empty(self.n_params, device=self.device, dtype=F32)
        with torch.no_grad():
            for p, off in zip(params, self._p_off):
                n = p.numel()
                self.flat_p[off:off + n].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[off:off + n].view_as(p)
        self.plan = ops.MultiTensorPlan(numels, self._p_off)

    def params_intact(self):
        base = self.flat_p.data_ptr()
        return all(p.data_ptr() == base + 4 * o for p, o in zip(self.params, self._p_off))

    def invalidate_packed(self):
        """Nothing is cached from the parameters between steps."""

    def attach_comm(self, comm):
        """Run the data-parallel path over `comm` (parallel/ddp.py Comm): the
        flat gradient's mean all-reduce after the backward (reduce_grads) and,
        in every EMAVectorQuantizer of the model, the global-batch codebook
        statistics.  Anything else is refused."""
        from ..model.layers_vq import EMAVectorQuantizer
        from ..parallel.ddp import Comm
        if not isinstance(comm, Comm):
            raise NotImplementedError("data parallel for the hierarchical models runs over a parallel.ddp.Comm, not "
                                      + type(comm).__name__)
        self.comm, self.world, self.rank = comm, comm.world, comm.rank
        self.flat_g = torch.zeros(self.n_params, device=self.device, dtype=F32)
        # every parameter's view of flat_g, made once (about 450 slices a step would cost the host a millisecond)
        self._g_views = [self.flat_g[off:off + p.numel()].view_as(p) for p, off in zip(self.params, self._p_off)]
        for q in self.m.modules():
            if isinstance(q, EMAVectorQuantizer):
                q.attach_comm(comm)

    def reduce_grads(self):
        """Data parallel: the mean over ranks of every gradient.  Packs the
        gradient tensors into flat_g (ceil(n / MULTI_MAX_TENSORS) launches;
        zeros for a parameter without one, so every rank sends the same
        ranges), all-reduces it in the Comm's buckets and makes the stream wait
        for them, then hands every parameter that had a gradient its view of
        flat_g.  A parameter without a gradient keeps None (Adam skips it, as
        torch.optim.Adam does).  Nothing without a comm."""
        if self.comm is None:
            return
        grads = self._grads()
        self.plan.set_grads(grads)
        ops.multi_pack(self.plan, self.flat_g)
        self.comm.grads_ready(self.flat_g, 0, self.n_params)
        self.comm.finish()
        for p, g, view in zip(self.params, grads, self._g_views):
            if g is not None:
                p.grad = view
        del grads

    # ------------------------------------------------------------ optimizer
    def init_optimizer(self, lr, betas=(0.5, 0.999), eps=1e-8, max_grad_norm=10.0, sched_step=None, sched_gamma=1.0,
                       kind="adam"):
        """kind 'adam' (torch.optim.Adam) or 'radam' (the reference's RAdam), both
        with the global-norm clip and StepLR; VQVAEEngine.init_optimizer's signature."""
        if kind not in ("adam", "radam"):
            raise ValueError(f"unknown optimizer {kind!r}")
        self.opt_kind = kind
        z = lambda n, dtype=F32: torch.zeros(n, device=self.device, dtype=dtype)  # noqa: E731
        self.exp_avg = z(self.n_params)
        self.exp_avg_sq = z(self.n_params)
        self.opt_step = z(1, torch.int64)
        self.hyper = z(16)
        self.sumsq = z(1)
        self.norm_part = z(1024)                     # the finish's 256-float scratch
        self.sq_part = z(max(self.plan.n_partials, 1))[:self.plan.n_partials]
        self.lr0, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        self.sched_step = sched_step or (1 << 30)
        self.sched_gamma = sched_gamma
        self.opt_ready = True

    def _grads(self):
        """The gradient tensors in parameter order (None where autograd gave
        none), contiguous float32; the list keeps converted copies alive until
        the launches that read them are queued."""
        out = []
        for p in self.params:
            g = p.grad
            if g is not None and (g.dtype != F32 or not g.is_contiguous()):
                g = g.to(F32).contiguous()
            out.append(g)
        return out

    def optimizer_step(self):
        """Clip + Adam / RAdam + StepLR from the parameters' .grad, with no
        host synchronisation: 2 * ceil(n / MULTI_MAX_TENSORS) multi-tensor
        launches and the two of the finish (three with RAdam)."""
        if not self.opt_ready:
            raise RuntimeError("init_optimizer() first")
        grads = self._grads()
        self.plan.set_grads(grads)
        clip = self.max_grad_norm > 0
        b1, b2 = self.betas
        hyper_args = (self.opt_step, self.lr0, self.sched_gamma, self.sched_step, b1, b2, self.eps, self.hyper)
        if clip:
            ops.multi_sq_norm(self.plan, self.sq_part)
            if self.opt_kind == "adam":
                ops.sq_norm_finish_adam(self.sq_part, None, None, self.sumsq, self.norm_part, *hyper_args)
            else:
                ops.sq_norm_finish(self.sq_part, None, None, self.sumsq, self.norm_part)
        if self.opt_kind == "radam":
            ops.radam_hyper(*hyper_args)
        elif not clip:
            ops.adam_hyper(*hyper_args)
        ops.multi_adam_step(self.flat_p, self.exp_avg, self.exp_avg_sq, self.plan, self.hyper,
                            self.sumsq if clip else None, float(self.max_grad_norm),
                            1 if self.opt_kind == "radam" else 0)
        del grads

    def train_step(self, x, y):
        """One training step (reference trainer/basic.py:55-79): forward and
        backward under autograd, [reduce_grads(),] then optimizer_step().  Returns the model's
        loss dict (its one readback happens at the end of the forward)."""
        for p in self.params:
            p.grad = None  # no zero-fill launches; autograd hands over its own tensors without an accumulate
        _, loss, detail = self.m((x, y))
        loss.backward()
        self.reduce_grads()
        self.optimizer_step()
        return detail

    def valid_step(self, x, y):
        """model.eval() forward without gradients.  A normalised codebook is
        renormalised in place by every forward of the quantizer; validation
        puts the parameter's bits back, so a validation pass leaves the
        training trajectory exactly where it was."""
        mutated = [q.embeddings for q in self.m.modules()
                   if getattr(q, "normalize", False) and isinstance(getattr(q, "embeddings", None), torch.nn.Parameter)]
        saved = [e.detach().clone() for e in mutated]
        self.m.eval()
        try:
            with torch.no_grad():
                _, _, detail = self.m((x, y))
                for e, s in zip(mutated, saved):
                    e.copy_(s)
        finally:
            self.m.train()
        return detail
