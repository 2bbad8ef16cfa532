"""Time one training step of the hierarchical model at the vae2 recipe's shape
(B = 96, T = 256, 80 mels, 3 levels, use_gst, about 70 M parameters in about
420 tensors), fp32 and bf16 compute, four ways:

  a  the whole step through this package's Trainer (engine/autograd_step.py:
     autograd forward + backward, multi-tensor clip + Adam + StepLR);
  b  the whole step through the reference recipe's loop on the same HIP model:
     zero_grad, forward, backward, clip_grad_norm_, torch.optim.Adam, StepLR;
  c  the optimizer part of a alone (engine.optimizer_step() on the gradients
     a step left behind);
  d  the optimizer part of b alone (clip_grad_norm_ + Adam.step + StepLR.step).

Also the two multi-tensor passes of c on their own, with the achieved bytes
per second from the algorithmic bytes (norm: g read once; Adam: p, g, m, v
read and p, m, v written once) against the 8 TB/s HBM figure, and the number
of launches of c.

--ddp times the price of the data-parallel path itself instead (scaling over
GPUs needs more than one): the whole step with a world-size-1 RCCL Comm
attached (vqx_multi_pack, one AVG all-reduce of the flat gradient per bucket,
the gradient views) against the step without one, two trainers in one process,
alternating; and, on the gradients a step left behind, the pack launches alone
and the pack + all-reduce + wait.  With the collectives, bytes and pack
launches per step.

Device events around windows of REPS iterations, the paths alternating, median
and spread over the windows.  A lab script, no pass/fail bar.
Usage (GPU box): python tools/hier_train_bench.py [--json OUT] [--dtypes fp32,bf16] [--ddp]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vae_npvc_amd import ops  # noqa: E402
from vae_npvc_amd.model.vqvae2 import Model  # noqa: E402
from vae_npvc_amd.trainer.basic import Trainer  # noqa: E402

B, T, MEL = 96, 256, 80
WARMUP, REPS, WINDOWS = 2, 4, 7
HBM_BYTES_PER_S = 8e12


def recipe(dtype):
    """The vae2 recipe's model and optimizer keys (egs/vcc20/vae2/conf/train_pytorch_vqvae2.yaml)."""
    enc = dict(kernel_size=3, z_channels=128, dilation=False, stack_kernel_size=3, stack_layers=1,
               use_weight_norm=True, use_causal_conv=False)
    dec = dict(out_channels=[512], skip_channels=128, kernel_size=3, upsample_scales=[1], dilation=False,
               stack_kernel_size=3, use_weight_norm=True, use_causal_conv=False)
    vq = dict(z_dim=128, z_num=512, normalize=True)
    return {
        "trainer_type": "vae_npvc_amd.trainer.basic", "model_type": "vae_npvc_amd.model.vqvae2",
        "optim_type": "Adam", "learning_rate": 1e-3, "max_grad_norm": 10, "lr_scheduler": "StepLR",
        "lr_param": {"step_size": 100000, "gamma": 0.5, "last_epoch": -1},
        "levels": 3, "y_dim": 128, "y_num": 117, "beta": 0.01, "use_gst": True, "use_ema": False, "jitter_p": 0.0,
        "compute_dtype": dtype,
        "encoder.0": dict(enc, in_channels=[MEL], out_channels=[512], downsample_scales=[1], stacks=[6]),
        "encoder.1": dict(enc, in_channels=[512, 512], out_channels=[512, 512], downsample_scales=[2, 2], stacks=[3, 3]),
        "encoder.2": dict(enc, in_channels=[512, 512], out_channels=[512, 512], downsample_scales=[4, 4], stacks=[3, 3]),
        "quantizer.0": dict(vq), "quantizer.1": dict(vq),
        "quantizer.2": dict(ref_embed_dim=128, gst_tokens=10, gst_token_dim=128, gst_heads=4),
        "decoder.0": dict(dec, in_channels=[384], cond_channels=128, final_channels=MEL, stacks=[10]),
        "decoder.1": dict(dec, in_channels=[128], cond_channels=256, final_channels=128, stacks=[6]),
        "decoder.2": dict(dec, in_channels=[128], cond_channels=128, final_channels=128, stacks=[6]),
    }


def timed(paths, warmup, reps, windows):
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in paths}
    for _ in range(windows):
        for name, fn in paths.items():  # alternate: every path sees the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / reps)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


def run(dtype):
    cfg = recipe(dtype)
    torch.manual_seed(0)
    tr = Trainer(cfg)
    ref = Model(cfg).cuda().train()
    ref.load_state_dict(tr.model.state_dict())
    x = torch.randn(B, MEL, T, device="cuda")
    y = torch.randint(0, cfg["y_num"], (B, 1), device="cuda")
    opt = torch.optim.Adam(ref.parameters(), lr=cfg["learning_rate"], betas=(0.5, 0.999), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.StepLR(optimizer=opt, **cfg["lr_param"])
    params = list(ref.parameters())
    eng = tr.engine

    def torch_optim():
        torch.nn.utils.clip_grad_norm_(params, cfg["max_grad_norm"])
        opt.step()
        sched.step()

    def torch_step():
        ref.zero_grad()
        _, loss, _ = ref((x, y))
        loss.backward()
        torch_optim()

    def fused_adam_only():
        ops.multi_adam_step(eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.plan, eng.hyper, eng.sumsq,
                            float(eng.max_grad_norm), 0)

    n, nt = eng.n_params, len(eng.params)
    groups = -(-nt // ops.MULTI_MAX_TENSORS)
    res = {"dtype": dtype, "shape": dict(B=B, T=T, mel=MEL), "parameters": n, "tensors": nt,
           "partials": eng.plan.n_partials, "reps": REPS, "windows": WINDOWS,
           "launches": {"fused_multi_sq_norm": groups, "fused_finish": 2, "fused_multi_adam": groups,
                        "fused_total": 2 * groups + 2}}
    res["step"] = timed({"a_trainer": lambda: tr.train_step((x, y)), "b_torch_loop": torch_step},
                        WARMUP, REPS, WINDOWS)
    # the optimizer parts, on the gradients the last steps left behind
    grads = eng._grads()
    eng.plan.set_grads(grads)
    res["optimizer"] = timed({"c_fused": eng.optimizer_step, "d_torch": torch_optim}, WARMUP, 10, WINDOWS)
    res["passes"] = timed({"multi_sq_norm": lambda: ops.multi_sq_norm(eng.plan, eng.sq_part),
                           "multi_adam": fused_adam_only}, WARMUP, 10, WINDOWS)
    for name, nbytes in (("multi_sq_norm", 4 * n), ("multi_adam", 28 * n)):
        r = res["passes"][name]
        r["algorithmic_bytes"] = nbytes
        r["bytes_per_s"] = nbytes / (r["median_us"] * 1e-6)
        r["fraction_of_hbm"] = r["bytes_per_s"] / HBM_BYTES_PER_S
    for group in ("step", "optimizer", "passes"):
        for name, r in res[group].items():
            extra = f", {r['bytes_per_s'] / 1e12:.2f} TB/s ({100 * r['fraction_of_hbm']:.0f}% of 8 TB/s)" \
                if "bytes_per_s" in r else ""
            print(f"{dtype} {group} {name}: median {r['median_us'] / 1e3:.3f} ms (min {r['min_us'] / 1e3:.3f}, "
                  f"max {r['max_us'] / 1e3:.3f}){extra}", flush=True)
    print(f"{dtype}: {n} parameters in {nt} tensors, {res['launches']['fused_total']} optimizer launches", flush=True)
    return res


def run_ddp(dtype):
    """The step with a world-size-1 RCCL Comm attached against the step without."""
    import socket

    import torch.distributed as dist

    from vae_npvc_amd.parallel.ddp import Comm
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dev = torch.device("cuda", torch.cuda.current_device())
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    cfg = recipe(dtype)
    torch.manual_seed(0)
    plain = Trainer(cfg)  # (world size 1: the Trainer attaches nothing)
    ddp = Trainer(cfg)
    ddp.model.load_state_dict(plain.model.state_dict())
    comm = Comm()
    eng = ddp.engine
    eng.attach_comm(comm)
    x = torch.randn(B, MEL, T, device="cuda")
    y = torch.randint(0, cfg["y_num"], (B, 1), device="cuda")
    n, nt = eng.n_params, len(eng.params)
    res = {"dtype": dtype, "shape": dict(B=B, T=T, mel=MEL), "parameters": n, "tensors": nt, "reps": REPS,
           "windows": WINDOWS, "backend": comm.backend, "world": comm.world}
    res["step"] = timed({"plain": lambda: plain.train_step((x, y)), "comm_world1": lambda: ddp.train_step((x, y))},
                        WARMUP, REPS, WINDOWS)
    comm.reset_stats()
    ddp.train_step((x, y))
    torch.cuda.synchronize()
    res["per_step"] = {"collectives": comm.calls, "bytes": comm.bytes, "pack_launches": -(-nt // ops.MULTI_MAX_TENSORS)}
    # the added work alone, on the gradient tensors autograd left behind in the plain trainer
    grads = plain.engine._grads()
    eng.plan.set_grads(grads)

    def pack_reduce_wait():
        ops.multi_pack(eng.plan, eng.flat_g)
        comm.grads_ready(eng.flat_g, 0, n)
        comm.finish()

    res["reduce"] = timed({"multi_pack": lambda: ops.multi_pack(eng.plan, eng.flat_g),
                           "pack_allreduce_wait": pack_reduce_wait}, WARMUP, 10, WINDOWS)
    r = res["reduce"]["multi_pack"]
    r["algorithmic_bytes"] = 8 * n  # g read once, flat written once
    r["bytes_per_s"] = 8 * n / (r["median_us"] * 1e-6)
    r["fraction_of_hbm"] = r["bytes_per_s"] / HBM_BYTES_PER_S
    for group in ("step", "reduce"):
        for name, r in res[group].items():
            extra = f", {r['bytes_per_s'] / 1e12:.2f} TB/s ({100 * r['fraction_of_hbm']:.0f}% of 8 TB/s)" \
                if "bytes_per_s" in r else ""
            print(f"{dtype} ddp {group} {name}: median {r['median_us'] / 1e3:.3f} ms (min {r['min_us'] / 1e3:.3f}, "
                  f"max {r['max_us'] / 1e3:.3f}){extra}", flush=True)
    a, b = res["step"]["plain"]["median_us"], res["step"]["comm_world1"]["median_us"]
    res["step"]["added_us"] = b - a
    print(f"{dtype} ddp: comm step - plain step = {(b - a) / 1e3:+.3f} ms; per step {res['per_step']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--ddp", action="store_true", help="time the data-parallel path (world-size-1 RCCL) instead")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "hier_train_bench needs the MI355X"
    out = [(run_ddp if a.ddp else run)(d) for d in a.dtypes.split(",")]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.ddp:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
