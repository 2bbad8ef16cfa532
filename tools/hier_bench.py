"""Time the hierarchical decoder's block stack forward + backward at the vae2
recipe's `decoder.1` shape (B = 96, T = 256, 128 -> 512 channels, cond 256 =
128 (T_l = 1) + 128 (T_l = 64), 6 ResSkip blocks, skip 128, final 128, bf16),
three ways:

  low    model.vqvae2.Decoder on the levels: conv_cond at the conditioning's
         own rate (B*64 rows), added in the conv_in epilogue by segment;
  full   the same module on the levels pre-stretched into a tensor c
         (B, 256, T): conv_cond and its gradients at full rate (B*256 rows);
  torch  the same stack from torch ops on the GPU under bf16 autocast.

Then `upsample_cat` for the 384-channel `decoder.0` input (levels of 128
channels at T_l = 256, 64, 1 -> bf16 [B*T, 384]) against torch's
repeat / cat / transpose / cast, with the achieved bytes per second from the
algorithmic bytes (levels read once in fp32, output written once in bf16).

Device events around windows of REPS iterations, the paths alternating, median
over the windows.  A lab script, no pass/fail bar.
Usage (GPU box): python tools/hier_bench.py [--json OUT] [--blocks N]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vae_npvc_amd import ops  # noqa: E402
from vae_npvc_amd.model.layers import ResSkipBlock  # noqa: E402
from vae_npvc_amd.model.vqvae2 import Decoder  # noqa: E402

B, T, CIN, C, S, FIN = 96, 256, 128, 512, 128, 128
LEVELS = ((128, 1), (128, 64))  # (channels, T_l) of the conditioning
WARMUP, REPS, WINDOWS = 3, 10, 7


def stretch(z, t):
    tl = z.shape[-1]
    return z[..., torch.clamp(torch.arange(t, device=z.device) // (t // tl), max=tl - 1)]


def composed(dec, x, c):
    """dec((x, c)) from stock torch ops on the module's parameters (vqvae2.py:352-371)."""
    skips = 0.0
    for layer in dec.layers:
        if isinstance(layer, ResSkipBlock):
            ci, cc, rs, n = layer.conv_in, layer.conv_cond, layer.res_skip_layers, layer.in_channels
            h = F.conv_transpose1d(x, ci.effective_weight(), ci.bias, padding=ci.padding, dilation=ci.dilation)
            h = F.group_norm(h + F.conv1d(c, cc.effective_weight(), cc.bias), 2, layer.norm_layer.weight,
                             layer.norm_layer.bias, eps=1e-5)
            r = F.conv1d(torch.tanh(h[:, :n]) * torch.sigmoid(h[:, n:]), rs.effective_weight(), rs.bias)
            x, skips = r[:, :n] + x, skips + r[:, n:]
        else:
            x = F.conv_transpose1d(x, layer.effective_weight(), layer.bias, padding=layer.padding)
    y = skips * math.sqrt(1.0 / len(dec.layers))
    f1, f2 = dec.final_layer[1], dec.final_layer[3]
    return F.conv1d(F.relu(F.conv1d(F.relu(y), f1.effective_weight(), f1.bias)), f2.effective_weight(), f2.bias)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--blocks", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "hier_bench needs the MI355X"
    torch.manual_seed(0)
    dec = Decoder(in_channels=[CIN], out_channels=[C], upsample_scales=[1], cond_channels=sum(c for c, _ in LEVELS),
                  skip_channels=S, final_channels=FIN, kernel_size=3, dilation=False, stack_kernel_size=3,
                  stacks=[a.blocks], compute_dtype="bf16").cuda()
    x = torch.randn(B, CIN, T, device="cuda", requires_grad=True)
    levels = [torch.randn(B, c, tl, device="cuda", requires_grad=True) for c, tl in LEVELS]
    c_full = torch.cat([stretch(z.detach(), T) for z in levels], dim=1).requires_grad_()
    go = torch.randn(B, FIN, T, device="cuda")

    def step(fn):
        dec.zero_grad(set_to_none=True)
        x.grad = None
        for z in (*levels, c_full):
            z.grad = None
        fn().backward(go)

    def torch_path():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return composed(dec, x, torch.cat([stretch(z, T) for z in levels], dim=1)).float()

    paths = {"low": lambda: step(lambda: dec((x, levels))), "full": lambda: step(lambda: dec((x, c_full))),
             "torch": lambda: step(torch_path)}
    grads = {}
    for name, fn in paths.items():
        fn()
        grads[name] = [p.grad.clone() for p in dec.parameters()] + [x.grad.clone()]
    l2 = lambda u, v: max(float((p - q).norm() / q.norm().clamp_min(1e-30)) for p, q in zip(u, v))  # noqa: E731
    res = {"shape": dict(B=B, T=T, cin=CIN, C=C, cond=[list(v) for v in LEVELS], blocks=a.blocks, skip=S, final=FIN),
           "reps": REPS, "windows": WINDOWS,
           "grad_rel_l2_worst": {"low_vs_full": l2(grads["low"], grads["full"]),
                                 "low_vs_torch": l2(grads["low"], grads["torch"])}}
    print(f"gradients, worst per-tensor relative L2 difference: low vs full {res['grad_rel_l2_worst']['low_vs_full']:.2e}, "
          f"low vs torch autocast {res['grad_rel_l2_worst']['low_vs_torch']:.2e}", flush=True)
    res["decoder"] = timed(paths, WARMUP, REPS, WINDOWS)
    for name, r in res["decoder"].items():
        print(f"decoder {name}: fwd+bwd median {r['median_us'] / 1e3:.3f} ms (min {r['min_us'] / 1e3:.3f}, "
              f"max {r['max_us'] / 1e3:.3f}) over {WINDOWS} windows of {REPS}", flush=True)

    # upsample_cat: the decoder.0 input, levels of 128 channels at T_l = 256, 64 and 1
    lens = (256, 64, 1)
    zs = [torch.randn(B, 128, tl, device="cuda") for tl in lens]
    rows = [z.transpose(1, 2).reshape(B * z.shape[2], 128).contiguous() for z in zs]  # the engine's frame-major layout
    out = torch.empty(B * T, 384, device="cuda", dtype=torch.bfloat16)
    nbytes = sum(r.numel() * 4 for r in rows) + out.numel() * 2

    def torch_cat():
        return torch.cat([z.unsqueeze(-1).repeat(1, 1, 1, T // z.shape[2]).flatten(-2, -1) for z in zs], dim=1) \
            .transpose(1, 2).contiguous().view(B * T, 384).to(torch.bfloat16)

    assert torch.equal(ops.upsample_cat_fwd(rows, B, T, out), torch_cat())
    res["upsample_cat"] = timed({"hip": lambda: ops.upsample_cat_fwd(rows, B, T, out), "torch": torch_cat}, 10, 100, 7)
    res["upsample_cat"]["algorithmic_bytes"] = nbytes
    for name in ("hip", "torch"):
        r = res["upsample_cat"][name]
        r["gbytes_per_s"] = nbytes / (r["median_us"] * 1e-6) / 1e9
        print(f"upsample_cat {name}: median {r['median_us']:.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f}), "
              f"{r['gbytes_per_s']:.0f} GB/s of {nbytes / 1e6:.1f} MB algorithmic", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
