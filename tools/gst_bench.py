"""Time the style-token layer forward + backward at the recipe's shape
(B = 96, R = 128, 10 tokens, F = 128, 4 heads, T = 4; fixture case batch96):
the fused libvqx path (StyleTokenLayer.pool_forward) against the same math
composed from torch ops on the GPU.  Device events around windows of REPS
iterations, the two paths alternating, median over the windows; then one
profiled iteration of each to count kernel launches.  A lab script, no
pass/fail bar.
Usage (GPU box): python tools/gst_bench.py [--json OUT]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vae_npvc_amd.model.layers_gst import StyleTokenLayer  # noqa: E402

B, R, N, FEAT, H, T = 96, 128, 10, 128, 4, 4
WARMUP, REPS, WINDOWS = 20, 200, 9


def composed(layer, z):
    """layer(z.mean(-1)) from stock torch ops on the layer's parameters."""
    m, dk = layer.mha, layer.mha.d_k
    tok = torch.tanh(layer.gst_embs)
    q = m.linear_q(z.mean(-1)).view(-1, H, dk)
    k = m.linear_k(tok).view(N, H, dk)
    v = m.linear_v(tok).view(N, H, dk)
    a = torch.softmax(torch.einsum("bhd,nhd->bhn", q, k) / math.sqrt(dk), dim=-1)
    return m.linear_out(torch.einsum("bhn,nhd->bhd", a, v).reshape(-1, H * dk))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gst_bench needs the MI355X"
    torch.manual_seed(0)
    layer = StyleTokenLayer(ref_embed_dim=R, gst_tokens=N, gst_token_dim=FEAT, gst_heads=H).cuda()
    z = torch.randn(B, R, T, device="cuda", requires_grad=True)
    go = torch.randn(B, FEAT, device="cuda")

    def step(fn):
        layer.zero_grad(set_to_none=True)
        z.grad = None
        fn(z).backward(go)

    paths = {"fused": lambda: step(layer.pool_forward), "torch": lambda: step(lambda x: composed(layer, x))}
    step(layer.pool_forward)
    g_fused = [p.grad.clone() for p in layer.parameters()] + [z.grad.clone()]
    step(lambda x: composed(layer, x))
    g_torch = [p.grad.clone() for p in layer.parameters()] + [z.grad.clone()]
    worst = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(g_fused, g_torch)
                if float(y.abs().max()) > 1e-5)  # linear_k.bias: zero against torch's rounding residue
    print(f"fused vs torch gradients: worst max-relative difference {worst:.2e}", flush=True)

    for fn in paths.values():
        for _ in range(WARMUP):
            fn()
    times = {k: [] for k in paths}
    for _ in range(WINDOWS):
        for name, fn in paths.items():  # alternate: both see the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / REPS)
    res = {"shape": dict(B=B, R=R, N=N, F=FEAT, H=H, T=T), "reps": REPS, "windows": WINDOWS, "grad_diff": worst}
    for name, ts in times.items():
        res[name] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}
        print(f"{name}: fwd+bwd median {res[name]['median_us']:.1f} us  (min {min(ts):.1f}, max {max(ts):.1f}) "
              f"over {WINDOWS} windows of {REPS}", flush=True)

    from torch.profiler import ProfilerActivity, profile
    for name, fn in paths.items():
        try:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                       and not e.name.lower().startswith(("memcpy", "memset"))]
            res[name]["launches"] = len(kernels)
            res[name]["vqx_launches"] = sum("vqx" in k for k in kernels)
            print(f"{name}: {len(kernels)} kernel launches per fwd+bwd ({res[name]['vqx_launches']} of libvqx)",
                  flush=True)
        except Exception as e:  # the profiler is optional; the timings above stand
            print(f"{name}: launches not measured ({type(e).__name__}: {e})", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
