"""Time the self-attention layer (model/layers_attn.py, csrc/vqx_attn.hip) on the
MI355X, bf16 and fp32 compute, at (B 96, T 256, F 128, H 4) and (B 96, T 64,
F 128, H 4):

  layer        SelfAttention forward + backward under autograd (layout changes,
               q/k/v GEMM, attention, output GEMM and their backward);
  attention    the attention launches alone: vqx_attn_fwd + vqx_attn_bwd on the
               layer's own qkv rows;
  projections  the GEMM side alone: the two forward GEMMs, their data
               gradients, weight gradients and bias column sums;
  sdpa         torch.nn.functional.scaled_dot_product_attention forward +
               backward on the same q, k, v in the same process, the yardstick.
               If the call does not run here the output says so; no number is
               substituted.

With the FLOPs from the shapes -- algorithmic: forward 2 products, backward 5,
each 2 * B * H * T^2 * d_k; executed by vqx_attn_bwd: 7 products, since each of
its two kernels recomputes S and dP -- and the resulting share of the MFMA peak
of the compute dtype (bf16 2.5 PFLOP/s dense; the f32-input MFMA runs at 1/16
of it).  That share is of a whole forward + backward call, launches included,
not of a kernel.

--model times one vqvae2a training step through this package's Trainer at the
vae2 recipe's dimensions (B 96, T 256, 80 mels, 3 levels, style-token top,
K = 1024 EMA codebooks) without and with `attention.0` / `attention.1`
(n_head 4), two trainers in one process, alternating.

Device events around windows of REPS iterations after warm-up, the paths
alternating, median and spread over the windows.  A lab script, no pass/fail bar.
Usage (GPU box): python tools/attn_bench.py [--json OUT] [--dtypes bf16,fp32] [--model]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hier_train_bench import B, MEL, T, recipe, timed  # noqa: E402
from vae_npvc_amd import ops  # noqa: E402
from vae_npvc_amd.model import layers_attn  # noqa: E402
from vae_npvc_amd.model.hier_common import DT, colsum, wgrad  # noqa: E402

SHAPES = [(96, 256, 128, 4), (96, 64, 128, 4)]
WARMUP, REPS, WINDOWS = 3, 20, 7
PEAK = {"bf16": 2.5e15, "fp32": 2.5e15 / 16}  # dense MFMA FLOP/s


def layer_paths(Bn, Tn, F, H, dtype):
    dt, dev = DT[dtype], "cuda"
    torch.manual_seed(0)
    layer = layers_attn.SelfAttention(F, H, compute_dtype=dtype).cuda()
    x = torch.randn(Bn, F, Tn, device=dev, requires_grad=True)
    go = torch.randn(Bn, F, Tn, device=dev)

    def whole():
        layer.zero_grad(set_to_none=True)
        x.grad = None
        layer(x).backward(go)

    # the layer's own intermediate tensors, for the two halves
    e = lambda *s, dtype: torch.empty(*s, device=dev, dtype=dtype)  # noqa: E731
    N = Bn * Tn
    packed = layers_attn._pack(layer._params(), dt)
    xr = layers_attn._rows_in(x.detach(), None, dt)[1]
    gr = layers_attn._rows_in(go, None, dt)[1]
    out, qkv, ctx, lse = layers_attn._attend(xr, Bn, Tn, H, None, packed)
    wqkv, bqkv, wo, bo = packed
    d_ctx, d_qkv = e(N, F, dtype=dt), e(N, 3 * F, dtype=dt)
    ws = e(ops.attn_workspace(Bn, Tn, F, H, dt), dtype=torch.float32)
    ops.conv_dgrad(gr, wo, d_ctx, T=Tn, cin=F, cout=F, ntaps=1, pad=0)
    part = e(64 * max(3 * F, 1024), dtype=torch.float32)
    lo, lqkv = layers_attn._Lin(F, F), layers_attn._Lin(F, 3 * F)
    dx = e(N, F, dtype=torch.float32)

    def attention():
        ops.attn_fwd(qkv, ctx, lse, Bn, Tn, H)
        ops.attn_bwd(qkv, ctx, lse, d_ctx, d_qkv, ws, Bn, Tn, H)

    def projections():
        ops.conv_fwd(xr, wqkv, qkv, T=Tn, cin=F, cout=3 * F, ntaps=1, pad=0, bias=bqkv)
        ops.conv_fwd(ctx, wo, out, T=Tn, cin=F, cout=F, ntaps=1, pad=0, bias=bo, out_f32=True)
        colsum(gr, part)
        wgrad(lo, gr, ctx, Tn)
        ops.conv_dgrad(gr, wo, d_ctx, T=Tn, cin=F, cout=F, ntaps=1, pad=0)
        colsum(d_qkv, part)
        wgrad(lqkv, d_qkv, xr, Tn)
        ops.conv_dgrad(d_qkv, wqkv, dx, T=Tn, cin=3 * F, cout=F, ntaps=1, pad=0, out_f32=True)

    paths = {"layer": whole, "attention": attention, "projections": projections}
    note = None
    try:
        d = F // H
        q, k, v = (qkv[:, i * F:(i + 1) * F].reshape(Bn, Tn, H, d).transpose(1, 2).contiguous().requires_grad_()
                   for i in range(3))
        g = torch.randn(Bn, H, Tn, d, device=dev, dtype=dt)

        def sdpa():
            q.grad = k.grad = v.grad = None
            torch.nn.functional.scaled_dot_product_attention(q, k, v).backward(g)
        sdpa()
        torch.cuda.synchronize()
        paths["sdpa"] = sdpa
    except Exception as err:  # the yardstick is optional; its absence is reported, not replaced
        note = f"scaled_dot_product_attention did not run here: {type(err).__name__}: {err}"
    return paths, note


def run_layer(dtype):
    res = []
    for Bn, Tn, F, H in SHAPES:
        paths, note = layer_paths(Bn, Tn, F, H, dtype)
        t = timed(paths, WARMUP, REPS, WINDOWS)
        d = F // H
        product = 2.0 * Bn * H * Tn * Tn * d
        flops = {"algorithmic_fwd_bwd": 7 * product, "executed_fwd_bwd": 9 * product}
        r = {"dtype": dtype, "shape": dict(B=Bn, T=Tn, F=F, H=H), "reps": REPS, "windows": WINDOWS, "times": t,
             "flops": flops, "sdpa_note": note}
        a = t["attention"]["median_us"] * 1e-6
        r["attention_flops_per_s"] = {k: v / a for k, v in flops.items()}
        r["attention_share_of_mfma_peak"] = {k: v / a / PEAK[dtype] for k, v in flops.items()}
        for name, v in t.items():
            print(f"{dtype} B{Bn} T{Tn} F{F} H{H} {name}: median {v['median_us']:.1f} us (min {v['min_us']:.1f}, "
                  f"max {v['max_us']:.1f})", flush=True)
        print(f"{dtype} B{Bn} T{Tn} attention fwd+bwd: {flops['algorithmic_fwd_bwd'] / 1e9:.2f} GFLOP algorithmic "
              f"({flops['executed_fwd_bwd'] / 1e9:.2f} executed) -> {r['attention_flops_per_s']['algorithmic_fwd_bwd'] / 1e12:.2f} "
              f"TFLOP/s, {100 * r['attention_share_of_mfma_peak']['algorithmic_fwd_bwd']:.2f} % of the {dtype} MFMA peak "
              f"({100 * r['attention_share_of_mfma_peak']['executed_fwd_bwd']:.2f} % executed)", flush=True)
        if note:
            print(f"{dtype} B{Bn} T{Tn}: {note}", flush=True)
        res.append(r)
    return res


def recipe_2a(dtype, attention):
    """hier_train_bench.recipe rewired for vqvae2a: decoder i reads cat([z_vq_i, decoder i+1's output]) and its
    own speaker embedding; EMA codebooks of K = 1024."""
    cfg = recipe(dtype)
    vq = dict(z_num=1024, z_dim=128, mu=0.99)
    cfg.update({"model_type": "vae_npvc_amd.model.vqvae2a", "use_ema": True, "quantizer.0": dict(vq),
                "quantizer.1": dict(vq)})
    for i, cin in ((2, 128), (1, 256), (0, 256)):
        cfg[f"decoder.{i}"] = dict(cfg[f"decoder.{i}"], in_channels=[cin], cond_channels=cfg["y_dim"])
    if attention:
        cfg.update({"attention.0": {"n_head": 4}, "attention.1": {"n_head": 4}})
    return cfg


def run_model(dtype):
    from vae_npvc_amd.trainer.basic import Trainer
    torch.manual_seed(0)
    plain, attn = Trainer(recipe_2a(dtype, False)), Trainer(recipe_2a(dtype, True))
    x = torch.randn(B, MEL, T, device="cuda")
    y = torch.randint(0, 117, (B, 1), device="cuda")
    t = timed({"without_attention": lambda: plain.train_step((x, y)),
               "attention_0_1": lambda: attn.train_step((x, y))}, 2, 4, 7)
    a, b = t["without_attention"]["median_us"], t["attention_0_1"]["median_us"]
    for name, v in t.items():
        print(f"{dtype} vqvae2a step {name}: median {v['median_us'] / 1e3:.3f} ms (min {v['min_us'] / 1e3:.3f}, "
              f"max {v['max_us'] / 1e3:.3f})", flush=True)
    print(f"{dtype} vqvae2a step: attention.0 + attention.1 add {(b - a) / 1e3:+.3f} ms ({100 * (b - a) / a:+.2f} %)",
          flush=True)
    return {"dtype": dtype, "shape": dict(B=B, T=T, mel=MEL), "step": t, "added_us": b - a,
            "parameters": {"without_attention": plain.engine.n_params, "attention_0_1": attn.engine.n_params}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--model", action="store_true", help="time the vqvae2a training step without / with attention")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attn_bench needs the MI355X"
    out = [(run_model if a.model else run_layer)(d) for d in a.dtypes.split(",")]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
