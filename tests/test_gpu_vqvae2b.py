"""vqvae2b on the MI355X (-m gpu):

  * vqx_upsample_cat_bwd_to: with fp32 levels bit-equal to
    vqx_upsample_cat_bwd, with bf16 levels that fp32 result rounded to nearest
    even by torch; bit-stable; nothing written beside a level's columns;
  * an unconditioned `vqvae2.Decoder` (forward((x, None))) against a float64
    torch restatement of its blocks, bound as tests/test_gpu_hier.py bounds the
    conditioned one (max|got - f64| / max|f64| <= max(8 * err32, 16 * 2^-23)
    per tensor, err32 the restatement's own float32 error), and a conditioned
    one through `_DecoderFn` bit-equal to `decoder_rows` + `decoder_rows_bwd`
    called on rows;
  * the fused decode side (`vqvae2b.decode_side`) bit-identical to the same
    decoders composed from `Decoder` modules and `upsample_cat`: the launches
    that compute, and the bits they read, are the same;
  * `vqvae2b.Model` against the reference's float64 fixtures
    (tests/golden/make_golden_vqvae2b.py, vq2b_<case>) step by step under the
    stored seeds, then encode and infer with a speaker per level; convert;
    bf16; this package's Trainer and the reference trainer's loop.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.hier_model_ref import ULP16, fixture
from tests.test_gpu_hier import max_ratios
from tests.test_gpu_hier import report as report_restated
from tests.test_gpu_hier_encoder import ratios, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODEL_CASES = ("ema_gst", "plain_last", "pooled_ema")
TRAIN = dict(learning_rate=1e-3, max_grad_norm=0.5, optim_type="Adam", lr_scheduler="StepLR",
             lr_param={"step_size": 1, "gamma": 0.5})


def reseed(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)


# ------------------------------------------------------------------ kernel
# case: B, T, level lengths, level channels
BWD_TO = {"T7": (2, 7, (7, 3, 1), (4, 8, 12)), "T130": (1, 130, (130, 32), (8, 4)),
          "T40_chunked": (2, 40, (1, 40), (8, 4))}  # a 40-frame segment: the eight-chunk summation


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(BWD_TO))
def test_upsample_cat_bwd_to_stores_the_same_sums(case, dtype):
    from vae_npvc_amd import ops
    B, T, lens, chans = BWD_TO[case]
    torch.manual_seed(31)
    width = sum(chans)
    dout = torch.randn(B * T, width + 8, device=DEV).to(dtype)[:, :width]  # ld > C on the full-rate side

    def levels(dt, fill):  # every level inside a wider buffer (ld > C)
        bufs = [torch.full((B * Tl, C + 4), fill, device=DEV, dtype=dt) for Tl, C in zip(lens, chans)]
        return bufs, [b[:, :C] for b, C in zip(bufs, chans)]
    _, base = levels(torch.float32, -7.0)
    ops.upsample_cat_bwd(base, B, T, dout)
    for dt in (torch.float32, torch.bfloat16):
        bufs, got = levels(dt, -7.0)
        ops.upsample_cat_bwd_to(got, B, T, dout)
        bufs2, again = levels(dt, 5.0)
        ops.upsample_cat_bwd_to(again, B, T, dout)
        for l, (g, a, b, buf, C) in enumerate(zip(got, again, base, bufs, chans)):
            assert g.dtype == dt
            assert torch.equal(g, b.to(dt)), (case, dt, l)  # fp32: the same bits; bf16: rounded once, to nearest even
            assert torch.equal(g, a), (case, dt, l)
            assert bool((buf[:, C:] == -7.0).all()), (case, dt, l)
    # mixed level dtypes are refused on the host
    with pytest.raises(ValueError, match="one dtype"):
        ops.upsample_cat_bwd_to([base[0], base[1].to(torch.bfloat16)], B, T, dout)


def test_upsample_cat_bwd_to_limits_return_minus_one():
    """With live device buffers: a bad level_dtype and each inherited limit return -1 and leave the levels untouched."""
    from vae_npvc_amd import _lib as L
    lib = L.load()
    B, T = 2, 7
    dout = torch.randn(B * T, 16, device=DEV)
    lv = torch.full((B * 3, 8), -7.0, device=DEV)

    def arr(z=None, Tl=3, C=8, ld=8):
        a = (L.HierLevel * 1)()
        a[0].z, a[0].T_l, a[0].C, a[0].ld = (lv.data_ptr() if z is None else z), Tl, C, ld
        return a
    s = torch.cuda.current_stream().cuda_stream
    F32, BF16 = L.VQX_F32, L.VQX_BF16
    bad = [(arr(), 1, B, T, dout.data_ptr(), 16, F32, 5), (arr(), 0, B, T, dout.data_ptr(), 16, F32, BF16),
           (arr(), 9, B, T, dout.data_ptr(), 16, F32, BF16), (arr(), 1, B, T, dout.data_ptr(), 16, 3, F32),
           (arr(), 1, 0, T, dout.data_ptr(), 16, F32, F32), (arr(), 1, B, 0, dout.data_ptr(), 16, F32, F32),
           (arr(), 1, B, T, 0, 16, F32, F32), (arr(), 1, B, T, dout.data_ptr() + 4, 16, F32, F32),
           (arr(z=0), 1, B, T, dout.data_ptr(), 16, F32, F32), (arr(z=lv.data_ptr() + 4), 1, B, T, dout.data_ptr(), 16, F32, F32),
           (arr(Tl=8), 1, B, T, dout.data_ptr(), 16, F32, F32), (arr(Tl=0), 1, B, T, dout.data_ptr(), 16, F32, F32),
           (arr(C=6), 1, B, T, dout.data_ptr(), 16, F32, F32), (arr(ld=4), 1, B, T, dout.data_ptr(), 16, F32, F32),
           (arr(ld=10), 1, B, T, dout.data_ptr(), 16, F32, F32), (arr(), 1, B, T, dout.data_ptr(), 4, F32, F32),
           (arr(), 1, B, T, dout.data_ptr(), 18, F32, F32)]
    for args in bad:
        assert lib.vqx_upsample_cat_bwd_to(*args, s) == -1, args[1:]
        assert b"vqx_upsample_cat_bwd_to" in lib.vqx_last_error()
    torch.cuda.synchronize()
    assert bool((lv == -7.0).all())


# ------------------------------------------------------------------ unconditioned decoder
DEC_ARGS = dict(in_channels=[32], out_channels=[32], upsample_scales=[1], cond_channels=0, skip_channels=16,
                final_channels=24, kernel_size=3, dilation=True, stack_kernel_size=3, stacks=[2],
                use_weight_norm=True, use_causal_conv=False)


def restated_unconditioned(args, params, x):
    """Decoder(**args).forward((x, None)) of the reference (vqvae2b.py:374-393, layers.py:218-249 with conv_cond
    None) in plain torch; tests/hier_ref.restated_decoder without the conditioning term."""
    def conv_w(pre):
        return torch._weight_norm(params[pre + ".weight_v"], params[pre + ".weight_g"], 0)
    k, ks = args["kernel_size"], args["stack_kernel_size"]
    i, skips = 0, 0.0
    for cout, nst in zip(args["out_channels"], args["stacks"]):
        x = F.conv_transpose1d(x, conv_w(f"layers.{i}"), params[f"layers.{i}.bias"], padding=(k - 1) // 2)
        i += 1
        for j in range(nst):
            d = 2 ** j if args["dilation"] else 1
            pre = f"layers.{i}"
            h = F.conv_transpose1d(x, conv_w(pre + ".conv_in"), params[pre + ".conv_in.bias"],
                                   padding=(ks - 1) // 2 * d, dilation=d)
            h = F.group_norm(h, 2, params[pre + ".norm_layer.weight"], params[pre + ".norm_layer.bias"], eps=1e-5)
            g = torch.tanh(h[:, :cout]) * torch.sigmoid(h[:, cout:])
            rs = F.conv1d(g, conv_w(pre + ".res_skip_layers"), params[pre + ".res_skip_layers.bias"])
            x = rs[:, :cout] + x
            skips = skips + rs[:, cout:]
            i += 1
    y = skips * math.sqrt(1.0 / i)
    y = F.conv1d(F.relu(y), conv_w("final_layer.1"), params["final_layer.1.bias"])
    return F.conv1d(F.relu(y), conv_w("final_layer.3"), params["final_layer.3.bias"])


def seeded_decoder(args, seed, dtype="fp32"):
    from vae_npvc_amd.model.vqvae2 import Decoder
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    dec = Decoder(**args, compute_dtype=dtype)
    with torch.no_grad():  # move the GroupNorm affine off its 1 / 0 initial values
        for k, v in dec.named_parameters():
            if "norm_layer" in k:
                v.add_(0.2 * torch.randn(v.shape, generator=g))
    return dec


@pytest.mark.parametrize("T", [64, 37])
def test_unconditioned_decoder_matches_the_float64_restatement(T):
    B = 2
    dec = seeded_decoder(DEC_ARGS, 9800 + T)
    assert not any(".conv_cond." in k for k in dec.state_dict())
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    g = torch.Generator().manual_seed(T)
    x, go = torch.randn(B, 32, T, generator=g), torch.randn(B, 24, T, generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        params = {k: v.clone().to(dt).requires_grad_() for k, v in sd.items()}
        xx = x.clone().to(dt).requires_grad_()
        out = restated_unconditioned(DEC_ARGS, params, xx)
        out.backward(go.to(dt))
        ref[dt] = dict({"out": out.detach(), "dx": xx.grad}, **{k: p.grad for k, p in params.items()})
    f64 = ref[torch.float64]
    err32 = {k: float((ref[torch.float32][k].double() - v).abs().max() / v.abs().max()) for k, v in f64.items()}
    dec = dec.cuda()
    xx = x.cuda().requires_grad_()
    out = dec((xx, None))
    out.backward(go.cuda())
    got = dict({"out": out.detach(), "dx": xx.grad}, **{k: p.grad for k, p in dec.named_parameters()})
    assert set(got) == set(f64)
    report_restated(f"unconditioned decoder T={T} fp32", max_ratios(got, f64, err32))
    with torch.no_grad():
        quiet = dec((xx.detach(), None))
        rows = torch.empty(B * T, 32, device=DEV)
        from vae_npvc_amd import ops
        ops.nct_to_ntc(x.cuda(), rows)
        by_rows = dec.forward_rows(rows, B, T, None)
    assert quiet.grad_fn is None and torch.equal(quiet, out.detach())
    assert torch.equal(by_rows.view(B, T, -1).transpose(1, 2), out.detach())
    with pytest.raises(ValueError, match="unconditioned"):
        dec.forward_rows(rows, B, T, [torch.zeros(B, 16, device=DEV)])
    with pytest.raises(ValueError, match="unconditioned"):
        dec((xx, torch.zeros(B, 16, T, device=DEV)))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conditioned_decoder_equals_the_rows_functions_bit_for_bit(dtype):
    """`_DecoderFn` (through Decoder.forward) against `decoder_rows` + `decoder_rows_bwd` called directly with the
    same layout changes around them: the split moved no launch."""
    from vae_npvc_amd import ops
    from vae_npvc_amd.model.hier_common import DT, to_nct, to_rows
    from vae_npvc_amd.model.hier_decoder import Plan, decoder_rows, decoder_rows_bwd
    B, T, lens = 2, 37, (1, 9)
    dec = seeded_decoder(dict(DEC_ARGS, cond_channels=24), 9850, dtype).cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 32, T, generator=g).cuda().requires_grad_()
    levels = [torch.randn(B, C, Tl, generator=g).cuda().requires_grad_() for C, Tl in zip((16, 8), lens)]
    go = torch.randn(B, 24, T, generator=g).cuda()
    out = dec((x, levels))
    out.backward(go)
    plan, dt = dec.plan, DT[dtype]
    with torch.no_grad():
        ts = [t.detach().float() for t in Plan.tensors(dec)]
        x2 = ops.nct_to_ntc(x.detach().contiguous(), torch.empty(B * T, 32, device=DEV, dtype=dt))
        rows = [to_rows(z.detach()) for z in levels]
        xhat, keep = decoder_rows(plan, x2, B, T, rows, lens, ts)
        dxhat = ops.nct_to_ntc(go, torch.empty(B * T, 24, device=DEV, dtype=dt))
        dx, dc, grads = decoder_rows_bwd(plan, B, T, keep, dxhat)
        dl = [torch.empty(B * Tl, z.shape[1], device=DEV) for z, Tl in zip(levels, lens)]
        ops.upsample_cat_bwd(dl, B, keep.Tc, dc)
    assert torch.equal(to_nct(xhat, B, T), out.detach())
    assert torch.equal(to_nct(dx, B, T), x.grad)
    for d, z in zip(dl, levels):
        assert torch.equal(to_nct(d, B, z.shape[2]), z.grad)
    # dL/d(effective weight) through torch's weight norm, as autograd applies it to the function's outputs
    live = [(t, gr) for t, gr in zip(Plan.tensors(dec), grads) if t.requires_grad]
    params = list(dec.parameters())
    want = [p.grad.clone() for p in params]
    dec.zero_grad(set_to_none=True)
    torch.autograd.backward([t for t, _ in live], [gr.reshape(t.shape) for t, gr in live])
    for p, w in zip(params, want):
        assert torch.equal(p.grad, w)


# ------------------------------------------------------------------ decode side
def _side_case(dtype, seed=9870):
    from vae_npvc_amd.model.vqvae2 import Decoder
    arch = fixture("vq2b", "ema_gst")[0]["arch"]
    torch.manual_seed(seed)
    decs = [Decoder(**arch[f"decoder.{i}"], compute_dtype=dtype).cuda() for i in range(3)]
    final = Decoder(**arch["final_decoder"], compute_dtype=dtype).cuda()
    g = torch.Generator().manual_seed(seed)
    B, shapes = 2, ((64, 64), (64, 16), (32, 1))
    zs = [torch.randn(B, C, Tl, generator=g).cuda().requires_grad_() for C, Tl in shapes]
    ys = [torch.randn(B, 16, generator=g).cuda().requires_grad_() for _ in shapes]
    go = torch.randn(B, 24, 64, generator=g).cuda()
    return decs, final, zs, ys, go


def _collect(out, go, decs, final, zs, ys):
    for t in (*zs, *ys):
        t.grad = None
    for d in (*decs, final):
        d.zero_grad(set_to_none=True)
    out.backward(go)
    res = {"xhat": out.detach()}
    res.update({f"dz.{i}": z.grad.clone() for i, z in enumerate(zs)})
    res.update({f"dy.{i}": y.grad.clone() for i, y in enumerate(ys)})
    for n, d in enumerate((*decs, final)):
        res.update({f"dec{n}.{k}": p.grad.clone() for k, p in d.named_parameters()})
    return res


@pytest.mark.parametrize("upsample_last", [False, True], ids=["stretch_first", "stretch_last"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fused_decode_side_equals_the_composition_bit_for_bit(dtype, upsample_last):
    from vae_npvc_amd.model.vqvae2 import upsample_cat
    from vae_npvc_amd.model.vqvae2b import decode_side
    decs, final, zs, ys, go = _side_case(dtype)
    time = 64
    fused = _collect(decode_side(decs, final, zs, ys, time, upsample_last), go, decs, final, zs, ys)
    outs = []
    for d, z, y in zip(decs, zs, ys):
        cond = [y.unsqueeze(-1)]  # (B, y_dim, 1): the one-frame speaker level
        outs.append(d((z, cond)) if upsample_last else d((upsample_cat([z], time), cond)))
    composed = _collect(final((upsample_cat(outs, time), None)), go, decs, final, zs, ys)
    assert set(fused) == set(composed) and all(v is not None for v in fused.values())
    diff = [k for k in fused if not torch.equal(fused[k], composed[k])]
    assert not diff, (dtype, upsample_last, diff)
    assert all(bool(torch.isfinite(v).all()) for v in fused.values())
    assert all(float(fused[k].abs().max()) > 0 for k in fused if k[:3] in ("xha", "dz.", "dy."))
    with torch.no_grad():
        quiet = decode_side(decs, final, zs, ys, time, upsample_last)
    assert quiet.grad_fn is None and torch.equal(quiet, fused["xhat"])


# ------------------------------------------------------------------ model
def state_dict(meta, arr):
    return {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}


def build_model(meta, arr, **over):
    from vae_npvc_amd.model.vqvae2b import Model
    m = Model(dict(meta["arch"], **over))
    assert list(m.state_dict().keys()) == meta["keys"]
    m.load_state_dict(state_dict(meta, arr), strict=True)
    return m.cuda().train()


def batch(arr):
    return torch.from_numpy(arr["x"].copy()).cuda(), torch.from_numpy(arr["y"].copy()).cuda()


def codebooks(m):
    return [q for q in m.quantizers if hasattr(q, "embeddings")]


def record_indices(m, sink):
    """Every codebook lookup of a forward appends its indices, in the order they run (tests/test_gpu_vqvae2a.py)."""
    from vae_npvc_amd.model.layers_vq import EMAVectorQuantizer
    hooks = []
    for q in codebooks(m):
        if isinstance(q, EMAVectorQuantizer):
            hooks.append(q.register_forward_hook(lambda mod, inp, out: sink.append(mod.last_indices.cpu())))
        else:
            hooks.append(q.register_forward_pre_hook(
                lambda mod, inp: sink.append(mod.forward_indices(inp[0].detach()).cpu())))
    return hooks


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_steps_encode_and_infer_match_the_float64_reference(case):
    meta, arr = fixture("vq2b", case)
    assert meta["gap"] >= 1e-3
    m = build_model(meta, arr)
    x, y = batch(arr)
    ids = []
    hooks = record_indices(m, ids)
    reseed(meta["run_seed"])
    for n in range(1, meta["steps"] + 1):
        p = f"s{n}."
        m.zero_grad(set_to_none=True)
        del ids[:]
        xhat, loss, detail = m((x, y))
        assert list(detail) == meta["loss_keys"][n - 1] and all(isinstance(v, float) for v in detail.values())
        loss.backward()
        assert len(ids) == meta["lookups"][n - 1]
        for j, idx in enumerate(ids):
            assert torch.equal(idx, torch.from_numpy(arr[p + f"idx.{j}"].copy())), (n, j)
        got = {p + "xhat": xhat.detach()}
        got.update({p + "loss." + k: torch.tensor(v, dtype=torch.float64) for k, v in detail.items()})
        got.update({p + "grad." + k: g.grad for k, g in m.named_parameters() if g.grad is not None})
        got.update({p + "buf." + k: b.detach().clone() for k, b in m.named_buffers() if b.is_floating_point()})
        assert sorted(k for k, g in m.named_parameters() if g.grad is not None) == sorted(meta["grads"])
        want = {k: arr[k] for k in got if k not in meta["abs32"]}
        assert set(want) == {k for k in meta["err32"] if k.startswith(p)}
        report(f"vq2b {case} step {n}", ratios(got, want, meta["err32"]))
        for k, a32 in meta["abs32"].items():  # exactly zero in exact arithmetic
            if k.startswith(p):
                scale = float(np.abs(arr[k[:-4] + "weight"]).max())
                assert float(got[k].abs().max()) <= max(8 * a32, ULP16 * scale), k
        for k, b in m.named_buffers():
            if not b.is_floating_point():
                assert bool(b) == bool(arr[p + "buf." + k]), k
        assert float(loss.detach()) == detail["Total"]
    for h in hooks:
        h.remove()
    # encode and infer in eval mode after the last step
    m.eval()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    codes = m.encode(x)
    assert len(codes) == m.levels and [int(c.shape[-1]) for c in codes] == meta["level_lengths"]
    got, want = {}, {}
    for i, c in enumerate(codes):
        if c.is_floating_point():
            got[f"enc.{i}"], want[f"enc.{i}"] = c, arr[f"enc.{i}"]
        else:
            assert c.dtype == torch.int64 and torch.equal(c.cpu(), torch.from_numpy(arr[f"enc.{i}"].copy())), i
    ys = torch.from_numpy(arr["ys"].copy()).cuda()
    out = m.infer((x, ys))
    assert not out.requires_grad and tuple(out.shape) == tuple(x.shape)
    got["infer"], want["infer"] = out, arr["infer"]
    report(f"vq2b {case} encode + infer", ratios(got, want, meta["err32"]))
    assert torch.equal(out, m.decode((codes, ys), time=x.shape[2]))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize("case", MODEL_CASES)
def test_convert_is_the_eval_forward_and_infer_agrees_with_it(case):
    meta, arr = fixture("vq2b", case)
    m = build_model(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    m((x, y))  # one training forward: the EMA codebooks are initialised
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out = m.convert((x, y))
    assert m.training and not out.requires_grad
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    m.eval()
    with torch.no_grad():
        xhat, _, detail = m((x, y))
    assert torch.equal(out, xhat)
    assert [k for k in detail if k.startswith("quanti_err")] == [f"quanti_err.{k}" for k in range(meta["lookups"][0])]
    m.train()
    for k, v in before.items():  # the eval forward renormalised a plain codebook in place: put the bits back
        m.state_dict()[k].copy_(v)
    # one speaker for every level through the code path: the same rendering, the codebook rows normalised by other
    # launches, so within the fixture's bound for `infer` and not bit for bit
    same = m.infer((x, y.expand(-1, m.levels).contiguous()))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    err = float((same.double() - out.double()).abs().max() / out.double().abs().max())
    bound = max(8 * meta["err32"]["infer"], ULP16)
    print(f"vq2b {case}: infer vs convert error/bound {err / bound:.3f}")
    assert err <= bound, (err, bound)


def test_decoder_hier_drives_convert():
    from vae_npvc_amd.decoder.hier import Decoder
    meta, arr = fixture("vq2b", "ema_gst")
    m = build_model(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    m((x, y))
    dec = Decoder.__new__(Decoder)
    dec.model = m
    assert torch.equal(dec.decode_step(x[:1], y[:1]), m.convert((x[:1], y[:1])))


def test_bf16_step_is_finite_with_the_same_keys():
    meta, arr = fixture("vq2b", "ema_gst")
    m = build_model(meta, arr, compute_dtype="bf16")
    x, y = batch(arr)
    reseed(meta["run_seed"])
    xhat, loss, detail = m((x, y))
    loss.backward()
    assert list(detail) == meta["loss_keys"][0] and all(np.isfinite(v) for v in detail.values())
    assert bool(torch.isfinite(xhat).all())
    assert sorted(k for k, p in m.named_parameters() if p.grad is not None) == sorted(meta["grads"])
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    assert all(bool(torch.isfinite(b).all()) for b in m.buffers())


def trainer(meta, arr, **over):
    from vae_npvc_amd.trainer.basic import Trainer
    cfg = dict(meta["arch"], **TRAIN, model_type="vae_npvc_amd.model.vqvae2b",
               trainer_type="vae_npvc_amd.trainer.basic", **over)
    tr = Trainer(cfg)
    tr.model.load_state_dict(state_dict(meta, arr))
    assert tr.engine.params_intact()
    return tr


def test_trainer_steps_validates_and_checkpoints(tmp_path):
    meta, arr = fixture("vq2b", "ema_gst")
    tr = trainer(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    totals = []
    for s in range(2):
        it, detail = tr.train_step((x, y))
        assert it == s + 1 and list(detail) == meta["loss_keys"][s] and all(np.isfinite(v) for v in detail.values())
        totals.append(detail["Total"])
    assert totals[0] != totals[1]
    assert all(bool(q.emb_init) for q in codebooks(tr.model))
    # valid_step leaves parameters and buffers bit-identical, and the model in training mode
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    rng = torch.get_rng_state()
    vdetail = tr.valid_step((x, y))
    assert list(vdetail) == ["Total", "VQ loss", "X like", "quanti_err.0", "quanti_err.1"]
    assert tr.model.training and torch.equal(torch.get_rng_state(), rng)
    assert all(torch.equal(v, before[k]) for k, v in tr.model.state_dict().items())
    # checkpoint round trip: parameters, EMA buffers, emb_init, moments, iteration
    path = tmp_path / "ck.pt"
    tr.save_checkpoint(str(path))
    tr2 = trainer(meta, arr)
    assert not any(bool(q.emb_init) for q in codebooks(tr2.model))
    assert tr2.load_checkpoint(str(path)) == 2 and tr2.iteration == 2
    for k, v in tr2.model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(q.initialized for q in codebooks(tr2.model))
    assert torch.equal(tr2.engine.exp_avg, tr.engine.exp_avg) and torch.equal(tr2.engine.exp_avg_sq, tr.engine.exp_avg_sq)
    # the two trainers continue alike
    reseed(11)
    _, d1 = tr.train_step((x, y))
    reseed(11)
    _, d2 = tr2.train_step((x, y))
    assert d1 == d2
    for (k, a), b in zip(tr.model.state_dict().items(), tr2.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_trainer_refuses_data_parallel_engine():
    meta, arr = fixture("vq2b", "pooled_ema")
    m = build_model(meta, arr)
    with pytest.raises(NotImplementedError, match="data parallel"):
        m.engine().attach_comm(object())


def test_reference_trainer_loop_runs():
    meta, arr = fixture("vq2b", "plain_last")
    m = build_model(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    totals = []
    for _ in range(2):
        opt.zero_grad()
        _, loss, detail = m((x, y))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10)
        opt.step()
        totals.append(detail["Total"])
        assert all(np.isfinite(v) for v in detail.values())
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert all(bool(torch.isfinite(b).all()) for b in m.buffers())
    assert totals[0] != totals[1]
