"""The hierarchical encoder and quantizer level on the MI355X: the masked layout
kernel vqx_nct_to_ntc_lrelu_bwd bit for bit, its use as the z_proj DGRAD's
residual, `vqvae2.Encoder` and `VectorQuantizer.forward` against the
reference's float64 fixtures (tests/golden/make_golden_vqvae2_model.py).

Bound (as tests/test_gpu_hier.py): the reference's own float32 run differs
from its float64 run by err32 per tensor; one sample of that rounding gets a
factor 8, with a floor of 16 ulp:
    max|got - f64| / max|f64| <= max(8 * err32, 16 * 2^-23)."""
import numpy as np
import pytest
import torch

from tests.hier_model_ref import ENC_CASES, LEVEL_CASES, ULP16, fast_encoder_case, fixture, run_restated_encoder
from tests.hier_ref import as_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vae_npvc_amd import ops
    return ops


def ratios(got, want, err32):
    r = {}
    for k, w in want.items():
        w = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float64)
        assert tuple(got[k].shape) == w.shape, k
        err = np.abs(got[k].double().cpu().numpy() - w).max() / np.abs(w).max()
        r[k] = err / max(8 * err32[k], ULP16)
    return r


def report(what, r):
    worst = max(r, key=r.get)
    print(f"{what}: worst error/bound {r[worst]:.3f} ({worst}); " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert all(np.isfinite(v) for v in r.values()), r
    assert r[worst] <= 1.0, r


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("dst_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 33, 7), (3, 128, 130), (2, 512, 64)])
def test_masked_layout_change_bit_for_bit(shape, dst_dtype):
    ops = _ops()
    B, C, T = shape
    gen = torch.Generator(device=DEV).manual_seed(11)
    g = torch.randn(B, C, T, device=DEV, generator=gen)
    wide = torch.randn(B * T, C + 24, device=DEV, generator=gen)
    a = wide[:, 8:8 + C] if shape == (2, 512, 64) else wide[:, :C].contiguous()  # a strided `a` in the last shape
    dst = torch.full((B * T, C), float("nan"), device=DEV, dtype=dst_dtype)
    ops.nct_to_ntc_lrelu_bwd(g, a, 0.2, dst)
    slope = torch.tensor(0.2, device=DEV)
    want = g.permute(0, 2, 1).reshape(-1, C) * torch.where(a > 0, torch.ones_like(slope), slope)
    assert torch.equal(dst, want.to(dst_dtype))  # the f32 product rounded once
    a16 = a.to(torch.bfloat16)  # a bf16 activation: only its sign is read
    dst2 = torch.empty_like(dst)
    ops.nct_to_ntc_lrelu_bwd(g, a16, 0.2, dst2)
    want2 = g.permute(0, 2, 1).reshape(-1, C) * torch.where(a16.float() > 0, torch.ones_like(slope), slope)
    assert torch.equal(dst2, want2.to(dst_dtype))


def test_dgrad_mask_with_masked_residual_is_the_two_step_expression():
    """conv_dgrad(mask=a, res=masked dfeat) against mask * (dgrad + dfeat).
    - Within 2 ulp of the f32 value wherever that is attainable: where mask == 1
      (the two forms are the same sum) and where the operands do not cancel
      (|result| at least half the larger operand).
    - Everywhere, cancelling elements included, the fused result is the
      same-order expression mask*dgrad + masked dfeat within 1 ulp of the result:
      either as two roundings or contracted into one fused multiply-add (the
      compiler may do either; the exact value is formed in float64, where the
      product of two f32 values is exact)."""
    ops = _ops()
    B, C, Z, T = 2, 32, 16, 24
    gen = torch.Generator(device=DEV).manual_seed(12)
    dz = torch.randn(B * T, Z, device=DEV, generator=gen)
    w = torch.randn(Z, C, device=DEV, generator=gen) / 4
    a = torch.randn(B * T, C, device=DEV, generator=gen)
    dfeat = torch.randn(B, C, T, device=DEV, generator=gen)
    res = ops.nct_to_ntc_lrelu_bwd(dfeat, a, 0.2, torch.empty(B * T, C, device=DEV))
    got, plain = torch.empty(B * T, C, device=DEV), torch.empty(B * T, C, device=DEV)
    kw = dict(T=T, cin=Z, cout=C, ntaps=1, pad=0)
    ops.conv_dgrad(dz, w, got, mask=a, mask_slope=0.2, res=res, **kw)
    ops.conv_dgrad(dz, w, plain, **kw)
    m = torch.where(a > 0, 1.0, 0.2)

    def ulps(x, ref):
        ulp = ref.abs().clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -23
        return (x.double() - ref.double()).abs() / ulp.double()

    want = m * (plain + dfeat.permute(0, 2, 1).reshape(-1, C))
    attainable = (m == 1.0) | (want.abs() >= 0.5 * torch.maximum((m * plain).abs(), res.abs()))
    assert int(attainable.sum()) > attainable.numel() // 2 and bool((m == 1.0).any()) and bool((~attainable).any())
    two_step = ulps(got, want)[attainable].max()
    two_round = (m * plain) + res
    one_round = (m.double() * plain.double() + res.double()).float()
    same_order = torch.minimum(ulps(got, two_round), ulps(got, one_round)).max()
    print(f"mask+res dgrad: {float(two_step):.2f} ulp of mask*(dgrad+dfeat) on {int(attainable.sum())} of "
          f"{attainable.numel()} elements; same-order form {float(same_order):.2f} ulp on all "
          f"(two roundings bit-equal: {bool(torch.equal(got, two_round))}, fma bit-equal: "
          f"{bool(torch.equal(got, one_round))})")
    assert float(two_step) <= 2.0
    assert float(same_order) <= 1.0


# ------------------------------------------------------------------ encoder
def build_encoder(args, sd, dtype="fp32"):
    from vae_npvc_amd.model.vqvae2 import Encoder
    enc = Encoder(**args, compute_dtype=dtype)
    enc.load_state_dict({k: torch.from_numpy(as_numpy(v)) for k, v in sd.items()}, strict=True)
    return enc.cuda()


def run_encoder(enc, x, dz, dfeat, x_grad=True):
    enc.zero_grad(set_to_none=True)
    t = lambda a: torch.from_numpy(as_numpy(a)).float().cuda()  # noqa: E731
    xx = t(x).requires_grad_(x_grad)
    z, feat = enc(xx)
    pairs = [(o, t(g)) for o, g in ((z, dz), (feat, dfeat)) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    res = {"z": z.detach(), "feat": feat.detach()}
    if x_grad:
        res["dx"] = xx.grad
    res.update({k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None})
    return res


def enc_expected(meta, arr):
    want = {"z": arr["z"], "feat": arr["feat"], "dx": arr["dx"]}
    want.update({k: arr["grad." + k] for k in meta["grads"]})
    return want


@pytest.mark.parametrize("case", ENC_CASES)
def test_encoder_fp32_matches_the_float64_reference(case):
    meta, arr = fixture("vqenc", case)
    enc = build_encoder(meta["encoder"], {k: arr["param." + k] for k in meta["keys"]})
    dz, dfeat = arr.get("dz"), arr.get("dfeat")
    got = run_encoder(enc, arr["x"], dz, dfeat)
    assert set(meta["grads"]) <= set(got)
    report(f"vqenc {case} fp32", ratios(got, enc_expected(meta, arr), meta["err32"]))
    again = run_encoder(enc, arr["x"], dz, dfeat)
    assert set(got) == set(again) and all(torch.equal(got[k], again[k]) for k in got)  # equal bits
    nodx = run_encoder(enc, arr["x"], dz, dfeat, x_grad=False)  # the mel input of level 0 needs no gradient
    assert all(torch.equal(got[k], nodx[k]) for k in nodx)


def test_encoder_no_grad_gives_the_training_bits_and_keeps_no_graph():
    meta, arr = fixture("vqenc", "down2x2")
    enc = build_encoder(meta["encoder"], {k: arr["param." + k] for k in meta["keys"]})
    x = torch.from_numpy(arr["x"].copy()).cuda()
    z, feat = enc(x)
    assert z.requires_grad and feat.requires_grad
    assert z.shape == (meta["B"], 16, meta["Tz"]) and feat.shape == (meta["B"], 32, meta["Tz"])
    with torch.no_grad():
        zq, fq = enc(x)
    assert zq.grad_fn is None and fq.grad_fn is None
    assert torch.equal(z.detach(), zq) and torch.equal(feat.detach(), fq)
    with pytest.raises(ValueError):
        enc(x[:, :, :22])  # not a multiple of the down-sampling


_fast = {}


def fast_reference():
    if not _fast:
        args, sd, x, dz, dfeat = fast_encoder_case()
        _fast.update(case=(args, sd, x, dz, dfeat), f64=run_restated_encoder(args, sd, x, dz, dfeat),
                     f32=run_restated_encoder(args, sd, x, dz, dfeat, dtype=torch.float32),
                     ac=run_restated_encoder(args, sd, x, dz, dfeat, dtype=torch.float32, autocast=True))
    return _fast


def test_encoder_fast_kernels_fp32():
    """B=2, T=256, C=128: the GNSTATS / fused-skip-GEMM path."""
    ref = fast_reference()
    args, sd, x, dz, dfeat = ref["case"]
    err32 = {k: float((ref["f32"][k].double() - v).abs().max() / v.abs().max()) for k, v in ref["f64"].items()}
    got = run_encoder(build_encoder(args, sd), x, dz, dfeat)
    report("vqenc fast fp32", ratios(got, ref["f64"], err32))


def test_encoder_fast_kernels_bf16_within_autocast_error():
    ref = fast_reference()
    args, sd, x, dz, dfeat = ref["case"]
    got = run_encoder(build_encoder(args, sd, "bf16"), x, dz, dfeat)
    l2 = lambda a, w: float((a.double().cpu() - w).norm() / w.norm().clamp_min(1e-30))  # noqa: E731
    hip = {k: l2(got[k], w) for k, w in ref["f64"].items()}
    ac = {k: l2(ref["ac"][k], w) for k, w in ref["f64"].items()}
    ratio = {k: hip[k] / ac[k] for k in hip}
    wr = max(ratio, key=ratio.get)
    print(f"vqenc fast bf16: worst HIP / autocast error ratio {ratio[wr]:.3f} ({wr}); "
          + " ".join(f"{k}={v:.3f}" for k, v in ratio.items()))
    assert all(np.isfinite(v) for v in hip.values())
    # worst ratio measured on the MI355X: 1.317 (encode.2.stack.5.weight, a GroupNorm weight gradient; the
    # median is near 1); asserted with the decoder test's margin of 1.25 on top
    bound = 1.25 * 1.317
    assert all(hip[k] <= bound * ac[k] for k in hip), {k: (hip[k], ac[k]) for k in hip if hip[k] > bound * ac[k]}


# ------------------------------------------------------------------ quantizer level
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("case", LEVEL_CASES)
def test_quantizer_level_matches_the_float64_reference(case, weighted):
    from vae_npvc_amd.model.layers_vq import VectorQuantizer
    meta, arr = fixture("vqlevel", case)
    q = VectorQuantizer(meta["K"], meta["D"], normalize=meta["normalize"])
    q.load_state_dict({"embeddings": torch.from_numpy(arr["param.embeddings"].copy())})
    q.cuda()
    z = torch.from_numpy(arr["z"].copy()).cuda().requires_grad_()
    go = torch.from_numpy(arr["go"].copy()).cuda()
    w_qut, w_enc = meta["loss_weights"]
    if weighted:
        z_vq, lvl, qut, enc, detail = q(z, loss_weights=(w_qut, w_enc))
        assert not qut.requires_grad and not enc.requires_grad
        ((z_vq * go).sum() + lvl).backward()
    else:
        z_vq, qut, enc, detail = q(z)
        ((z_vq * go).sum() + w_qut * qut + w_enc * enc).backward()
    assert qut.dim() == 0 and enc.dim() == 0 and torch.is_tensor(detail["entropy"]) and detail["entropy"].is_cuda
    # the indices of forward's own launches (the fixture's smallest top-2 gap is >= 1e-3): every frame, none exempted
    assert meta["gap"] >= 1e-3
    want_idx = torch.from_numpy(arr["idx"].copy())
    assert torch.equal(q.forward_indices(z.detach()).cpu(), want_idx)
    assert torch.equal(q.encode(z.detach()).cpu(), want_idx)
    got = {"z_vq": z_vq.detach(), "z_qut_loss": qut.detach(), "z_enc_loss": enc.detach(),
           "entropy": detail["entropy"].detach(), "dz": z.grad, "dE": q.embeddings.grad}
    report(f"vqlevel {case} weighted={weighted}", ratios(got, {k: arr[k] for k in got}, meta["err32"]))
    if weighted and not meta["normalize"]:
        assert torch.equal(lvl.detach(), w_qut * qut + w_enc * enc)


def test_normalize_forward_writes_unit_rows_back_to_the_parameter():
    """embed_norm() inside forward (layers_vq.py:96): rows scaled away from 1 come back to unit norm within 2 ulp."""
    from vae_npvc_amd.model.layers_vq import VectorQuantizer
    meta, arr = fixture("vqlevel", "k16_norm")
    q = VectorQuantizer(meta["K"], meta["D"], normalize=True)
    scale = torch.linspace(0.5, 1.5, meta["K"]).view(-1, 1)
    q.load_state_dict({"embeddings": torch.from_numpy(arr["param.embeddings"].copy()) * scale})
    q.cuda()
    before = q.embeddings.detach().norm(dim=1)
    assert float((before - 1).abs().max()) > 0.4
    q(torch.from_numpy(arr["z"].copy()).cuda())
    n = q.embeddings.detach().double().norm(dim=1)
    print(f"row norms after forward: max |n - 1| = {float((n - 1).abs().max()) / 2.0 ** -23:.3f} ulp")
    assert float((n - 1).abs().max()) <= 2 * 2.0 ** -23


def test_quantizer_forward_early_exit_and_unbuilt_width():
    from vae_npvc_amd.model.layers_vq import VectorQuantizer
    q = VectorQuantizer(16, 64).cuda()
    q.quantize = False
    z = torch.randn(2, 64, 5, device=DEV)
    out = q(z)
    assert out[0] is z and len(out) == 4 and float(out[1]) == 0.0
    with pytest.raises(NotImplementedError):
        VectorQuantizer(16, 32).cuda()(torch.randn(2, 32, 5, device=DEV))
