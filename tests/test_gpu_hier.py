"""The hierarchical decoder's pieces on the MI355X (-m gpu):

  * vqx_upsample_cat_fwd against torch's indexing, bit for bit;
  * vqx_upsample_cat_bwd against the float64 segment sums, within
    r * 2^-24 * sum|terms| per element (r = the longest segment: a chain of at
    most r fp32 additions, each rounding by at most 2^-24 of a partial sum that
    never exceeds sum|terms|), and bit-stable;
  * the conv forward with a segmented row bias (vqx_conv_args.rowbias_T), per
    kernel family, bit for bit the same call without a row bias plus
    P[segment] added in fp32 (the epilogue's own order: bias, then row bias);
  * model.vqvae2.Decoder against the reference's float64 fixtures
    (tests/golden/vqdec_*) with the GST bound
    max|got - f64| / max|f64| <= max(8 * err32, 16 * 2^-23) per tensor, and at a
    fast-kernel shape against the float64 restatement pinned by
    tests/test_hier_host.py; bf16 per tensor within 1.25x of the restatement's
    own error under torch CPU bf16 autocast (relative L2 against float64).

Worst ratios measured on the MI355X are in DESIGN.md ("Hierarchical decoder").
"""
import numpy as np
import pytest
import torch

from tests.hier_ref import CASES, ULP16, as_numpy, expected, fast_case, fixture, fixture_cond, run_restated

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vae_npvc_amd import ops
    return ops


def src_of(T, Tl):
    return torch.clamp(torch.arange(T, device=DEV) // (T // Tl), max=Tl - 1)


# ------------------------------------------------------------------ upsample_cat
UPCAT = {"T20_v4": (2, 20, (1, 3, 8, 20), (8, 4, 12, 16)), "T20_v8": (2, 20, (1, 3, 8, 20), (8, 16, 24, 8)),
         "T256": (2, 256, (1, 3, 64), (8, 16, 24)), "T256_v4": (2, 256, (1, 3, 64), (4, 20, 8))}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(UPCAT))
def test_upsample_cat_fwd_equals_indexing_bit_for_bit(case, dtype):
    ops = _ops()
    B, T, lens, chans = UPCAT[case]
    torch.manual_seed(11)
    levels = [torch.randn(B * Tl, C, device=DEV) for Tl, C in zip(lens, chans)]
    want = torch.cat([z.view(B, Tl, -1)[:, src_of(T, Tl)].reshape(B * T, -1) for z, Tl in zip(levels, lens)], dim=1)
    width = sum(chans)
    for ldo in (width, width + 8):  # a destination wider than the levels: nothing written beside the columns
        buf = torch.full((B * T, ldo), -7.0, device=DEV, dtype=dtype)
        ops.upsample_cat_fwd(levels, B, T, buf[:, :width] if ldo > width else buf)
        assert torch.equal(buf[:, :width], want.to(dtype)), (case, ldo)
        assert (buf[:, width:] == -7.0).all()
    # a level read from a wider buffer (ld > C)
    wide = torch.randn(B * lens[1], chans[1] + 4, device=DEV)
    lv = list(levels)
    lv[1] = wide[:, :chans[1]]
    out = torch.empty(B * T, width, device=DEV, dtype=dtype)
    ops.upsample_cat_fwd(lv, B, T, out)
    off = chans[0]
    assert torch.equal(out[:, off:off + chans[1]],
                       lv[1].reshape(B, lens[1], -1)[:, src_of(T, lens[1])].reshape(B * T, -1).to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(UPCAT))
def test_upsample_cat_bwd_sums_segments(case, dtype):
    ops = _ops()
    B, T, lens, chans = UPCAT[case]
    torch.manual_seed(12)
    width = sum(chans)
    dout = torch.randn(B * T, width + 8, device=DEV).to(dtype)[:, :width]
    runs = []
    for _ in range(2):
        dl = [torch.full((B * Tl, C), float("nan"), device=DEV) for Tl, C in zip(lens, chans)]
        ops.upsample_cat_bwd(dl, B, T, dout)
        runs.append(dl)
    off, worst = 0, 0.0
    for got, again, Tl, C in zip(runs[0], runs[1], lens, chans):
        assert torch.equal(got, again)  # fixed summation order: equal bits
        d = dout[:, off:off + C].double().view(B, T, C)
        idx = src_of(T, Tl)
        want = torch.zeros(B, Tl, C, device=DEV, dtype=torch.float64).index_add_(1, idx, d)
        mass = torch.zeros(B, Tl, C, device=DEV, dtype=torch.float64).index_add_(1, idx, d.abs())
        r = T - (Tl - 1) * (T // Tl)  # the longest (tail) segment
        err = (got.double().view(B, Tl, C) - want).abs()
        bound = r * 2.0 ** -24 * mass
        assert (err <= bound).all(), (case, Tl, float((err / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        if T // Tl == 1 and Tl == T:
            assert torch.equal(got, dout[:, off:off + C].float())  # T_l = T: a conversion
        off += C
    print(f"upsample_cat_bwd {case} {dtype}: worst error/bound {worst:.3f}")


def test_upsample_autograd_equals_torch():
    """model.vqvae2.upsample / upsample_cat on (B, C, T) tensors, forward and gradient."""
    from vae_npvc_amd.model.vqvae2 import upsample, upsample_cat
    torch.manual_seed(13)
    B, T = 2, 20
    zs = [torch.randn(B, C, Tl, device=DEV, requires_grad=True) for C, Tl in ((8, 1), (16, 3), (4, 8))]
    go = torch.randn(B, 28, T, device=DEV)
    out = upsample_cat(zs, T)
    want = torch.cat([z[:, :, src_of(T, z.shape[2])] for z in zs], dim=1)
    assert torch.equal(out, want)
    out.backward(go)
    got = [z.grad.clone() for z in zs]
    for z in zs:
        z.grad = None
    want.backward(go)
    for g, z in zip(got, zs):
        assert torch.allclose(g, z.grad, rtol=1e-6, atol=1e-6)
    assert torch.equal(upsample(zs[1].detach(), T), zs[1].detach()[:, :, src_of(T, 3)])


# ------------------------------------------------------------------ segmented row bias
POL = {"auto": 0, "tr128": 4, "tall256": 2, "tall512": 3}
# family: dtype, policy, B, T, cin, cout, Tc list, whether the family writes GNSTATS tiles here
FAMILIES = {
    "fp32": (torch.float32, "auto", 13, 20, 32, 64, (3,), False),     # 128-frame tiles span several utterances
    "bf16_im2col": (torch.bfloat16, "auto", 3, 160, 64, 128, (40,), False),
    "bf16_tr128": (torch.bfloat16, "tr128", 2, 256, 128, 256, (64, 3), True),
    "bf16_tall256": (torch.bfloat16, "tall256", 2, 256, 128, 256, (64, 3), True),
    "bf16_tall512": (torch.bfloat16, "tall512", 2, 256, 128, 256, (64, 3), True),  # the ping-pong kernel
}
SEG_CASES = [(f, tc) for f, v in FAMILIES.items() for tc in v[6]]


def _conv_operands(family):
    dtype, pol, B, T, cin, cout, _, stats = FAMILIES[family]
    torch.manual_seed(21)
    x = torch.randn(B * T, cin, device=DEV).to(dtype)
    w = (torch.randn(cout, 3 * cin, device=DEV) / (3 * cin) ** 0.5).to(dtype)
    bias = torch.randn(cout, device=DEV)
    return dtype, POL[pol], B, T, cin, cout, stats, x, w, bias


@pytest.mark.parametrize("family,Tc", SEG_CASES, ids=[f"{f}-Tc{tc}" for f, tc in SEG_CASES])
def test_conv_segmented_rowbias_is_the_plain_call_plus_the_segment_row(family, Tc):
    ops = _ops()
    dtype, pol, B, T, cin, cout, stats, x, w, bias = _conv_operands(family)
    N = B * T
    P = torch.randn(B * Tc, cout, device=DEV)
    kw = dict(T=T, cin=cin, cout=cout, ntaps=3, pad=1, bias=bias, out_f32=True)
    plain, seg = torch.empty(N, cout, device=DEV), torch.empty(N, cout, device=DEV)
    with ops.kernel_policy(pol):
        ops.conv_fwd(x, w, plain, **kw)
        if stats:
            tiles = torch.full((N // 128 * (cout // 128) * 4,), float("nan"), device=DEV)
            ops.conv_fwd(x, w, seg, rowbias=P, rowbias_T=Tc, gn_stats=tiles, gn_groups=2, **kw)
        else:
            ops.conv_fwd(x, w, seg, rowbias=P, rowbias_T=Tc, **kw)
    row = (torch.arange(B, device=DEV) * Tc).view(B, 1) + src_of(T, Tc).view(1, T)  # b*Tc + min(t // (T//Tc), Tc-1)
    want = plain + P[row.reshape(-1)]
    assert torch.equal(seg, want), (family, Tc, float((seg - want).abs().max()))
    if Tc == 3 and T == 256:
        assert int(row[0, 255]) == 2 and int(row[0, 254]) == 2 and int(row[0, 170]) == 2 and int(row[0, 169]) == 1
    if stats:  # the tiles are the statistics of the stored u (row bias included)
        mr_fused, mr_ref = torch.empty(B, 2, 2, device=DEV), torch.empty(B, 2, 2, device=DEV)
        ops.gn_finalize_tiles(tiles, N, T, cout, 2, mr_fused)
        ops.groupnorm_stats(seg, T, 2, torch.empty(B * 2 * 24, device=DEV), mr_ref)
        a, b = mr_fused.double().cpu(), mr_ref.double().cpu()
        rel = float((a - b).norm() / b.norm())
        assert rel < 1e-5, (family, Tc, rel)  # the bound of test_gnstats_epilogue_matches_standalone (fp32 values)


@pytest.mark.parametrize("family", ["fp32", "bf16_im2col", "bf16_tr128", "bf16_tall512"])
def test_rowbias_T_0_and_1_give_todays_bits(family):
    ops = _ops()
    dtype, pol, B, T, cin, cout, _, x, w, bias = _conv_operands(family)
    N = B * T
    rb = torch.randn(B, cout, device=DEV)
    outs = []
    with ops.kernel_policy(pol):
        for kw in ({}, {"rowbias_T": 0}, {"rowbias_T": 1}):
            for f32 in (True, False):
                y = torch.empty(N, cout, device=DEV, dtype=torch.float32 if f32 else dtype)
                ops.conv_fwd(x, w, y, T=T, cin=cin, cout=cout, ntaps=3, pad=1, bias=bias, rowbias=rb, out_f32=f32,
                             **kw)
                outs.append(y)
        plain = torch.empty(N, cout, device=DEV)
        ops.conv_fwd(x, w, plain, T=T, cin=cin, cout=cout, ntaps=3, pad=1, bias=bias, out_f32=True)
    for i in (2, 4):
        assert torch.equal(outs[0], outs[i]) and torch.equal(outs[1], outs[i + 1])
    assert torch.equal(outs[0], plain + rb.repeat_interleave(T, dim=0))


# ------------------------------------------------------------------ Decoder
def build_decoder(args, sd, dtype="fp32"):
    from vae_npvc_amd.model.vqvae2 import Decoder
    dec = Decoder(**args, compute_dtype=dtype)
    dec.load_state_dict({k: torch.from_numpy(as_numpy(v)) for k, v in sd.items()}, strict=True)
    return dec.cuda()


def run_decoder(dec, x, cond, go):
    """{"out", "dx", "d<cond name>"..., "<key>" gradient...} of one forward + backward."""
    dec.zero_grad(set_to_none=True)
    g = lambda a: torch.from_numpy(as_numpy(a)).float().cuda().requires_grad_()  # noqa: E731
    xx = g(x)
    tensor_c = not isinstance(cond, (list, tuple))
    cc = g(cond) if tensor_c else [g(z) for z in cond]
    out = dec((xx, cc))
    out.backward(torch.from_numpy(as_numpy(go)).float().cuda())
    res = {"out": out.detach(), "dx": xx.grad}
    if tensor_c:
        res["dc"] = cc.grad
    else:
        res.update({f"dlevel.{i}": z.grad for i, z in enumerate(cc)})
    res.update({k: p.grad.detach().clone() for k, p in dec.named_parameters()})
    return res


def max_ratios(got, want, err32):
    """{tensor: (max|got - f64| / max|f64|) / max(8 * err32, 16 * 2^-23)}"""
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


def same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", CASES)
def test_decoder_fp32_matches_the_float64_reference(case):
    meta, arr = fixture(case)
    dec = build_decoder(meta["decoder"], {k: arr["param." + k] for k in meta["keys"]})
    got = run_decoder(dec, arr["x"], fixture_cond(meta, arr), arr["go"])
    assert got["out"].shape == (meta["B"], 16, meta["T"])
    report(f"vqdec {case} fp32", max_ratios(got, expected(meta, arr), meta["err32"]))
    again = run_decoder(dec, arr["x"], fixture_cond(meta, arr), arr["go"])
    assert same_bits(got, again)  # two runs of one path: equal bits


def test_decoder_tail_case_through_a_prestretched_tensor_c():
    """The low-rate path's case run the reference's way: the levels stretched to
    T and stacked into c (B, 24, T) beforehand; the same bound holds, and the
    level gradients are the segment sums of dc."""
    meta, arr = fixture("tail")
    dec = build_decoder(meta["decoder"], {k: arr["param." + k] for k in meta["keys"]})
    levels = fixture_cond(meta, arr)
    T = meta["T"]
    c = np.concatenate([z[:, :, src_of(T, z.shape[2]).cpu().numpy()] for z in levels], axis=1)
    low = run_decoder(dec, arr["x"], levels, arr["go"])
    full = run_decoder(dec, arr["x"], c, arr["go"])
    want = expected(meta, arr)
    off = 0
    for i, z in enumerate(levels):  # fold dc back onto the levels (float64, on the host)
        d = full["dc"][:, off:off + z.shape[1]].double().cpu()
        idx = src_of(T, z.shape[2]).cpu()
        full[f"dlevel.{i}"] = torch.zeros(z.shape, dtype=torch.float64).index_add_(2, idx, d)
        off += z.shape[1]
    del full["dc"]
    report("vqdec tail fp32 via tensor c", max_ratios(full, want, meta["err32"]))
    keys = [k for k in low if not k.startswith("dlevel.")]
    print("vqdec tail: low-rate and full-rate paths agree bit for bit on "
          f"{sum(torch.equal(low[k], full[k]) for k in keys)} of {len(keys)} tensors "
          f"(out: {torch.equal(low['out'], full['out'])})")


def test_decoder_no_grad_gives_the_training_bits_and_keeps_no_graph():
    meta, arr = fixture("tail")
    dec = build_decoder(meta["decoder"], {k: arr["param." + k] for k in meta["keys"]})
    x = torch.from_numpy(arr["x"].copy()).cuda()
    levels = [torch.from_numpy(z.copy()).cuda() for z in fixture_cond(meta, arr)]
    train = dec((x, levels))
    assert train.requires_grad
    with torch.no_grad():
        quiet = dec((x, levels))
    assert not quiet.requires_grad and quiet.grad_fn is None
    assert torch.equal(train.detach(), quiet)
    for p in dec.parameters():
        p.requires_grad_(False)
    frozen = dec((x, levels))
    assert frozen.grad_fn is None and torch.equal(train.detach(), frozen)


def test_decoder_resampling_stages_raise():
    from vae_npvc_amd.model.vqvae2 import Decoder
    meta, _ = fixture("tail")
    with pytest.raises(NotImplementedError):
        Decoder(**dict(meta["decoder"], upsample_scales=[2]))


_fast = {}


def fast_reference():
    """The fast-kernel case and its restated float64 / float32 / bf16-autocast runs (computed once)."""
    if not _fast:
        args, sd, x, levels, go = fast_case()
        f64 = run_restated(args, sd, x, levels, go)
        f32 = run_restated(args, sd, x, levels, go, dtype=torch.float32)
        ac = run_restated(args, sd, x, levels, go, dtype=torch.float32, autocast=True)
        _fast.update(case=(args, sd, x, levels, go), f64=f64, f32=f32, ac=ac)
    return _fast


def test_decoder_fast_kernels_fp32():
    """B=2, T=256, C=128: the GNSTATS / gn_glu_fwd_tiles path and Tc = 64."""
    ref = fast_reference()
    args, sd, x, levels, go = ref["case"]
    err32 = {k: float((ref["f32"][k].double() - v).abs().max() / v.abs().max()) for k, v in ref["f64"].items()}
    dec = build_decoder(args, sd)
    got = run_decoder(dec, x, levels, go)
    report("vqdec fast fp32", max_ratios(got, ref["f64"], err32))


def test_decoder_fast_kernels_bf16_within_autocast_error():
    ref = fast_reference()
    args, sd, x, levels, go = ref["case"]
    dec = build_decoder(args, sd, "bf16")
    got = run_decoder(dec, x, levels, go)
    l2 = lambda a, w: float((a.double().cpu() - w).norm() / w.norm().clamp_min(1e-30))  # noqa: E731
    hip = {k: l2(got[k], w) for k, w in ref["f64"].items()}
    ac = {k: l2(ref["ac"][k], w) for k, w in ref["f64"].items()}
    med = lambda d: sorted(d.values())[len(d) // 2]  # noqa: E731
    wh, wa = max(hip, key=hip.get), max(ac, key=ac.get)
    print(f"vqdec fast bf16 rel L2 vs f64: HIP median {med(hip):.3g} worst {hip[wh]:.3g} ({wh}); "
          f"torch autocast median {med(ac):.3g} worst {ac[wa]:.3g} ({wa})")
    ratio = {k: hip[k] / ac[k] for k in hip}
    wr = max(ratio, key=ratio.get)
    print(f"vqdec fast bf16: worst HIP / autocast error ratio {ratio[wr]:.3f} ({wr})")
    assert all(np.isfinite(v) for v in hip.values())
    assert all(hip[k] <= 1.25 * ac[k] for k in hip), {k: (hip[k], ac[k]) for k in hip if hip[k] > 1.25 * ac[k]}
