"""The length-aware kernels (vae_npvc_amd/csrc/vqx_varlen.hip) on the MI355X,
each against its torch expression in fp32 and bf16: a padded batch [B*T][ld]
in which utterance b owns rows t < len[b].  Pad rows of every input hold NaN:
a kernel that read one would show it.  One case of every kernel holds more
utterances than a launch's by-value table (896; 96 for the concatenation)."""
import numpy as np
import pytest
import torch

from tests.hier_ref import stretch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
# B, T, lengths: 1 and T among them, the longest not last; then more utterances than one launch's table
SMALL = (5, 37, [37, 1, 8, 23, 36])
MANY = (900, 9, [1 + (7 * b) % 9 for b in range(900)])


def _ops():
    from vae_npvc_amd import ops
    return ops


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def padded(B, T, C, lens, dtype, gen, ld=None, scale=1.5, shift=0.3):
    """[B*T, ld] rows: N(shift, scale) in the valid rows, NaN in the pad rows and the pad columns."""
    ld = ld or C
    x = torch.full((B, T, ld), float("nan"))
    for b, n in enumerate(lens):
        x[b, :n, :C] = torch.randn(n, C, generator=gen) * scale + shift
    return x.view(B * T, ld).to(dtype).to(DEV)


def guarded(rows, cols, dtype, fill=float("nan")):
    """(whole, view): `rows` rows between 3 sentinel rows in front and behind, holding `fill`."""
    whole = torch.full((rows + 6, cols), fill, device=DEV, dtype=dtype)
    return whole, whole[3:3 + rows]


def guards_intact(whole, fill_is_nan=True):
    g = torch.cat([whole[:3], whole[-3:]])
    return bool(torch.isnan(g).all()) if fill_is_nan else bool((g == 7.0).all())


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,C,ld", [(1, 96, 96), (2, 64, 80)])
@pytest.mark.parametrize("shape", [SMALL, MANY], ids=["small", "many"])
def test_groupnorm_stats_len_against_float64(dtype, G, C, ld, shape):
    """mean and 1/sqrt(var + eps) over (C/G, t < len[b]) against float64 of the same (rounded) input, under
    the bound tests/test_gpu_kernels.py::test_gnstats_epilogue_matches_standalone holds the statistics
    kernel to: relative 1e-5 (fp32) / 5e-3 (bf16) over the tensor."""
    ops = _ops()
    B, T, lens = shape
    gen = torch.Generator().manual_seed(410 + C)
    x = padded(B, T, C, lens, dtype, gen, ld)
    mr = torch.full((B, G, 2), float("nan"), device=DEV)
    ops.groupnorm_stats_len(x[:, :C], T, G, lens, torch.empty(B * G * 24, device=DEV), mr)
    xx = x.view(B, T, ld)[:, :, :C].double().cpu()
    mean, rstd = torch.empty(B, G), torch.empty(B, G)
    for b, n in enumerate(lens):
        v = xx[b, :n].reshape(n, G, C // G)
        mean[b] = v.mean(dim=(0, 2))
        rstd[b] = 1.0 / torch.sqrt(v.var(dim=(0, 2), unbiased=False) + 1e-5)
    tol = 1e-5 if dtype == torch.float32 else 5e-3
    em, er = relerr(mr[..., 0], mean), relerr(mr[..., 1], rstd)
    print(f"groupnorm_stats_len {dtype} G={G} B={B}: mean {em:.3g} rstd {er:.3g} (tol {tol:g})")
    assert em < tol and er < tol
    again = torch.empty_like(mr)
    ops.groupnorm_stats_len(x[:, :C], T, G, lens, torch.empty(B * G * 24, device=DEV), again)
    assert torch.equal(again, mr)  # fixed summation order


# ------------------------------------------------------------------ applies and mask
def _apply_case(dtype, glu, C, ld, shape, seed):
    ops = _ops()
    B, T, lens = shape
    gen = torch.Generator().manual_seed(seed)
    G, cout = (2, C // 2) if glu else (1, C)
    h = padded(B, T, C, lens, dtype, gen, ld)[:, :C]
    gamma = (torch.randn(C, generator=gen) * 0.5 + 1.0).to(DEV)
    beta = (torch.randn(C, generator=gen) * 0.5).to(DEV)
    mr = torch.empty(B, G, 2, device=DEV)
    ops.groupnorm_stats_len(h, T, G, lens, torch.empty(B * G * 24, device=DEV), mr)
    whole, out = guarded(B * T, ld, dtype)
    if glu:
        ops.gn_glu_fwd_len(h, out[:, :cout], T, lens, mr, gamma, beta)
    else:
        ops.gn_lrelu_fwd_len(h, out[:, :cout], T, lens, mr, gamma, beta)
    # the existing kernel on the same rows with the same statistics: pad rows of its input zeroed (it reads them)
    h0 = torch.nan_to_num(h, nan=0.0).contiguous()
    want = torch.empty(B * T, cout, device=DEV, dtype=dtype)
    if glu:
        ops.gn_glu_fwd(h0, want, T, mr, gamma, beta)
    else:
        ops.gn_lrelu_fwd(h0, want, T, mr, gamma, beta)
    got, want = out[:, :cout].view(B, T, cout), want.view(B, T, cout)
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n], want[b, :n]), b  # bit-equal on the valid rows
        assert bool((got[b, n:] == 0).all()), b          # exact zeros in the tail
    assert bool(torch.isfinite(got).all())
    assert bool(torch.isnan(out[:, cout:]).all()) and guards_intact(whole)  # pad columns and neighbours untouched


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,ld", [(96, 96), (32, 48)])
@pytest.mark.parametrize("shape", [SMALL, MANY], ids=["small", "many"])
def test_gn_lrelu_fwd_len_is_the_plain_kernel_on_the_valid_rows(dtype, C, ld, shape):
    _apply_case(dtype, False, C, ld, shape, 500 + C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,ld", [(64, 64), (256, 272)])
@pytest.mark.parametrize("shape", [SMALL, MANY], ids=["small", "many"])
def test_gn_glu_fwd_len_is_the_plain_kernel_on_the_valid_rows(dtype, C, ld, shape):
    _apply_case(dtype, True, C, ld, shape, 600 + C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,ld", [(24, 24), (64, 80)])
@pytest.mark.parametrize("shape", [SMALL, MANY, (3, 12, [12, 12, 12])], ids=["small", "many", "no_tail"])
def test_mask_tail_zeroes_the_tails_alone(dtype, C, ld, shape):
    ops = _ops()
    B, T, lens = shape
    whole, x = guarded(B * T, ld, dtype, fill=7.0)
    gen = torch.Generator(device=DEV).manual_seed(7)
    x[:, :C] = torch.randn(B * T, C, device=DEV, generator=gen).to(dtype)
    for b, n in enumerate(lens):  # whatever a GEMM epilogue may have left in a tail: NaN and huge values
        x.view(B, T, ld)[b, n:, :C:2] = float("nan")
        x.view(B, T, ld)[b, n:, 1:C:2] = 1e30
    before = whole.clone()
    ops.mask_tail(x[:, :C], T, lens)
    got, was = x.view(B, T, ld), before[3:3 + B * T].view(B, T, ld)
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n], was[b, :n]), b
        assert bool((got[b, n:, :C] == 0).all()), b
    assert torch.equal(got[:, :, C:], was[:, :, C:]) and guards_intact(whole, fill_is_nan=False)


# ------------------------------------------------------------------ concatenation
def _cat_reference(levels, lens, level_lens, T, ldo, out_dtype):
    """Per utterance: cat([stretch(level[b, :m], n_b)]) in the valid rows, zeros below; NaN where nothing is written."""
    B = len(lens)
    total = sum(z.shape[2] for z in levels)
    want = torch.full((B, T, ldo), float("nan"))
    for b, n in enumerate(lens):
        parts = [stretch(z[b:b + 1, :m[b]].transpose(1, 2), n)[0].t() for z, m in zip(levels, level_lens)]
        want[b, :n, :total] = torch.cat(parts, dim=1)
        want[b, n:, :total] = 0
    return want.view(B * T, ldo).to(out_dtype)


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("D", [64, 320])
def test_codes_upsample_cat_len_is_the_per_utterance_stretch(out_dtype, normalize, D):
    """A dense one-frame level (the style), an indexed level with a replicate tail for some utterances and none
    for others (n_b // m exact: 32 / 16, 24 / 24; tails: 37 / 9, 23 / 5), an indexed level with m = 1, and a
    dense multi-frame level; ldo wider than the sum; every index entry at t >= m out of range."""
    ops = _ops()
    gen = torch.Generator().manual_seed(700 + D)
    T, lens = 37, [32, 37, 24, 23, 1]
    B, K = len(lens), 16
    m1, m2, m3 = [16, 9, 24, 5, 1], [1, 1, 1, 1, 1], [8, 37, 3, 23, 1]
    T1, T2, T3 = 24, 2, 37  # the levels' own padded lengths
    style = torch.randn(B, 1, 32, generator=gen)
    E1, E2 = torch.randn(K, D, generator=gen) * 2.0, torch.randn(K, 64, generator=gen) * 0.5
    dense = torch.full((B, T3, 8), float("nan"))
    idx1, idx2 = torch.full((B, T1), 1 << 40), torch.full((B, T2), -5)  # never read beyond m
    for b in range(B):
        idx1[b, :m1[b]] = torch.randint(0, K, (m1[b],), generator=gen)
        idx2[b, :m2[b]] = torch.randint(0, K, (m2[b],), generator=gen)
        dense[b, :m3[b]] = torch.randn(m3[b], 8, generator=gen)
    total = 32 + D + 64 + 8
    ldo = total + 8
    whole, out = guarded(B * T, ldo, out_dtype)
    levels = [style.view(B, 32).to(DEV), (idx1.to(DEV), E1.to(DEV), normalize), (idx2.to(DEV), E2.to(DEV), normalize),
              dense.view(B * T3, 8).to(DEV)]
    ops.codes_upsample_cat_len(levels, B, T, lens, [[1] * B, m1, m2, m3], out)
    # a normalised row as the plain kernel writes it (E[k] / sqrt(sum E[k]^2) in its summation order): one row a code
    def rows(E):
        if not normalize:
            return E
        every = torch.arange(K, device=DEV).view(1, K)
        return ops.codes_upsample_cat([(every, E.to(DEV), True)], 1, K, torch.empty(K, E.shape[1], device=DEV)).cpu()
    z1, z2 = rows(E1)[idx1.clamp(0, K - 1)], rows(E2)[idx2.clamp(0, K - 1)]
    want = _cat_reference([style, z1, z2, torch.nan_to_num(dense)], lens, [[1] * B, m1, m2, m3], T, ldo, out_dtype)
    assert torch.equal(torch.nan_to_num(out.cpu().float(), nan=-77.0), torch.nan_to_num(want.float(), nan=-77.0))
    assert guards_intact(whole)


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_codes_upsample_cat_len_more_utterances_than_a_launch(out_dtype):
    """200 utterances (96 a launch): dense-only and indexed levels, equal to the plain kernel per utterance."""
    ops = _ops()
    gen = torch.Generator().manual_seed(71)
    B, T, K, D = 200, 12, 16, 64
    lens = [1 + (5 * b) % 12 for b in range(B)]
    m = [1 + (b % n) for b, n in enumerate(lens)]
    E = torch.randn(K, D, generator=gen).to(DEV)
    idx = torch.randint(0, K, (B, T), generator=gen).to(DEV)
    dense = torch.randn(B * T, 8, generator=gen).to(DEV)
    out = torch.full((B * T, D + 8), float("nan"), device=DEV, dtype=out_dtype)
    ops.codes_upsample_cat_len([(idx, E, True), dense], B, T, lens, [m, m], out)
    got = out.view(B, T, D + 8)
    for b in (0, 1, 95, 96, 97, 191, 192, 199):  # both sides of every launch boundary
        n, mb = lens[b], m[b]
        one = torch.empty(n, D + 8, device=DEV, dtype=out_dtype)
        ops.codes_upsample_cat([(idx[b:b + 1, :mb].contiguous().clone(), E, True),
                                dense.view(B, T, 8)[b, :mb].contiguous()], 1, n, one)
        assert torch.equal(got[b, :n], one), b
        assert bool((got[b, n:] == 0).all()), b
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ segment mean
@pytest.mark.parametrize("C,ld", [(64, 64), (100, 112)])
@pytest.mark.parametrize("shape", [SMALL, MANY], ids=["small", "many"])
def test_segment_mean_against_float64(C, ld, shape):
    """f32 sums of at most T = 37 terms in a fixed order, one division: within 37 * 2^-24 of the float64 mean,
    relative to the mean of the absolute values (the bound of a recursive sum of n terms, n * u * sum|x|)."""
    ops = _ops()
    B, T, lens = shape
    gen = torch.Generator().manual_seed(800 + C)
    z = padded(B, T, C, lens, torch.float32, gen, ld)
    whole, out = guarded(B, ld, torch.float32)
    ops.segment_mean(z[:, :C], T, lens, out[:, :C])
    zz = z.view(B, T, ld)[:, :, :C].double().cpu()
    want = torch.stack([zz[b, :n].mean(0) for b, n in enumerate(lens)])
    scale = torch.stack([zz[b, :n].abs().mean(0) for b, n in enumerate(lens)])
    err = float(((out[:, :C].double().cpu() - want).abs() / scale).max())
    print(f"segment_mean C={C} B={B}: err {err:.3g} bound {(T + 1) * 2.0 ** -24:.3g}")
    assert err <= (T + 1) * 2.0 ** -24
    assert bool(torch.isnan(out[:, C:]).all()) and guards_intact(whole)
    again = torch.empty(B, C, device=DEV)
    ops.segment_mean(z[:, :C], T, lens, again)
    assert torch.equal(again, out[:, :C])


def test_a_refused_call_writes_nothing():
    """A length outside 1..T fails on the host: VqxError naming the item, the output untouched."""
    ops = _ops()
    x = torch.randn(3 * 10, 16, device=DEV)
    before = x.clone()
    with pytest.raises(ops.L.VqxError, match="item 2: len 11"):
        ops.mask_tail(x, 10, [10, 4, 11])
    with pytest.raises(ops.L.VqxError, match="item 0: len 0"):
        ops.mask_tail(x, 10, [0, 4, 10])
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    with pytest.raises(ValueError, match="host values"):
        ops.mask_tail(x, 10, torch.tensor([10, 4, 9], device=DEV))  # lengths never come from the device
    assert np.isfinite(float(x.sum()))
