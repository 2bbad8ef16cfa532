"""vqx_codes_upsample_cat on the MI355X (include/vqx.h): the first decoder's
frame-major input straight from codes.

  * dense and un-normalised indexed levels against index_select plus the
    reference's repeat / replicate stretch written in torch, bit for bit;
  * normalised levels against E64 / ||E64|| in float64, within
    max(8 * err32, 16 * 2^-23) of the largest value, err32 the error of torch's
    own fp32 E / E.norm(dim=1, keepdim=True) on the same codebook;
  * bf16 output == the f32 output .to(bfloat16), bit for bit;
  * padding columns and the codebook are left alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP16 = 16 * 2.0 ** -23


def _ops():
    from vae_npvc_amd import ops
    return ops


def stretch(rows, B, T):
    """Model.upsample (vqvae2.py:130-143) on frame-major rows [B*T_l, C]: every frame repeated
    T // T_l times, the tail replicate-padded from the last frame."""
    z = rows.view(B, -1, rows.shape[1])
    T_l = z.shape[1]
    z = z.repeat_interleave(T // T_l, dim=1)
    if z.shape[1] < T:
        z = torch.cat([z, z[:, -1:].expand(-1, T - z.shape[1], -1)], dim=1)
    return z.reshape(B * T, -1)


# B, T, levels: ("dense", C, T_l) | ("idx", K, D, T_l); extra = ldo - sum C_l
CASES = {
    "dense+padded_tail": (2, 5, [("dense", 4, 1), ("idx", 3, 4, 2)], 0),
    "T70": (1, 70, [("idx", 16, 64, 17), ("idx", 16, 64, 70)], 0),
    "D256": (3, 8, [("idx", 7, 256, 2)], 0),
    "ldo_padding": (2, 5, [("idx", 3, 4, 2), ("dense", 8, 5), ("idx", 5, 132, 1)], 12),
    # more than 64 granules in a level: a lane's second round, in the sum of squares and in the copy
    "D320": (2, 7, [("idx", 5, 320, 3), ("dense", 260, 2)], 4),
}


def build(case, normalize):
    B, T, spec, extra = CASES[case]
    gen = torch.Generator(device=DEV).manual_seed(len(case))
    levels, want = [], []
    for lv in spec:
        if lv[0] == "dense":
            _, C, T_l = lv
            z = torch.randn(B * T_l, C, device=DEV, generator=gen)
            levels.append(z)
            want.append(("dense", z))
        else:
            _, K, D, T_l = lv
            # rows of different lengths, so that normalising changes every one of them
            E = torch.randn(K, D, device=DEV, generator=gen) * torch.linspace(0.25, 3.0, K, device=DEV).view(-1, 1)
            idx = torch.randint(0, K, (B, T_l), device=DEV, generator=gen)
            idx.view(-1)[0], idx.view(-1)[-1] = K - 1, 0  # both ends of the codebook
            levels.append((idx, E, normalize))
            want.append(("idx", idx, E))
    return B, T, levels, want, extra


def run(ops, B, T, levels, extra, dtype=torch.float32):
    width = sum(lv.shape[1] if torch.is_tensor(lv) else lv[1].shape[1] for lv in levels)
    out = torch.full((B * T, width + extra), float("nan"), device=DEV, dtype=dtype)
    ops.codes_upsample_cat(levels, B, T, out)
    return out, width


@pytest.mark.parametrize("case", CASES)
def test_plain_levels_equal_index_select_and_stretch_bit_for_bit(case):
    ops = _ops()
    B, T, levels, want, extra = build(case, normalize=False)
    books = [lv[1].clone() for lv in levels if not torch.is_tensor(lv)]
    out, width = run(ops, B, T, levels, extra)
    ref = torch.cat([stretch(w[1] if w[0] == "dense" else w[2].index_select(0, w[1].reshape(-1)), B, T)
                     for w in want], dim=1)
    assert torch.equal(out[:, :width], ref)
    assert bool(torch.isnan(out[:, width:]).all())  # columns from sum C_l up are not written
    out16, _ = run(ops, B, T, levels, extra, torch.bfloat16)
    assert torch.equal(out16[:, :width], out[:, :width].to(torch.bfloat16))
    assert bool(torch.isnan(out16[:, width:]).all())
    assert all(torch.equal(a, lv[1]) for a, lv in zip(books, [lv for lv in levels if not torch.is_tensor(lv)]))


@pytest.mark.parametrize("case", CASES)
def test_normalised_levels_match_float64_rows_over_their_norm(case):
    ops = _ops()
    B, T, levels, want, extra = build(case, normalize=True)
    books = [lv[1].clone() for lv in levels if not torch.is_tensor(lv)]
    out, width = run(ops, B, T, levels, extra)
    col = 0
    for w in want:
        if w[0] == "dense":  # exactly the copy of vqx_upsample_cat_fwd
            C = w[1].shape[1]
            assert torch.equal(out[:, col:col + C], stretch(w[1], B, T))
            col += C
            continue
        _, idx, E = w
        D = E.shape[1]
        E64 = E.double()
        n64 = E64 / E64.norm(dim=1, keepdim=True)
        err32 = float(((E / E.norm(dim=1, keepdim=True)).double() - n64).abs().max() / n64.abs().max())
        ref = stretch(n64.index_select(0, idx.reshape(-1)), B, T)
        err = float((out[:, col:col + D].double() - ref).abs().max() / ref.abs().max())
        bound = max(8 * err32, ULP16)
        print(f"codes_upsample_cat {case} D={D}: error {err:.3e}, torch fp32 {err32:.3e}, bound {bound:.3e}")
        assert err <= bound
        col += D
    assert col == width and bool(torch.isnan(out[:, width:]).all())
    out16, _ = run(ops, B, T, levels, extra, torch.bfloat16)
    assert torch.equal(out16[:, :width], out[:, :width].to(torch.bfloat16))  # the f32 value rounded once
    again, _ = run(ops, B, T, levels, extra)
    assert torch.equal(again[:, :width], out[:, :width])  # equal arguments, equal bits
    assert all(torch.equal(a, lv[1]) for a, lv in zip(books, [lv for lv in levels if not torch.is_tensor(lv)]))


def test_strided_operands_with_the_debug_extent_checks_on():
    """A codebook and a dense level that are column slices of wider buffers (ld > C) and an output that is
    a slice too, through the wrapper's extent checks."""
    ops = _ops()
    B, T = 2, 6
    gen = torch.Generator(device=DEV).manual_seed(5)
    wide_E = torch.randn(9, 24, device=DEV, generator=gen)
    wide_z = torch.randn(B * 3, 16, device=DEV, generator=gen)
    E, z = wide_E[:, 4:12], wide_z[:, 8:12]
    idx = torch.randint(0, 9, (B, 2), device=DEV, generator=gen)
    buf = torch.full((B * T, 20), float("nan"), device=DEV)
    prev = ops.set_debug_checks(True)
    try:
        ops.codes_upsample_cat([z, (idx, E, False)], B, T, buf[:, 4:16])
    finally:
        ops.set_debug_checks(prev)
    ref = torch.cat([stretch(z.contiguous(), B, T), stretch(E.index_select(0, idx.reshape(-1)), B, T)], dim=1)
    assert torch.equal(buf[:, 4:16], ref)
    assert bool(torch.isnan(buf[:, :4]).all()) and bool(torch.isnan(buf[:, 16:]).all())
