"""The three kernels of a quantizer level under autograd, bit for bit against
torch expressions: vqx_ntc_to_nct_gather (the output layout change with the
jitter gather folded in), vqx_nct_to_ntc_keep (the jitter's backward folded
into the layout change) and vqx_vq_commit_bwd_g (the EMA level's commitment
gradient with the upstream gradient read on the device).

Shapes: T = 2 (the shortest length a map can be drawn for), tile edges in
both axes (33 = 32 + 1, 31, 5), more than one tile in both axes, and a channel
count that is no multiple of 32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 64, 2), (3, 64, 5), (2, 128, 33), (2, 256, 64), (2, 80, 31)]
MAPS = ["identity", "null", "all_replaced", "drawn"]


def _ops():
    from vae_npvc_amd import ops
    return ops


def make_map(kind, T):
    """(host map or None for NULL, the map as index array)."""
    ident = np.arange(T, dtype=np.int32)
    if kind == "null":
        return None, ident
    if kind == "identity":
        return ident, ident
    if kind == "all_replaced":  # every frame shows a neighbour
        src = ident + np.where(ident % 2 == 0, 1, -1).astype(np.int32)
        src[T - 1] = T - 2 if src[T - 1] >= T else src[T - 1]
        assert (src != ident).all()
        return src, src
    from vae_npvc_amd.model.layers_vq import Jitter
    np.random.seed(100 + T)
    src = Jitter(0.5).train().draw(T)
    return src, src


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_layout_change_bit_for_bit(shape, kind, dtype):
    ops = _ops()
    B, C, T = shape
    gen = torch.Generator(device=DEV).manual_seed(21)
    wide = torch.randn(B * T, C + 8, device=DEV, generator=gen).to(dtype)
    y = wide[:, 4:4 + C] if shape == (2, 80, 31) else wide[:, :C].contiguous()  # strided rows in one shape
    host, idx = make_map(kind, T)
    src = None if host is None else torch.from_numpy(host).to(DEV)
    x = torch.full((B, C, T), float("nan"), device=DEV)
    ops.ntc_to_nct_gather(y, src, x)
    want = y.float().reshape(B, T, C)[:, torch.from_numpy(idx).long().to(DEV), :].permute(0, 2, 1)
    assert torch.equal(x, want)
    if kind == "null":  # the plain transposition's bits
        assert torch.equal(x, ops.ntc_to_nct(y, torch.empty_like(x)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_keep_layout_change_bit_for_bit(shape, kind, dtype):
    ops = _ops()
    B, C, T = shape
    gen = torch.Generator(device=DEV).manual_seed(22)
    g = torch.randn(B, C, T, device=DEV, generator=gen)
    host, idx = make_map(kind, T)
    src = None if host is None else torch.from_numpy(host).to(DEV)
    wide = torch.full((B * T, C + 8), float("nan"), device=DEV, dtype=dtype)
    y = wide[:, 4:4 + C] if shape == (2, 80, 31) else torch.full((B * T, C), float("nan"), device=DEV, dtype=dtype)
    ops.nct_to_ntc_keep(g, src, y)
    keep = torch.from_numpy(idx == np.arange(T)).to(DEV)
    want = torch.where(keep[None, :, None], g.permute(0, 2, 1), torch.zeros((), device=DEV)).reshape(B * T, C)
    assert torch.equal(y, want.to(dtype))  # rounded once
    if kind == "all_replaced":
        assert not bool(y.float().abs().sum())
    if shape == (2, 80, 31):  # nothing outside the C columns was written
        assert bool(torch.isnan(wide[:, :4].float()).all()) and bool(torch.isnan(wide[:, 4 + C:].float()).all())


@pytest.mark.parametrize("nct", [True, False])
@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_commit_gradient_bit_for_bit(shape, with_g, nct):
    ops = _ops()
    B, D, T = shape
    gen = torch.Generator(device=DEV).manual_seed(23)
    z = torch.randn(B * T, D, device=DEV, generator=gen)
    zq = torch.randn(B * T, D, device=DEV, generator=gen)
    g = torch.randn(1, device=DEV, generator=gen) if with_g else None
    s = 2.0 * 0.25 / (B * T)
    dz = torch.full((B, D, T) if nct else (B * T, D), float("nan"), device=DEV)
    ops.vq_commit_bwd_g(z, zq, B, T, s, g, dz)
    s32 = torch.tensor(s, dtype=torch.float32, device=DEV)
    want = (z - zq) * (s32 * g if with_g else s32)  # the product of the scalars first, in fp32
    if nct:
        want = want.reshape(B, T, D).permute(0, 2, 1)
    assert torch.equal(dz, want)


def test_bad_arguments_return_the_library_error_without_launching():
    from vae_npvc_amd import _lib as L
    ops = _ops()
    t = torch.zeros(8, 4, device=DEV)
    x = torch.zeros(1, 4, 8, device=DEV)
    p, F32 = L.ptr, L.VQX_F32
    torch.cuda.synchronize()
    for name, args in (
            ("vqx_ntc_to_nct_gather", (0, 4, F32, 1, 4, 8, 0, p(x))),
            ("vqx_ntc_to_nct_gather", (p(t), 4, F32, 1, 4, 0, 0, p(x))),
            ("vqx_ntc_to_nct_gather", (p(t), 4, F32, 1, 0, 8, 0, p(x))),
            ("vqx_ntc_to_nct_gather", (p(t), 1 << 20, F32, 2, 1 << 20, 1 << 10, 0, p(x))),
            ("vqx_nct_to_ntc_keep", (p(x), 1, 4, 8, 0, 0, 4, F32)),
            ("vqx_nct_to_ntc_keep", (p(x), 1, 4, 0, 0, p(t), 4, F32)),
            ("vqx_nct_to_ntc_keep", (p(x), 2, 1 << 20, 1 << 10, 0, p(t), 1 << 20, F32)),
            ("vqx_vq_commit_bwd_g", (p(t), 0, 1, 4, 8, 1.0, 0, 1, p(x))),
            ("vqx_vq_commit_bwd_g", (p(t), p(t), 1, 0, 8, 1.0, 0, 1, p(x))),
            ("vqx_vq_commit_bwd_g", (p(t), p(t), 1, 4, 0, 1.0, 0, 0, p(x))),
            ("vqx_vq_commit_bwd_g", (p(t), p(t), 2, 1 << 20, 1 << 10, 1.0, 0, 0, p(x)))):
        with pytest.raises(L.VqxError, match=name):
            L.call(name, *args, L.stream_ptr())
    with pytest.raises(ValueError, match="src_t"):
        ops.ntc_to_nct_gather(t, torch.zeros(8, dtype=torch.int64, device=DEV), x)
    with pytest.raises(ValueError, match="src_t"):
        ops.nct_to_ntc_keep(x, torch.zeros(7, dtype=torch.int32, device=DEV), t)
    torch.cuda.synchronize()
    assert not bool(t.abs().sum()) and not bool(x.abs().sum())  # nothing was written
