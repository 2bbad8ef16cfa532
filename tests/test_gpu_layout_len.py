"""vqx_nct_to_ntc_len / vqx_ntc_to_nct_len on the MI355X against the torch
expression they restate, exactly: both directions, fp32 and bf16, channel
counts off and on the 32-wide tile (24, 80, 160), frame counts 1, 33 and 130,
lengths on the tile edges (1, 32, 33, T), a row stride above C, T_out < T, NaN
in the part of the source that must not be read, and a batch of 900 utterances,
which crosses the 896-entry length table of one launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _lengths(B, T):
    """B lengths over the tile edges that fit T, T itself among them."""
    edges = [n for n in (1, 32, 33, 64, 65, T - 1, T) if 1 <= n <= T]
    return [edges[(2 * b + 1) % len(edges)] for b in range(B - 1)] + [T]


def _keep(lens, T):
    return torch.arange(T)[None, :] < torch.tensor(lens)[:, None]  # (B, T)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 33, 130])
@pytest.mark.parametrize("C", [24, 80, 160])
def test_nct_to_ntc_len_is_the_masked_transpose(C, T, dtype):
    from vae_npvc_amd import ops
    B, ld = 6, C + 8
    lens = _lengths(B, T)
    g = torch.Generator().manual_seed(C * 1000 + T)
    x = torch.randn(B, C, T, generator=g)
    keep = _keep(lens, T)
    want = torch.where(keep[:, :, None], x.transpose(1, 2), torch.zeros(())).to(DT[dtype])  # (B, T, C)
    x_bad = torch.where(keep[:, None, :], x, torch.full((), float("nan")))  # the padding is never read
    for src in (x, x_bad):
        y = torch.full((B * T, ld), 7.0, device="cuda", dtype=DT[dtype])
        out = ops.nct_to_ntc_len(src.cuda(), lens, y[:, :C])
        assert out.data_ptr() == y.data_ptr()
        got = y.cpu().view(B, T, ld)
        assert torch.equal(got[:, :, :C], want)
        assert bool((got[:, :, C:] == 7.0).all())  # nothing past the C columns is written


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 33, 130])
@pytest.mark.parametrize("C", [24, 80, 160])
def test_ntc_to_nct_len_is_the_masked_transpose(C, T, dtype):
    from vae_npvc_amd import ops
    B, ld = 6, C + 8
    lens = _lengths(B, T)
    g = torch.Generator().manual_seed(C * 1000 + T + 1)
    rows = torch.randn(B, T, ld, generator=g).to(DT[dtype])
    keep = _keep(lens, T)
    rows_bad = torch.where(keep[:, :, None], rows, torch.full((), float("nan"), dtype=DT[dtype]))
    for T_out in sorted({T, max(1, T - 1), max(1, T - 40)}):
        want = torch.where(keep[:, None, :T_out], rows[:, :T_out, :C].float().transpose(1, 2), torch.zeros(()))
        for src in (rows, rows_bad):
            y = src.reshape(B * T, ld).cuda()
            x = torch.full((B, C, T_out), 7.0, device="cuda")
            ops.ntc_to_nct_len(y[:, :C], T, lens, x)
            assert torch.equal(x.cpu(), want), (T_out, src is rows_bad)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_batch_beyond_one_launch_table(dtype):
    """B = 900 > 896 utterances: the second launch's pointers and table entries."""
    from vae_npvc_amd import ops
    B, C, T = 900, 8, 4
    lens = [1 + (b * 7) % T for b in range(B)]
    x = torch.randn(B, C, T, generator=torch.Generator().manual_seed(5))
    keep = _keep(lens, T)
    y = torch.full((B * T, C), 7.0, device="cuda", dtype=DT[dtype])
    ops.nct_to_ntc_len(x.cuda(), lens, y)
    want = torch.where(keep[:, :, None], x.transpose(1, 2), torch.zeros(())).to(DT[dtype])
    assert torch.equal(y.cpu().view(B, T, C), want)
    back = torch.full((B, C, 3), 7.0, device="cuda")
    ops.ntc_to_nct_len(y, T, lens, back)
    assert torch.equal(back.cpu(), want.float().transpose(1, 2)[:, :, :3])


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from vae_npvc_amd import ops
    x = torch.zeros(2, 8, 6, device="cuda")
    y = torch.zeros(12, 8, device="cuda")
    with pytest.raises(ops.L.VqxError, match="item 1: len 7 outside \\[1, T = 6\\]"):
        ops.nct_to_ntc_len(x, [6, 7], y)
    with pytest.raises(ValueError, match="3 entries for a batch of 2"):
        ops.nct_to_ntc_len(x, [6, 5, 4], y)
    with pytest.raises(ValueError, match="T_out"):
        ops.ntc_to_nct_len(y, 6, [6, 5], torch.zeros(2, 8, 7, device="cuda"))
    with pytest.raises(ops.L.VqxError, match="item 0: len 0"):
        ops.ntc_to_nct_len(y, 6, [0, 5], torch.zeros(2, 8, 6, device="cuda"))
