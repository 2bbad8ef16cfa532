"""The two launches of vqvae2a / vqvae2b's batched conversion on the MI355X
(-m gpu), against torch on the host, bit for bit:

  * vqx_nct_to_ntc_pad_len: y[b*T + t][c] = t < len[b] ? cvt(x[b][c][t]) : 0
    over t < T >= T_in, the source NaN from len[b] on (never loaded);
  * vqx_index_mask_len: out[b][t] = t < len[b] ? idx[b*T + t] : 0 over
    t < T_out <= T, sentinels beyond len (int64 min / max included);
  * their limits: -1 with the item named, nothing launched, the output unchanged.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _ops():
    from vae_npvc_amd import ops
    return ops


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


# (B, C, T_in, T, lens, ldy): partial tiles with ldy > C; full tiles, T == T_in; more utterances than a launch (896)
PAD_CASES = {
    "partial": (3, 5, 37, 40, [37, 1, 33], 8),
    "tiles": (2, 33, 64, 64, [64, 40], 33),
    "launches": (897, 1, 2, 3, [1 + b % 2 for b in range(897)], 1),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(PAD_CASES))
def test_nct_to_ntc_pad_len_bit_for_bit(case, dtype):
    ops = _ops()
    B, C, T_in, T, lens, ldy = PAD_CASES[case]
    gen = torch.Generator().manual_seed(len(case))
    x = torch.randn(B, C, T_in, generator=gen)
    want = torch.zeros(B, T, C, dtype=dtype)
    for b, n in enumerate(lens):
        want[b, :n] = x[b, :, :n].t().to(dtype)  # torch rounds to nearest even, as cvt does
        x[b, :, n:] = float("nan")               # never loaded
    buf = torch.full((B * T, ldy), -7.0, device=DEV, dtype=dtype)
    y = buf[:, :C]
    assert ops.nct_to_ntc_pad_len(x.to(DEV), T, lens, y) is y
    assert torch.equal(y.cpu().view(B, T, C), want)
    assert bool((buf[:, C:] == -7.0).all())  # nothing beside the C columns
    again = torch.full((B * T, ldy), 3.0, device=DEV, dtype=dtype)[:, :C]
    ops.nct_to_ntc_pad_len(x.to(DEV), T, torch.tensor(lens), again)
    assert torch.equal(again, y)


def test_nct_to_ntc_pad_len_is_nct_to_ntc_len_when_nothing_is_padded():
    ops = _ops()
    B, C, T, lens = 3, 40, 50, [50, 7, 33]
    x = torch.randn(B, C, T, generator=torch.Generator().manual_seed(5)).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        a = ops.nct_to_ntc_len(x, lens, torch.empty(B * T, C, device=DEV, dtype=dtype))
        b = ops.nct_to_ntc_pad_len(x, T, lens, torch.empty(B * T, C, device=DEV, dtype=dtype))
        assert torch.equal(a, b)


# (B, T, T_out, lens)
MASK_CASES = {"small": (3, 5, 4, [4, 1, 3]), "launches": (897, 2, 2, [1 + b % 2 for b in range(897)])}


@pytest.mark.parametrize("case", sorted(MASK_CASES))
def test_index_mask_len_bit_for_bit(case):
    ops = _ops()
    B, T, T_out, lens = MASK_CASES[case]
    gen = torch.Generator().manual_seed(11)
    idx = torch.randint(0, 512, (B, T), generator=gen)
    want = torch.zeros(B, T_out, dtype=torch.int64)
    sentinels = [I64_MIN, I64_MAX, -1, 1 << 40]
    for b, n in enumerate(lens):
        want[b, :n] = idx[b, :n]
        for t in range(n, T):
            idx[b, t] = sentinels[(b + t) % 4]  # never loaded
    idx[0, 0], want[0, 0] = I64_MAX, I64_MAX    # a valid entry keeps all 64 bits
    idx[B - 1, 0], want[B - 1, 0] = I64_MIN, I64_MIN
    out = torch.full((B, T_out), -7, dtype=torch.int64, device=DEV)
    assert ops.index_mask_len(idx.to(DEV), lens, out) is out
    assert torch.equal(out.cpu(), want)
    again = torch.full((B, T_out), 9, dtype=torch.int64, device=DEV)
    ops.index_mask_len(idx.to(DEV), torch.tensor(lens), again)
    assert torch.equal(again, out)


def test_limits_return_minus_one_and_launch_nothing():
    from vae_npvc_amd import _lib as L
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    B, C, T_in, T = 3, 8, 6, 8
    x = torch.randn(B, C, T_in, device=DEV)
    y = torch.full((B * T, C), -7.0, device=DEV)
    X, Y, F32, BF16 = x.data_ptr(), y.data_ptr(), L.VQX_F32, L.VQX_BF16
    good = i32(6, 1, 3)
    assert lib.vqx_nct_to_ntc_pad_len(X, B, C, T_in, T, good, Y, C, F32, s) == 0
    torch.cuda.synchronize()
    y.fill_(-7.0)
    bad = [(0, B, C, T_in, T, good, Y, C, F32), (X, B, C, T_in, T, good, 0, C, F32), (X, B, C, T_in, T, None, Y, C, F32),
           (X + 2, B, C, T_in, T, good, Y, C, F32), (X, B, C, T_in, T, good, Y + 2, C, F32),
           (X, B, C, T_in, T, good, Y + 1, C, BF16), (X, B, C, T_in, T_in - 1, good, Y, C, F32),
           (X, B, C, T_in, 0, good, Y, C, F32), (X, 0, C, T_in, T, good, Y, C, F32), (X, B, 0, T_in, T, good, Y, C, F32),
           (X, B, C, 0, T, good, Y, C, F32), (X, B, C, T_in, T, good, Y, C - 1, F32), (X, B, C, T_in, T, good, Y, C, 7)]
    for args in bad:
        assert lib.vqx_nct_to_ntc_pad_len(*args, s) == -1, args[1:5]
        assert b"vqx_nct_to_ntc_pad_len" in lib.vqx_last_error()
    for lens, msg in ((i32(6, 0, 3), b"item 1: len 0"), (i32(6, 1, 7), b"item 2: len 7"), (i32(-1, 1, 3), b"item 0: len -1")):
        assert lib.vqx_nct_to_ntc_pad_len(X, B, C, T_in, T, lens, Y, C, F32, s) == -1
        assert msg in lib.vqx_last_error(), lib.vqx_last_error()  # len is bounded by T_in, not by T
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())

    T, T_out = 5, 4
    idx = torch.randint(0, 16, (B, T), device=DEV)
    out = torch.full((B, T_out), -7, dtype=torch.int64, device=DEV)
    I, O = idx.data_ptr(), out.data_ptr()
    good = i32(4, 1, 3)
    assert lib.vqx_index_mask_len(I, B, T, good, O, T_out, s) == 0
    torch.cuda.synchronize()
    out.fill_(-7)
    bad = [(0, B, T, good, O, T_out), (I, B, T, good, 0, T_out), (I, B, T, None, O, T_out), (I + 4, B, T, good, O, T_out),
           (I, B, T, good, O + 4, T_out), (I, B, T, good, O, T + 1), (I, B, T, good, O, 0), (I, 0, T, good, O, T_out),
           (I, B, 0, good, O, T_out)]
    for args in bad:
        assert lib.vqx_index_mask_len(*args, s) == -1, args[1:]
        assert b"vqx_index_mask_len" in lib.vqx_last_error()
    for lens, msg in ((i32(4, 0, 3), b"item 1: len 0"), (i32(4, 1, 5), b"item 2: len 5")):
        assert lib.vqx_index_mask_len(I, B, T, lens, O, T_out, s) == -1
        assert msg in lib.vqx_last_error(), lib.vqx_last_error()  # len is bounded by T_out, not by T
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    ops = _ops()
    with pytest.raises(ops.L.VqxError, match="item 2: len 5"):
        ops.index_mask_len(idx, [4, 1, 5], out)
    with pytest.raises(ops.L.VqxError, match="item 1: len 7"):
        ops.nct_to_ntc_pad_len(x, 8, [6, 7, 3], y)
    with pytest.raises(ValueError, match="host values"):
        ops.index_mask_len(idx, torch.tensor([4, 1, 3], device=DEV), out)  # lengths never come from the device
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((y == -7.0).all())
