"""vqx_vq_forward's "exact first-min argmin" on inputs where the rule decides
the answer: planted identical codebook rows, an integer grid on which float32
and float64 distances coincide and ties arise by themselves, the modules above
the kernel with a duplicated codebook, and frames that are not finite.

Every expected index is the first-minimum rule's own (tests/vq_tie_cases.py:
the lowest index among the codes at the float64 minimum), whose preconditions
tests/test_vq_ties_host.py proves on the CPU.  No tolerance anywhere: indices,
gathered rows, counts and sums are compared bit for bit.
"""
from types import SimpleNamespace

import pytest
import torch

from tests import vq_tie_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vae_npvc_amd import ops
    return ops


def run_full(z, E, bsum0=None, bcnt0=None):
    """The full call: zq, zq_c in bf16, sqerr and the EMA statistics (accumulated onto bsum0 / bcnt0)."""
    ops = _ops()
    N, D = z.shape
    K = E.shape[0]
    zd, Ed = z.to(DEV), E.to(DEV)
    idx = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    zq = torch.full((N, D), float("nan"), device=DEV)
    zqc = torch.full((N, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    sq = torch.full((1,), float("nan"), device=DEV)
    bsum = torch.zeros(K, D, device=DEV) if bsum0 is None else bsum0.to(DEV)
    bcnt = torch.zeros(K, device=DEV) if bcnt0 is None else bcnt0.to(DEV)
    ops.vq_forward(zd, Ed, idx, zq, zqc, sq, None, bsum, bcnt)
    torch.cuda.synchronize()
    return SimpleNamespace(idx=idx.cpu(), zq=zq.cpu(), zqc=zqc.cpu(), sq=sq.cpu(), bsum=bsum.cpu(), bcnt=bcnt.cpu())


def run_index_only(z, E):
    """The form the `encode` paths use."""
    idx = torch.full((z.shape[0],), -1, dtype=torch.int64, device=DEV)
    _ops().vq_forward(z.to(DEV), E.to(DEV), idx, None, None, None)
    torch.cuda.synchronize()
    return idx.cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- A1
@pytest.mark.parametrize("D", C.DIMS)
@pytest.mark.parametrize("name", list(C.PLANTED))
def test_planted_twins_go_to_the_lower_index(name, D):
    """Identical codebook rows a < b (< c), frames near them: every frame gets a, in the full call and in the
    index-only call, whichever stage of the argmin meets the tie (in-lane '<' over the steps, shuffle merge, LDS
    merge over the code splits), in full and in partial workgroups; z_q is row a's bits; the higher twins count
    no frame."""
    c = C.planted(name, D)
    r = run_full(c.z, c.E)
    wrong = (r.idx != c.expect).nonzero().flatten().tolist()
    assert not wrong, (name, D, [(n, int(r.idx[n]), int(c.expect[n])) for n in wrong[:8]])
    assert torch.equal(run_index_only(c.z, c.E), c.expect)
    assert same_bits(r.zq, c.E[c.expect])
    assert torch.equal(r.zqc, c.E[c.expect].to(torch.bfloat16))
    for g in c.groups:
        assert float(r.bcnt[g[0]]) == c.per, g
        assert not bool(r.bcnt[list(g[1:])].any()), g
    assert float(r.bcnt.sum()) == c.N


# ---- A2
@pytest.mark.parametrize("D", C.DIMS)
@pytest.mark.parametrize("K", C.GRID_K)
def test_integer_grid_matches_the_float64_first_minimum_exactly(K, D):
    """z and E from {-1, 0, 1}: every product, norm and partial sum is a small integer, so the kernel's float32
    distance IS the float64 one in any summation order; ties between different codes arise by themselves (26 to
    131 of 777 frames) and a strictly nearer higher-indexed code must still win.  Indices, z_q, z_q in bf16,
    counts, per-code sums (accumulated onto integer-valued buffers) and the squared error are exact
    (vqx_vq_forward sums the squared error unscaled, and every partial sum is an integer below 2^24)."""
    ops = _ops()
    c = C.grid(K, D)
    gen = torch.Generator().manual_seed(K + D)
    bsum0 = torch.randint(-9, 10, (K, D), generator=gen).float()
    bsum0[bsum0 == 0] = 3.0
    bcnt0 = torch.randint(1, 10, (K,), generator=gen).float()
    want_c = torch.bincount(c.expect, minlength=K).double()
    want_s = torch.zeros(K, D, dtype=torch.float64).index_add_(0, c.expect, c.z.double())
    want_sq = (c.E[c.expect].double() - c.z.double()).pow(2).sum()
    assert float(want_sq) < 2 ** 24

    r = run_full(c.z, c.E, bsum0, bcnt0)
    wrong = (r.idx != c.expect).nonzero().flatten().tolist()
    assert not wrong, (K, D, len(wrong), [(n, int(r.idx[n]), int(c.expect[n])) for n in wrong[:8]])
    assert torch.equal(run_index_only(c.z, c.E), c.expect)
    assert same_bits(r.zq, c.E[c.expect])
    assert torch.equal(r.zqc, c.E[c.expect].to(torch.bfloat16)) and torch.equal(r.zqc.float(), c.E[c.expect])
    assert torch.equal(r.bcnt.double(), bcnt0.double() + want_c)
    assert torch.equal(r.bsum.double(), bsum0.double() + want_s)
    assert float(r.sq[0]) == float(want_sq), (float(r.sq[0]), float(want_sq))

    # vqx_vq_stats alone on the expected indices: the same counts and sums
    part = torch.empty(ops.vq_workspace(c.N, K, True, D), device=DEV)
    bsum, bcnt = bsum0.to(DEV), bcnt0.to(DEV)
    ops.vq_stats(c.z.to(DEV), c.expect.to(DEV), K, part, bsum, bcnt)
    torch.cuda.synchronize()
    assert same_bits(bcnt.cpu(), r.bcnt) and same_bits(bsum.cpu(), r.bsum)


# ---- A3
def _frames(B, D, T, seed):
    return torch.randn(B, D, T, generator=torch.Generator().manual_seed(seed))


def test_flat_model_encode_never_returns_the_upper_twin():
    """vqvae.Model.encode (vcc20: K = 512, D = 128), alone and on a two-utterance padded batch, with the codebook
    buffer's upper half a copy of its lower half: no index at or above K / 2."""
    from tests import flat_ragged_ref as R
    cfg, sd, xs, _ = R.draw("vcc20", R.SEED["vcc20"])
    m = R.model(SimpleNamespace(cfg=cfg, sd=sd))
    K = m.quantizer.embeddings.shape[0]
    with torch.no_grad():
        m.quantizer.embeddings[K // 2:] = m.quantizer.embeddings[:K // 2]
    assert torch.equal(m.quantizer.embeddings[K // 2:], m.quantizer.embeddings[:K // 2])
    a, b = xs[1], xs[5]  # 70 and 33 frames
    alone = m.encode(a.unsqueeze(0).cuda()).cpu()
    assert tuple(alone.shape) == (1, 70) and int(alone.min()) >= 0 and int(alone.max()) < K // 2
    assert alone.unique().numel() > 1
    x = torch.zeros(2, a.shape[0], 70)
    x[0], x[1, :, :33] = a, b
    both = m.encode(x.cuda(), lengths=[70, 33]).cpu()
    assert tuple(both.shape) == (2, 70) and int(both.min()) >= 0 and int(both.max()) < K // 2
    assert torch.equal(both[0:1], alone) and not bool(both[1, 33:].any())


def test_ema_quantizer_eval_never_returns_the_upper_twin():
    from vae_npvc_amd.model.layers_vq import EMAVectorQuantizer
    K, D, B, T = 16, 64, 2, 37
    q = EMAVectorQuantizer(K, D, 0.9).cuda()
    E = C.duplicated_halves(K, D, 11)
    with torch.no_grad():
        q.embeddings.copy_(E)
    q.mark_initialized()
    q.eval()
    z = _frames(B, D, T, 12)
    z_vq = q(z.cuda())[0].cpu()
    idx = q.last_indices.cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < K // 2
    assert torch.equal(q.encode(z.cuda()).cpu(), idx)
    assert same_bits(z_vq.transpose(1, 2).reshape(-1, D), E[idx.reshape(-1)])


@pytest.mark.parametrize("normalize", [False, True])
def test_plain_quantizer_never_returns_the_upper_twin(normalize):
    """VectorQuantizer.encode and .forward_indices with duplicated parameter rows; with `normalize` the rows the
    kernel sees are the normalised ones, checked to be identical bit for bit before the indices are."""
    from vae_npvc_amd.model.layers_vq import VectorQuantizer
    K, D, B, T = 16, 64, 2, 37
    q = VectorQuantizer(K, D, normalize=normalize).cuda()
    with torch.no_grad():
        q.embeddings.copy_(C.duplicated_halves(K, D, 21, scale=1.7))
    emb = q._codebook()
    torch.cuda.synchronize()
    assert same_bits(emb[K // 2:].cpu(), emb[:K // 2].cpu())
    if normalize:
        assert not torch.equal(emb.cpu(), q.embeddings.detach().cpu())
    z = _frames(B, D, T, 22).cuda()
    for idx in (q.encode(z).cpu(), q.forward_indices(z).cpu()):
        assert tuple(idx.shape) == (B, T) and int(idx.min()) >= 0 and int(idx.max()) < K // 2
        assert idx.unique().numel() > 1
    assert same_bits(q.embeddings[K // 2:].detach().cpu(), q.embeddings[:K // 2].detach().cpu())


# ---- A4
def test_nonfinite_frames_get_an_index_in_range_and_touch_no_other_frame():
    """Frames with NaN, +inf or an overflowing norm among finite ones (N = 70, K = 128, D = 128; two of the four
    in the last, partial workgroup).

    Where the index is guarded (vq_forward_kernel, vqx_vq.hip): a lane's candidate starts as (+inf, 0x7fffffff)
    and is replaced only where `d < best_d` holds, which no NaN or +inf distance satisfies; the shuffle merge and
    the LDS merge over the code splits only choose between such candidates; the epilogue then reads
    `my_idx = (bi >= K || bi < 0) ? 0 : bi` before the one place an address is formed from the index, the gather
    `E + my_idx * D`, and before the index is stored.  vq_stats_kernel reads the stored indices and drops any
    code outside [0, K) on its own.  No unguarded path was found.

    A frame holding a NaN gets 0, which is also torch.argmin's answer on a row of NaN distances.  The +inf and
    3e38 frames have distances that are +inf or NaN code by code: torch.argmin picks the first NaN, the kernel
    picks 0 (no distance compares below +inf); that difference is left unpinned, and only the range and
    z_q = E[idx] are required there.  A finite frame sharing a 16-frame MFMA tile with a poisoned one keeps the
    index and z_q bits of a run in which the poisoned frames are zeros."""
    c = C.nonfinite()
    r = run_full(c.z, c.E)
    assert int(r.idx.min()) >= 0 and int(r.idx.max()) < c.K
    assert int(r.idx[c.nan_elem]) == 0 and int(r.idx[c.nan_row]) == 0
    for row in (c.nan_elem, c.nan_row, c.inf_elem, c.big_elem):
        assert same_bits(r.zq[row], c.E[r.idx[row]]), row
    assert torch.equal(run_index_only(c.z, c.E), r.idx)
    assert torch.equal(r.bcnt, torch.bincount(r.idx, minlength=c.K).float())
    clean = run_full(c.clean, c.E)
    want = C.first_min(C.distances(c.clean.double(), c.E.double()))
    assert torch.equal(clean.idx[c.finite], want[c.finite])
    assert torch.equal(r.idx[c.finite], clean.idx[c.finite])
    assert same_bits(r.zq[c.finite], clean.zq[c.finite])
    assert torch.equal(r.zqc[c.finite], clean.zqc[c.finite])
