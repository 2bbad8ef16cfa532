"""Kernel-level tests of the straight-through quantizer (csrc/vqx_vq.hip:
vqx_vq_normalize, vqx_vq_perplexity, vqx_vq_plain_bwd, vqx_vq_plain_bwd_g)
against one float64 restatement of VectorQuantizer.forward
(OracleVQVAE.quantize_plain's autograd expression), at the ragged K and N the
step fixtures never reach.  Runs on the MI355X only (-m gpu).

Tolerance: err32 is the error of the same expression evaluated by stock torch
in float32 on the CPU against float64, in the norm the check uses (relerr:
the 2-norm of the difference over the 2-norm of the reference); the kernel may
be 4 x err32 away (its summation order differs: lane-serial, then wave
shuffles, against torch's vectorised sums), a bf16 output 2^-8 more.  One
float32 evaluation of a scalar (a loss sum, a perplexity) or of a handful of
row norms is one sample of a rounding that can come out as exactly 0, so for
the forward outputs err32 is the largest of 16 such evaluations, each with the
channels (for the perplexity: the codes) in another order -- every output is
invariant under that order up to rounding."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
BETA = 0.25
N_PERM = 16


def _ops():
    from vae_npvc_amd import ops
    return ops


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def guarded(shape, dtype=F32, fill=NAN):
    """(whole, view): a tensor of `shape` and one more row (element) of sentinels behind it."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    whole = torch.full((shape[0] + 1,) + shape[1:], fill, device=DEV, dtype=dtype)
    return whole, whole[:shape[0]]


def intact(whole):
    """The sentinel row is still NaN and nothing before it is."""
    return bool(torch.isnan(whole[-1:]).all()) and not bool(torch.isnan(whole[:-1]).any())


def dev(t, dtype=F32):
    return t.to(dtype).to(DEV).contiguous()


# ---- inputs and the float64 reference

@functools.lru_cache(maxsize=None)
def make_inputs(D, K, N, normalize):
    """E [K, D], z [N, D] (float32 values) and code [N]: every frame next to
    its code, three codes unused.

    Without normalisation E and z are multiples of 2^-10.  There the kernel's
    operands are the frames and codes themselves, and the per-code sums bsum
    (at most 9 frames, |z| < 8) are then exact in float32, so casting the
    reference's forward to float32 loses nothing.  It matters for dE =
    s (cnt emb - bsum), which cancels to 2-3 % of its operands: with E and z
    off that grid the cast of bsum alone -- before any kernel arithmetic --
    puts dE 9e-7 .. 1.5e-6 from float64, 4.9 .. 6.0 x the bound below
    (measured; the kernel's result was that of a float64 evaluation from the
    cast inputs), which says nothing about the kernel."""
    gen = torch.Generator(device="cpu").manual_seed(1000 * D + 10 * K + N + int(normalize))
    E = torch.randn(K, D, generator=gen)
    code = torch.arange(N) % max(K - 3, 1)
    if normalize:
        rows = E[code] / E[code].norm(dim=1, keepdim=True)
        z = (rows + torch.randn(N, D, generator=gen) * 0.05 / D ** 0.5) * (0.5 + 2.0 * torch.rand(N, 1, generator=gen))
    else:
        E = torch.round(E * 1024) / 1024
        z = torch.round((E[code] + 0.05 * torch.randn(N, D, generator=gen)) * 1024) / 1024
    return E, z, code


def normalize_ref(E, z, dtype, perm=None):
    """vqx_vq_normalize in stock torch: embed_norm() on the parameter
    (layers_vq.py:28-33), then emb = 1.0 * E / ||E|| (:99) and z_norm = 1.0 * z / ||z|| (:97)."""
    E, z = E.to(dtype), z.to(dtype)
    inv = None
    if perm is not None:
        E, z, inv = E[:, perm], z[:, perm], torch.argsort(perm)
    E1 = E * (1.0 / E.norm(dim=1, keepdim=True))
    e_len = E1.norm(dim=1, keepdim=True)
    z_len = z.norm(dim=1, keepdim=True)
    zn = 1.0 * z / z_len
    out = dict(E=E1, emb_norm=1.0 * E1 / e_len, e_len=e_len.flatten(), z_norm=zn, z_len=z_len.flatten(),
               normloss=(zn - z).pow(2).sum().reshape(1))
    if inv is not None:
        for k in ("E", "emb_norm", "z_norm"):
            out[k] = out[k][:, inv]
    return out


def level_ref(E, z, normalize, BT, dzq=None, dtype=F64, perm=None):
    """VectorQuantizer.forward ('frame_mean', layers_vq.py:79-150) on frames z
    [N, D] with the codebook parameter E as it is after embed_norm(), and the
    gradients of (z_vq * dzq).sum() + z_qut + BETA * z_enc by autograd."""
    E, z = E.to(dtype), z.to(dtype)
    inv = None
    if perm is not None:
        E, z, inv = E[:, perm], z[:, perm], torch.argsort(perm)
        dzq = None if dzq is None else dzq[:, perm]
    E, z = E.clone().requires_grad_(), z.clone().requires_grad_()
    if normalize:
        z_len, e_len = z.norm(dim=1, keepdim=True), E.norm(dim=1, keepdim=True)
        zn, emb = 1.0 * z / z_len, 1.0 * E / e_len
    else:
        z_len = e_len = None
        zn, emb = z, E
    dist = zn.pow(2).sum(1, keepdim=True) + emb.pow(2).sum(1) - 2 * zn @ emb.t()
    idx = dist.argmin(1)
    top2 = dist.detach().topk(2, dim=1, largest=False).values if E.shape[0] > 1 else None
    zq = emb.index_select(0, idx)
    counts = torch.bincount(idx, minlength=E.shape[0]).to(dtype)
    p = counts / idx.numel()
    perp = torch.exp(-(p * torch.log(p + 1e-10)).sum())
    qut_sum = (zq - zn.detach()).pow(2).sum()
    enc = (zq.detach() - zn).pow(2)
    norm_sum = (zn - z).pow(2).sum() if normalize else None
    if normalize:
        enc = enc + (zn - z).pow(2)
    z_vq = zn + (zq - zn).detach()
    loss = qut_sum / BT + BETA * (enc.sum() / BT)
    if dzq is not None:
        loss = loss + (z_vq * dzq.to(dtype)).sum()
    loss.backward()
    out = dict(z_norm=zn.detach(), emb=emb.detach(), zq=zq.detach(), idx=idx, counts=counts,
               bsum=torch.zeros_like(emb).index_add_(0, idx, zn.detach()), perp=perp.detach().reshape(1),
               qut_sum=qut_sum.detach().reshape(1), dz=z.grad, dE=E.grad)
    if normalize:
        out.update(z_len=z_len.detach().flatten(), e_len=e_len.detach().flatten(),
                   norm_sum=norm_sum.detach().reshape(1))
    if top2 is not None:
        out["gap"] = float(((top2[:, 1] - top2[:, 0]) / top2[:, 1]).min())
    if inv is not None:
        for k in ("z_norm", "emb", "zq", "bsum", "dz", "dE"):
            out[k] = out[k][:, inv]
    return out


def perms(D, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randperm(D, generator=gen) for _ in range(N_PERM)]


def worst_err32(evaluate, ref, keys, D, seed):
    """{key: the largest relerr of evaluate(perm)[key] (float32) against ref[key] over N_PERM channel orders}."""
    err = {k: 0.0 for k in keys}
    for perm in perms(D, seed):
        got = evaluate(perm)
        for k in keys:
            err[k] = max(err[k], relerr(got[k], ref[k]))
    return err


def check(name, got, ref, err32, ratios, extra=0.0):
    e = relerr(got, ref)
    bound = 4 * err32 + extra
    ratios[name] = e / bound if bound > 0 else (0.0 if e == 0 else float("inf"))
    print(f"  {name}: err {e:.3g} err32 {err32:.3g} ratio {ratios[name]:.3f}")
    return e <= bound


def jitter_map(T, seed):
    """src_t of the Jitter (layers_vq.py:353-379): about a third of the frames
    replaced by a neighbour, the first and the last among them."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    src = torch.arange(T, dtype=torch.int32)
    for t in (torch.randperm(T - 2, generator=gen)[:T // 3 - 2] + 1).tolist():
        src[t] = t + (1 if torch.rand(1, generator=gen).item() < 0.5 else -1)
    src[0], src[T - 1] = 1, T - 2
    return src


def assert_reference_is_decisive(ref, code):
    """No near-tie in the float64 reference: the argmin is the code the frame was built from."""
    assert torch.equal(ref["idx"], code)
    assert ref.get("gap", 1.0) >= 1e-2, ref["gap"]


# ---- vqx_vq_normalize

@pytest.mark.parametrize("K,N", [(18, 37), (48, 130), (16, 1)])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_vq_normalize_matches_float64(D, K, N):
    """vqx_vq_normalize at K % 4 != 0 and N % 4 != 0 (the last codebook block
    and the last frame block hold idle waves; N = 1 is a single frame block):
    E renormalised in place, emb_norm, e_len, z_norm, z_len and the
    normalisation loss sum against float64 within 4 x err32; a second call on
    the already normalised E keeps E within the same bound; with normloss_out
    NULL every other output has the same bits.  Worst error / bound over the
    nine cases, measured on the MI355X (pytest -s prints each): E 0.24 (0.31
    after the second call), emb_norm 0.24, e_len 0.21, z_norm 0.25, z_len
    0.25, normloss 0.25."""
    ops = _ops()
    E0, z, _ = make_inputs(D, K, N, True)
    ref = normalize_ref(E0, z, F64)
    keys = ("E", "emb_norm", "e_len", "z_norm", "z_len", "normloss")
    err32 = worst_err32(lambda perm: normalize_ref(E0, z, F32, perm), ref, keys, D, 5 * D + K)
    zd = dev(z)
    runs = []
    for with_loss in (True, False):
        o = {k: guarded(s) for k, s in (("E", (K, D)), ("emb_norm", (K, D)), ("e_len", K), ("z_norm", (N, D)),
                                        ("z_len", N), ("normloss", 1), ("part", N // 4 + 1))}
        o["E"][1].copy_(dev(E0))
        ops.vq_normalize(zd, o["E"][1], o["z_norm"][1], o["z_len"][1], o["emb_norm"][1], o["e_len"][1], o["part"][1],
                         o["normloss"][1] if with_loss else None)
        torch.cuda.synchronize()
        runs.append(o)
    a, b = runs
    print(f"vq_normalize D={D} K={K} N={N}")
    ratios = {}
    for k in keys:
        assert intact(a[k][0]), k
        assert check(k, a[k][1], ref[k], err32[k], ratios), (k, ratios[k])
    assert bool(torch.isnan(a["part"][0][(N + 3) // 4:]).all())
    for k in ("E", "emb_norm", "e_len", "z_norm", "z_len"):
        assert intact(b[k][0]) and torch.equal(a[k][0][:-1], b[k][0][:-1]), k
    assert bool(torch.isnan(b["normloss"][0]).all())
    # once more on the normalised codebook
    ops.vq_normalize(zd, a["E"][1], a["z_norm"][1], a["z_len"][1], a["emb_norm"][1], a["e_len"][1], a["part"][1], None)
    torch.cuda.synchronize()
    assert intact(a["E"][0]) and check("E twice", a["E"][1], ref["E"], err32["E"], ratios), ratios


# ---- vqx_vq_perplexity

def _perplexity(counts, n_rows, dtype):
    p = counts.to(dtype) / n_rows
    return torch.exp(-(p * torch.log(p + 1e-10)).sum()).reshape(1)


@pytest.mark.parametrize("K", [1, 18, 512, 2048])
def test_vq_perplexity_matches_float64(K):
    """vqx_vq_perplexity = exp(-sum p log(p + 1e-10)), p = counts / n_rows, for
    counts with about half the codes empty and n_rows odd (K = 1: every frame
    in the one code), and for one code holding every frame of a K-code book
    (perplexity 1).  Within 4 x err32; measured error / bound on the MI355X:
    0.25 (K = 1, 18), 0.19 (512), 0.22 (2048), and 0.25 at perplexity 1, where
    kernel and float32 torch both return exactly 1."""
    ops = _ops()
    gen = torch.Generator(device="cpu").manual_seed(90 + K)
    counts = torch.randint(0, 40, (K,), generator=gen).float() * (torch.rand(K, generator=gen) < 0.5)
    counts[K // 2] += 3 - (int(counts.sum()) % 2)  # never empty, and an odd total >= 3: no power of two
    single = torch.zeros(K)
    single[K - 1] = 1001
    ratios = {}
    print(f"vq_perplexity K={K}")
    for name, c in (("mixed", counts), ("single", single)):
        n_rows = int(c.sum())
        assert n_rows & (n_rows - 1) and (K == 1 or name == "single" or bool((c == 0).any()))
        ref = _perplexity(c, n_rows, F64)
        err32 = max(relerr(_perplexity(c[torch.randperm(K, generator=gen)], n_rows, F32), ref) for _ in range(N_PERM))
        whole, out = guarded(1)
        ops.vq_perplexity(dev(c), n_rows, out)
        torch.cuda.synchronize()
        assert intact(whole)
        assert check(name, out, ref, err32, ratios), (name, float(out), float(ref))
        if name == "single" or K == 1:
            assert abs(float(out) - 1.0) < 1e-6


# ---- vqx_vq_plain_bwd, fed the reference's forward

def _bwd_inputs(ref, E, z, normalize):
    """The device inputs of vqx_vq_plain_bwd from the reference's forward, cast to float32."""
    d = dict(z=dev(z), z_norm=dev(ref["z_norm"]), zq=dev(ref["zq"]), bsum=dev(ref["bsum"]), bcnt=dev(ref["counts"]),
             emb=dev(ref["emb"]), z_len=None, e_len=None)
    if normalize:
        d.update(z_len=dev(ref["z_len"]), e_len=dev(ref["e_len"]))
    return d


def _plain_bwd(ops, d, dzq, src_t, T, normalize, scale, dtype, K, D, N):
    dz_w, dz = guarded((N, D), dtype)
    dE_w, dE = guarded((K, D))
    ops.vq_plain_bwd(d["z"], d["z_norm"], d["z_len"], d["zq"], dzq, src_t, T, normalize, BETA, scale, dz, d["bsum"],
                     d["bcnt"], d["emb"], d["e_len"], dE)
    torch.cuda.synchronize()
    assert intact(dz_w) and intact(dE_w)
    return dz, dE


@pytest.mark.parametrize("normalize", [0, 1], ids=["plain", "norm"])
@pytest.mark.parametrize("B,T", [(1, 37), (3, 43)])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_vq_plain_bwd_matches_float64_autograd(D, B, T, normalize):
    """vqx_vq_plain_bwd alone (K = 18: the last codebook block has two idle
    waves; N = 37 / 129: a ragged last frame block), fed z_norm, z_len, zq,
    bsum, bcnt, emb_norm and e_len of the float64 forward cast to float32.
    dz (fp32 and bf16, dzq in the same dtype) and dE against the float64
    autograd gradients of (z_vq * st(dzq)).sum() + z_qut + 0.25 * z_enc, for
    dzq NULL, dzq random, and dzq random under a jitter map that replaces a
    third of the frames (t = 0 and T - 1 among them), beta 0.25, scale
    2 / (B T); within 4 x err32 (+ 2^-8 for bf16 dz).  The dE rows of the three
    unused codes are exactly 0.  Worst error / bound measured on the MI355X:
    dz 0.25 (fp32), 0.44 (bf16), dE 0.65.  (make_inputs says why the
    unnormalised inputs lie on a 2^-10 grid.)"""
    ops = _ops()
    K, N = 18, B * T
    E0, z, code = make_inputs(D, K, N, bool(normalize))
    E = normalize_ref(E0, z, F64)["E"].float() if normalize else E0  # the parameter after embed_norm()
    gen = torch.Generator(device="cpu").manual_seed(31 * D + N)
    dzq32 = torch.randn(N, D, generator=gen)
    src = jitter_map(T, 7 * D + T)
    kept = (src == torch.arange(T, dtype=torch.int32)).repeat(B).view(N, 1)
    assert int((~kept).sum()) >= B * (T // 3) and not bool(kept[0]) and not bool(kept[T - 1])
    base = level_ref(E, z, normalize, N)
    assert_reference_is_decisive(base, code)
    assert int((base["counts"] == 0).sum()) == 3
    assert normalize or torch.equal(base["bsum"].float().double(), base["bsum"])  # make_inputs: a lossless cast
    d = _bwd_inputs(base, E, z, normalize)
    scale = 2.0 / N
    print(f"vq_plain_bwd D={D} B={B} T={T} normalize={normalize}")
    ratios = {}
    for dtype in (F32, torch.bfloat16):
        dzq_v = dzq32.to(dtype)  # the values the kernel reads
        for name, dzq, src_t in (("none", None, None), ("dzq", dzq_v, None), ("jitter", dzq_v, src)):
            masked = None if dzq is None else dzq.double() * (kept if src_t is not None else 1.0)
            ref = level_ref(E, z, normalize, N, masked)
            r32 = level_ref(E, z, normalize, N, masked, F32)
            dz, dE = _plain_bwd(ops, d, None if dzq is None else dev(dzq, dtype),
                                None if src_t is None else src_t.to(DEV), T, normalize, scale, dtype, K, D, N)
            tag = f"{name}/{'bf16' if dtype != F32 else 'f32'}"
            assert check(f"dz {tag}", dz, ref["dz"], relerr(r32["dz"], ref["dz"]), ratios,
                         2.0 ** -8 if dtype != F32 else 0.0), ratios
            assert check(f"dE {tag}", dE, ref["dE"], relerr(r32["dE"], ref["dE"]), ratios), ratios
            assert bool((dE[base["counts"].to(DEV) == 0] == 0).all())


@pytest.mark.parametrize("normalize", [0, 1], ids=["plain", "norm"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_vq_plain_bwd_g_bit_identities(D, normalize):
    """vqx_vq_plain_bwd_g with both upstream gradients NULL, s_qut = scale and
    s_enc = float32(beta * scale) has vqx_vq_plain_bwd's bits; with device
    scalars g_qut, g_enc it has the bits of the call whose s_qut, s_enc were
    multiplied by them on the host in float32 (K = 18, B x T = 3 x 43, fp32
    and bf16 dz)."""
    ops = _ops()
    K, B, T = 18, 3, 43
    N = B * T
    E0, z, code = make_inputs(D, K, N, bool(normalize))
    E = normalize_ref(E0, z, F64)["E"].float() if normalize else E0
    base = level_ref(E, z, normalize, N)
    assert_reference_is_decisive(base, code)
    d = _bwd_inputs(base, E, z, normalize)
    gen = torch.Generator(device="cpu").manual_seed(17 * D + normalize)
    dzq32 = torch.randn(N, D, generator=gen)
    scale = np.float32(2.0 / N)
    s_enc = np.float32(BETA) * scale
    gq, ge = np.float32(0.37), np.float32(-1.9)

    def bwd_g(dtype, dzq, s_qut, s_enc, g_qut, g_enc):
        dz_w, dz = guarded((N, D), dtype)
        dE_w, dE = guarded((K, D))
        ops.vq_plain_bwd_g(d["z"], d["z_norm"], d["z_len"], d["zq"], dzq, T, normalize, float(s_qut), float(s_enc),
                           g_qut, g_enc, dz, d["bsum"], d["bcnt"], d["emb"], d["e_len"], dE)
        torch.cuda.synchronize()
        assert intact(dz_w) and intact(dE_w)
        return dz, dE

    for dtype in (F32, torch.bfloat16):
        dzq = dev(dzq32, dtype)
        want = _plain_bwd(ops, d, dzq, None, T, normalize, float(scale), dtype, K, D, N)
        got = bwd_g(dtype, dzq, scale, s_enc, None, None)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), dtype
        dev_g = bwd_g(dtype, dzq, scale, s_enc, torch.tensor([gq], device=DEV), torch.tensor([ge], device=DEV))
        host_g = bwd_g(dtype, dzq, scale * gq, s_enc * ge, None, None)
        assert torch.equal(dev_g[0], host_g[0]) and torch.equal(dev_g[1], host_g[1]), dtype
        assert not torch.equal(dev_g[1], want[1])


# ---- the whole level

@pytest.mark.parametrize("D", [64, 128, 256])
def test_vq_plain_level_chain_matches_float64(D):
    """vqx_vq_normalize -> vqx_vq_forward (zeroed bsum / bcnt) ->
    vqx_vq_perplexity -> vqx_vq_plain_bwd on K = 48 codes (three unused) and
    N = 2 x 65 frames, normalised, dzq under a jitter map: the indices equal
    the float64 argmin (smallest relative top-2 gap ~ 0.99), the commitment
    and normalisation loss sums, the perplexity, dz and dE within 4 x err32.
    Worst error / bound measured on the MI355X: qut_sum 0.25, norm_sum 0.16,
    perplexity 0.52, dz 0.25, dE 0.43."""
    ops = _ops()
    K, B, T = 48, 2, 65
    N = B * T
    E0, z, code = make_inputs(D, K, N, True)
    gen = torch.Generator(device="cpu").manual_seed(53 * D)
    dzq = torch.randn(N, D, generator=gen)
    src = jitter_map(T, 3 * D)
    kept = (src == torch.arange(T, dtype=torch.int32)).repeat(B).view(N, 1)
    E1 = normalize_ref(E0, z, F64)["E"]  # float64: what embed_norm() leaves exactly
    ref = level_ref(E1, z, 1, N, dzq.double() * kept)
    assert_reference_is_decisive(ref, code)
    keys = ("qut_sum", "norm_sum", "perp", "dz", "dE")
    E1_32 = normalize_ref(E0, z, F32)["E"]
    err32 = worst_err32(lambda perm: level_ref(E1_32, z, 1, N, dzq * kept, F32, perm), ref, keys, D, 11 * D)
    zd = dev(z)
    E_w, Ed = guarded((K, D))
    Ed.copy_(dev(E0))
    o = {k: guarded(s) for k, s in (("emb", (K, D)), ("e_len", K), ("z_norm", (N, D)), ("z_len", N), ("zq", (N, D)),
                                    ("stats", 3), ("part", N // 4 + 1), ("dE", (K, D)), ("dz", (N, D)))}
    idx_w, idx = guarded(N, torch.int64, -1)
    bsum, bcnt = torch.zeros(K, D, device=DEV), torch.zeros(K, device=DEV)
    stats = o["stats"][1]
    ops.vq_normalize(zd, Ed, o["z_norm"][1], o["z_len"][1], o["emb"][1], o["e_len"][1], o["part"][1], stats[1:2])
    ops.vq_forward(o["z_norm"][1], o["emb"][1], idx, o["zq"][1], None, stats[0:1], None, bsum, bcnt)
    ops.vq_perplexity(bcnt, N, stats[2:3])
    ops.vq_plain_bwd(zd, o["z_norm"][1], o["z_len"][1], o["zq"][1], dev(dzq), src.to(DEV), T, 1, BETA, 2.0 / N,
                     o["dz"][1], bsum, bcnt, o["emb"][1], o["e_len"][1], o["dE"][1])
    torch.cuda.synchronize()
    for k in ("emb", "e_len", "z_norm", "z_len", "zq", "stats", "dE", "dz"):
        assert intact(o[k][0]), k
    assert intact(E_w) and int(idx_w[-1]) == -1
    assert torch.equal(idx.cpu(), ref["idx"])
    assert torch.equal(bcnt.cpu().double(), ref["counts"])
    print(f"vq level chain D={D}")
    ratios = {}
    for k, got in (("qut_sum", stats[0:1]), ("norm_sum", stats[1:2]), ("perp", stats[2:3]), ("dz", o["dz"][1]),
                   ("dE", o["dE"][1])):
        assert check(k, got, ref[k], err32[k], ratios), (k, ratios)
    assert bool((o["dE"][1][bcnt == 0] == 0).all()) and int((bcnt == 0).sum()) == 3
