"""`EMAVectorQuantizer.forward`, `Jitter` and the jitter path of
`VectorQuantizer.forward` on the MI355X against the reference's float64
fixtures (tests/golden/make_golden_vqvae2a.py: vqema_<case>, vqjit_<case>),
under the stored seeds.  Bound as tests/test_gpu_hier_encoder.py:
max|got - f64| / max|f64| <= max(8 * err32, 16 * 2^-23) per tensor."""
import numpy as np
import pytest
import torch

from tests.hier_model_ref import fixture
from tests.test_gpu_hier_encoder import ratios, report

pytestmark = pytest.mark.gpu
EMA_CASES = ("init_k16", "tile_k64", "dead_k16", "k512")
BUFFERS = ("emb_sum", "emb_elem", "embeddings")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def reseed(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)


def build_ema(meta, arr):
    from vae_npvc_amd.model.layers_vq import EMAVectorQuantizer
    q = EMAVectorQuantizer(meta["K"], meta["D"], meta["mu"], threshold=meta["threshold"])
    state = {k[len("state."):]: torch.from_numpy(v.copy()) for k, v in arr.items() if k.startswith("state.")}
    if state:
        q.load_state_dict(state, strict=True)
    return q.cuda().train()


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("case", EMA_CASES)
def test_ema_level_matches_the_float64_reference(case, weighted):
    meta, arr = fixture("vqema", case)
    q = build_ema(meta, arr)
    was_init = bool(q.emb_init)
    assert was_init == ("state.emb_init" in arr)
    reseed(meta["run_seed"])
    got, want = {}, {}
    for n in meta["steps_names"]:
        if n == "eval":
            continue
        z = cuda(arr[f"{n}.z"]).requires_grad_()
        if weighted:
            z_vq, loss, zero, enc, detail = q(z, loss_weights=(1.0, meta["w_enc"]))
            assert not enc.requires_grad
        else:
            z_vq, zero, enc, detail = q(z)
            loss = meta["w_enc"] * enc
        assert zero == 0.0 and not z_vq.requires_grad and list(detail) == meta["detail_keys"]
        assert all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in detail.values())
        loss.backward()
        assert torch.equal(q.last_indices.cpu(), torch.from_numpy(arr[f"{n}.idx"].copy())), n
        assert bool(q.emb_init) and q.initialized  # flips once, on the first training call
        res = {"z_vq": z_vq, "z_enc_loss": enc.detach(), "dz": z.grad, **{k: v.detach() for k, v in detail.items()}}
        res.update({"buf." + k: getattr(q, k).detach().clone() for k in BUFFERS})
        for k, v in res.items():
            got[f"{n}.{k}"], want[f"{n}.{k}"] = v, arr[f"{n}.{k}"]
        assert bool(arr[f"{n}.buf.emb_init"])
        if case == "dead_k16":  # the replaced rows are the reference's: frames of z, bit for bit
            dead = arr[f"{n}.buf.emb_elem"] < meta["threshold"]
            assert 0 < dead.sum() and float(arr[f"{n}.usage"]) == meta["K"] - dead.sum() < meta["K"]
            assert np.array_equal(q.embeddings.cpu().numpy()[dead], arr[f"{n}.buf.embeddings"][dead])
    report(f"vqema {case} {'weighted' if weighted else 'plain'}", ratios(got, want, meta["err32"]))
    if meta["eval_after"]:
        q.eval()
        before = {k: v.detach().clone() for k, v in q.state_dict().items()}
        z = cuda(arr[f"s{meta['steps']}.z"])
        z_vq, zero, enc, detail = q(z)
        assert detail == {} and zero == 0.0
        assert all(torch.equal(v, before[k]) for k, v in q.state_dict().items())  # bit-identical buffers
        assert torch.equal(q.last_indices.cpu(), torch.from_numpy(arr["eval.idx"].copy()))
        report(f"vqema {case} eval", ratios({"eval.z_vq": z_vq, "eval.z_enc_loss": enc},
                                            {k: arr[k] for k in ("eval.z_vq", "eval.z_enc_loss")}, meta["err32"]))


@pytest.mark.parametrize("K", [16, 512, 1024])
def test_dead_code_rows_on_both_sides_of_the_512_code_threshold(K):
    """mu = 1 keeps emb_sum / emb_elem (1*a + 0*b), and with threshold 2 > emb_elem = 1 every code counts as dead:
    the codebook after the first training call is z[second permutation] bit for bit, whether the rows are read
    inside the update launch (K <= 512) or gathered before it, and z_vq shows the first permutation's rows."""
    from vae_npvc_amd.model.layers_vq import EMAVectorQuantizer
    D, B, T = 64, 4, 512
    z = torch.randn(B, D, T, generator=torch.Generator().manual_seed(K)).cuda()
    zf = z.transpose(1, 2).reshape(-1, D)
    torch.manual_seed(5)
    perm1, perm2 = torch.randperm(B * T)[:K].cuda(), torch.randperm(B * T)[:K].cuda()
    q = EMAVectorQuantizer(K, D, 1.0, threshold=2.0).cuda().train()
    torch.manual_seed(5)
    z_vq, _, _, detail = q(z)
    assert torch.equal(q.embeddings, zf[perm2])
    assert torch.equal(q.emb_sum, zf[perm1]) and torch.equal(q.emb_elem, torch.ones(K, device="cuda"))
    assert float(detail["usage"]) == 0.0
    zq = z_vq.transpose(1, 2).reshape(-1, D)
    assert torch.equal(zq[perm1], zf[perm1])  # a frame that became a code is its own nearest code


def test_ema_level_limits_raise_before_any_launch():
    from vae_npvc_amd.model.layers_vq import EMAVectorQuantizer
    for K, D, what in ((16, 32, "z_dim"), (24, 64, "z_num"), (4096, 64, "z_num")):
        q = EMAVectorQuantizer(K, D, 0.9).cuda().train()
        with pytest.raises(NotImplementedError, match=what):
            q(torch.zeros(2, D, 4, device="cuda"))
        assert not bool(q.emb_init)
    q = EMAVectorQuantizer(16, 64, 0.9).cuda().train()
    with pytest.raises(ValueError, match="channels"):
        q(torch.zeros(2, 32, 4, device="cuda"))


def test_jitter_module_matches_the_reference():
    from vae_npvc_amd.model.layers_vq import Jitter
    meta, arr = fixture("vqjit", "jitter")
    x, go = cuda(arr["x"]).requires_grad_(), cuda(arr["go"])
    jit = Jitter(meta["p"]).train()
    reseed(meta["run_seed"])
    y = jit(x)
    assert float(np.random.random_sample()) == meta["next_uniform"]
    (y * go).sum().backward()
    report("vqjit jitter", ratios({"y": y.detach(), "dx": x.grad}, {"y": arr["y"], "dx": arr["dx"]}, meta["err32"]))
    replaced = torch.from_numpy(arr["map"] != np.arange(meta["T"])).cuda()
    assert bool(replaced.any()) and not bool(replaced.all())
    assert not bool(x.grad[:, :, replaced].abs().sum())  # exact zeros: a replaced frame passes no gradient
    assert torch.equal(x.grad[:, :, ~replaced], go[:, :, ~replaced])
    assert jit.eval()(x) is x


def _plain(meta, arr):
    from vae_npvc_amd.model.layers_vq import VectorQuantizer
    q = VectorQuantizer(meta["K"], meta["D"], normalize=meta["normalize"])
    q.load_state_dict({"embeddings": torch.from_numpy(arr["param.embeddings"].copy())})
    return q.cuda()


def test_plain_quantizer_with_a_jitter_map_matches_the_reference():
    from vae_npvc_amd.model.layers_vq import Jitter
    meta, arr = fixture("vqjit", "plain_jitter")
    q = _plain(meta, arr)
    z, go = cuda(arr["z"]).requires_grad_(), cuda(arr["go"])
    reseed(meta["run_seed"])
    src = Jitter(meta["p"]).train().draw(meta["T"])
    assert src.tolist() == arr["map"].tolist()
    z_vq, qut, enc, detail = q(z, src_t=src)
    w_qut, w_enc = meta["loss_weights"]
    ((z_vq * go).sum() + w_qut * qut + w_enc * enc).backward()
    assert meta["gap"] >= 1e-3
    assert torch.equal(q.forward_indices(z.detach()).cpu(), torch.from_numpy(arr["idx"].copy()))
    got = {"z_vq": z_vq.detach(), "z_qut_loss": qut.detach(), "z_enc_loss": enc.detach(), "entropy": detail["entropy"],
           "dz": z.grad, "dE": q.embeddings.grad}
    report("vqjit plain_jitter", ratios(got, {k: arr[k] for k in got}, meta["err32"]))


def test_plain_quantizer_without_a_map_keeps_its_bits():
    meta, arr = fixture("vqjit", "plain_jitter")
    outs = []
    for kw in ({}, {"src_t": None}):
        q = _plain(meta, arr)
        z, go = cuda(arr["z"]).requires_grad_(), cuda(arr["go"])
        z_vq, loss, qut, enc, detail = q(z, loss_weights=(1.0, 0.25), **kw)
        ((z_vq * go).sum() + loss).backward()
        outs.append((z_vq.detach(), loss.detach(), qut, enc, detail["entropy"], z.grad, q.embeddings.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # an identity map goes through the two new kernels and gives the same bits as well
    q = _plain(meta, arr)
    z, go = cuda(arr["z"]).requires_grad_(), cuda(arr["go"])
    z_vq, loss, qut, enc, detail = q(z, loss_weights=(1.0, 0.25), src_t=np.arange(meta["T"], dtype=np.int32))
    ((z_vq * go).sum() + loss).backward()
    third = (z_vq.detach(), loss.detach(), qut, enc, detail["entropy"], z.grad, q.embeddings.grad)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], third))
