"""`vqvae2a.Model` on the MI355X against the reference's float64 fixtures
(tests/golden/make_golden_vqvae2a.py, vq2a_<case>) step by step under the
stored seeds, its encode / convert, bf16, this package's Trainer on it and the
reference trainer's loop.  Bound as tests/test_gpu_hier_encoder.py;
`mha.linear_k.bias` has a mathematically zero gradient, so its bound is
absolute (tests/test_gpu_hier_model.py)."""
import numpy as np
import pytest
import torch

from tests.hier_model_ref import ULP16, fixture
from tests.test_gpu_hier_encoder import ratios, report

pytestmark = pytest.mark.gpu
MODEL_CASES = ("ema_gst", "plain_shared", "single_ema")
TRAIN = dict(learning_rate=1e-3, max_grad_norm=0.5, optim_type="Adam", lr_scheduler="StepLR",
             lr_param={"step_size": 1, "gamma": 0.5})


def reseed(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)


def state_dict(meta, arr):
    return {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}


def build_model(meta, arr, **over):
    from vae_npvc_amd.model.vqvae2a import Model
    m = Model(dict(meta["arch"], **over))
    assert list(m.state_dict().keys()) == meta["keys"]
    m.load_state_dict(state_dict(meta, arr), strict=True)
    return m.cuda().train()


def batch(arr):
    return torch.from_numpy(arr["x"].copy()).cuda(), torch.from_numpy(arr["y"].copy()).cuda()


def codebooks(m):
    mods = list(m.quantizers) if m.use_quantizers else [m.quantizer]
    return [q for q in mods if hasattr(q, "embeddings")]


def record_indices(m, sink):
    """Every codebook lookup of a forward appends its indices, in the order they run: an EMA level's own
    (`last_indices`), a plain level's from the same launches on the input it received."""
    from vae_npvc_amd.model.layers_vq import EMAVectorQuantizer
    hooks = []
    for q in codebooks(m):
        if isinstance(q, EMAVectorQuantizer):
            hooks.append(q.register_forward_hook(lambda mod, inp, out: sink.append(mod.last_indices.cpu())))
        else:
            hooks.append(q.register_forward_pre_hook(
                lambda mod, inp: sink.append(mod.forward_indices(inp[0].detach()).cpu())))
    return hooks


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_steps_match_the_float64_reference(case):
    meta, arr = fixture("vq2a", case)
    assert meta["gap"] >= 1e-3
    m = build_model(meta, arr)
    x, y = batch(arr)
    ids = []
    hooks = record_indices(m, ids)
    reseed(meta["run_seed"])
    for n in range(1, meta["steps"] + 1):
        p = f"s{n}."
        m.zero_grad(set_to_none=True)
        del ids[:]
        xhat, loss, detail = m((x, y))
        assert list(detail) == meta["loss_keys"][n - 1] and all(isinstance(v, float) for v in detail.values())
        loss.backward()
        assert len(ids) == meta["lookups"][n - 1]
        for j, idx in enumerate(ids):
            assert torch.equal(idx, torch.from_numpy(arr[p + f"idx.{j}"].copy())), (n, j)
        got = {p + "xhat": xhat.detach()}
        got.update({p + "loss." + k: torch.tensor(v, dtype=torch.float64) for k, v in detail.items()})
        got.update({p + "grad." + k: g.grad for k, g in m.named_parameters() if g.grad is not None})
        got.update({p + "buf." + k: b.detach().clone() for k, b in m.named_buffers() if b.is_floating_point()})
        assert sorted(k for k, g in m.named_parameters() if g.grad is not None) == sorted(meta["grads"])
        want = {k: arr[k] for k in got if k not in meta["abs32"]}
        assert set(want) == {k for k in meta["err32"] if k.startswith(p)}
        report(f"vq2a {case} step {n}", ratios(got, want, meta["err32"]))
        for k, a32 in meta["abs32"].items():  # exactly zero in exact arithmetic
            if k.startswith(p):
                scale = float(np.abs(arr[k[:-4] + "weight"]).max())
                assert float(got[k].abs().max()) <= max(8 * a32, ULP16 * scale), k
        for k, b in m.named_buffers():
            if not b.is_floating_point():
                assert bool(b) == bool(arr[p + "buf." + k]), k
        assert float(loss.detach()) == detail["Total"]
    for h in hooks:
        h.remove()
    # encode in eval mode after the last step
    m.eval()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    codes = m.encode(x)
    assert len(codes) == m.levels
    got, want = {}, {}
    for i, c in enumerate(codes):
        if c.is_floating_point():
            got[f"enc.{i}"], want[f"enc.{i}"] = c, arr[f"enc.{i}"]
        else:
            assert c.dtype == torch.int64 and torch.equal(c.cpu(), torch.from_numpy(arr[f"enc.{i}"].copy())), i
    if got:
        report(f"vq2a {case} encode", ratios(got, want, meta["err32"]))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize("case", MODEL_CASES)
def test_convert_is_the_eval_forward_and_writes_nothing(case):
    meta, arr = fixture("vq2a", case)
    m = build_model(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    m((x, y))  # one training forward: the EMA codebooks are initialised
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out = m.convert((x, y))
    assert m.training and not out.requires_grad
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    m.eval()
    with torch.no_grad():
        xhat, _, detail = m((x, y))
    assert torch.equal(out, xhat)
    k_q = len(meta["loss_keys"][0]) - 3
    assert [k for k in detail if k.startswith("quanti_err")] == [f"quanti_err.{k}" for k in range(meta["lookups"][0])]
    if m.use_ema:  # an EMA level reports nothing else in eval mode
        assert list(detail) == ["Total", "VQ loss", "X like"] + [f"quanti_err.{k}" for k in range(meta["lookups"][0])]
        assert k_q == 5 * meta["lookups"][0]


def test_decoder_hier_drives_convert():
    from vae_npvc_amd.decoder.hier import Decoder
    meta, arr = fixture("vq2a", "single_ema")
    m = build_model(meta, arr)
    x, y = batch(arr)
    dec = Decoder.__new__(Decoder)
    dec.model = m
    assert torch.equal(dec.decode_step(x[:1], y[:1]), m.convert((x[:1], y[:1])))


def test_bf16_step_is_finite_with_the_same_keys():
    meta, arr = fixture("vq2a", "ema_gst")
    m = build_model(meta, arr, compute_dtype="bf16")
    x, y = batch(arr)
    reseed(meta["run_seed"])
    xhat, loss, detail = m((x, y))
    loss.backward()
    assert list(detail) == meta["loss_keys"][0] and all(np.isfinite(v) for v in detail.values())
    assert bool(torch.isfinite(xhat).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert all(bool(torch.isfinite(b).all()) for b in m.buffers())


def test_mean_pool_is_the_mean_and_its_adjoint():
    """The pooled quantized top level (pooling_last without a style layer).  A sum of T fp32 terms in any order
    is within (T - 1) * 2^-24 * sum|z_t| of the exact sum, and the 1/T scaling rounds once more."""
    from vae_npvc_amd.model.vqvae2a import mean_pool
    B, C, T = 3, 64, 37
    z = torch.randn(B, C, T, generator=torch.Generator().manual_seed(8)).cuda().requires_grad_()
    go = torch.randn(B, C, 1, generator=torch.Generator().manual_seed(9)).cuda()
    out = mean_pool(z)
    (out * go).sum().backward()
    exact = z.detach().double().mean(dim=-1, keepdim=True)
    bound = T * 2.0 ** -24 * z.detach().double().abs().mean(dim=-1, keepdim=True) + 2.0 ** -23 * exact.abs()
    assert tuple(out.shape) == (B, C, 1) and bool(((out.double() - exact).abs() <= bound).all())
    want = (go.double() / T).expand(B, C, T)
    assert bool(((z.grad.double() - want).abs() <= 2.0 ** -23 * want.abs()).all())


def test_two_levels_with_a_mean_pooled_ema_top_level_train():
    """levels 2 without a style layer: the top level is mean-pooled to one frame, so its EMA codebook sees
    B = 2 < K frames and takes the host tiling path at init and at every update.  No fixture anchors this
    configuration: the step runs, every value is finite, every parameter receives a gradient."""
    from vae_npvc_amd.model.vqvae2a import Model
    arch = fixture("vq2a", "ema_gst")[0]["arch"]
    arch = dict(arch, levels=2, use_gst=False, pooling_last=True, jitter_p=0.0,
                **{"decoder.1": dict(arch["decoder.1"], in_channels=[64])})
    reseed(3)
    m = Model(arch).cuda().train()
    x, y = batch(fixture("vq2a", "ema_gst")[1])
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        xhat, loss, detail = m((x, y))
        loss.backward()
        assert list(detail) == ["Total", "VQ loss", "X like"] + [
            f"{k}.{i}" for i in range(2) for k in ("entropy", "used_curr", "usage", "diff_emb", "quanti_err")]
        assert all(np.isfinite(v) for v in detail.values()) and tuple(xhat.shape) == tuple(x.shape)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert tuple(m.quantizers[1].last_indices.shape) == (2, 1)
    assert all(bool(q.emb_init) and bool(torch.isfinite(q.embeddings).all()) for q in m.quantizers)
    assert [tuple(c.shape) for c in m.encode(x)] == [(2, 64), (2, 1)]


def trainer(meta, arr, **over):
    from vae_npvc_amd.trainer.basic import Trainer
    cfg = dict(meta["arch"], **TRAIN, model_type="vae_npvc_amd.model.vqvae2a",
               trainer_type="vae_npvc_amd.trainer.basic", **over)
    tr = Trainer(cfg)
    tr.model.load_state_dict(state_dict(meta, arr))
    assert tr.engine.params_intact()
    return tr


def test_trainer_steps_validates_and_checkpoints(tmp_path):
    meta, arr = fixture("vq2a", "ema_gst")
    tr = trainer(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    totals = []
    for s in range(2):
        it, detail = tr.train_step((x, y))
        assert it == s + 1 and list(detail) == meta["loss_keys"][s] and all(np.isfinite(v) for v in detail.values())
        totals.append(detail["Total"])
    assert totals[0] != totals[1]
    assert all(bool(q.emb_init) for q in codebooks(tr.model))
    # valid_step leaves parameters and buffers bit-identical, and the model in training mode
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    rng = torch.get_rng_state()
    vdetail = tr.valid_step((x, y))
    assert list(vdetail) == ["Total", "VQ loss", "X like", "quanti_err.0", "quanti_err.1"]
    assert tr.model.training and torch.equal(torch.get_rng_state(), rng)
    assert all(torch.equal(v, before[k]) for k, v in tr.model.state_dict().items())
    # checkpoint round trip: parameters, EMA buffers, emb_init, moments, iteration
    path = tmp_path / "ck.pt"
    tr.save_checkpoint(str(path))
    tr2 = trainer(meta, arr)
    assert not any(bool(q.emb_init) for q in codebooks(tr2.model))
    assert tr2.load_checkpoint(str(path)) == 2 and tr2.iteration == 2
    for k, v in tr2.model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(q.initialized for q in codebooks(tr2.model))
    assert torch.equal(tr2.engine.exp_avg, tr.engine.exp_avg) and torch.equal(tr2.engine.exp_avg_sq, tr.engine.exp_avg_sq)
    # the two trainers continue alike
    reseed(11)
    _, d1 = tr.train_step((x, y))
    reseed(11)
    _, d2 = tr2.train_step((x, y))
    assert d1 == d2
    for (k, a), b in zip(tr.model.state_dict().items(), tr2.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_trainer_refuses_data_parallel_engine():
    meta, arr = fixture("vq2a", "single_ema")
    m = build_model(meta, arr)
    with pytest.raises(NotImplementedError, match="data parallel"):
        m.engine().attach_comm(object())


def test_reference_trainer_loop_runs():
    meta, arr = fixture("vq2a", "ema_gst")
    m = build_model(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    totals = []
    for _ in range(2):
        opt.zero_grad()
        _, loss, detail = m((x, y))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10)
        opt.step()
        totals.append(detail["Total"])
        assert all(np.isfinite(v) for v in detail.values())
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert all(bool(torch.isfinite(b).all()) for b in m.buffers())
    assert totals[0] != totals[1]
