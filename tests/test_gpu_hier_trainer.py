"""This package's Trainer on the hierarchical model (`model_type:
vae_npvc_amd.model.vqvae2`, engine/autograd_step.py) on the MI355X:

1  against the reference's training steps in float64 (tests/golden/
   make_golden_vqvae2_train.py, vqtrain_<case>): loss dicts, pre-clip gradient
   norms (bound as tests/test_gpu_hier_model.py: error <= max(8 err32, 16 ulp)
   per quantity) and the indices of every forward;
2  against the reference recipe's loop (torch.optim.Adam, clip_grad_norm_,
   StepLR) on the same HIP model, fp32 and bf16, after one step: loss dicts
   equal, parameters and moments to 1e-6 norm-relative (tests/test_gpu_optim.py's
   measure and bound for the same kind of comparison).  Not after a second
   step: gradient elements at rounding-noise level (mha.linear_k.bias,
   mathematically zero) make Adam's sign-like update ill-conditioned once the
   two runs' parameters differ in the last bit;
3  checkpoints; 4  valid_step; 5  the flat views, and RAdam.

Config = the fixture's arch + the fixture generator's trainer keys.  Runs on
the MI355X only (-m gpu)."""
import json

import pytest
import torch

from tests.helpers import GOLD
from tests.hier_model_ref import MODEL_CASES, fixture
from tests.test_gpu_hier_encoder import ratios, report
from tests.test_gpu_optim import relerr

pytestmark = pytest.mark.gpu

BETAS = (0.5, 0.999)
_train = {}


def train_fixture(case):
    """(meta, arrays) of tests/golden/vqtrain_<case>; loaded once, read-only."""
    if case not in _train:
        import numpy as np
        meta = json.load(open(GOLD / f"vqtrain_{case}.json"))
        arr = dict(np.load(GOLD / meta["files"][0], allow_pickle=False))
        for v in arr.values():
            v.setflags(write=False)
        _train[case] = (meta, arr)
    return _train[case]


def config(case, **over):
    meta, _ = fixture("vqmodel", case)
    tmeta, _ = train_fixture(case)
    cfg = dict(meta["arch"], **tmeta["train"])
    cfg.update(model_type="vae_npvc_amd.model.vqvae2", trainer_type="vae_npvc_amd.trainer.basic")
    cfg.update(over)
    return cfg


def state_dict(case):
    meta, arr = fixture("vqmodel", case)
    return {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}


def batch(case):
    _, arr = fixture("vqmodel", case)
    return torch.from_numpy(arr["x"].copy()).cuda(), torch.from_numpy(arr["y"].copy()).cuda()


def make_trainer(case, **over):
    from vae_npvc_amd.trainer.basic import Trainer
    tr = Trainer(config(case, **over))
    tr.model.load_state_dict(state_dict(case))
    assert tr.engine.params_intact()
    return tr


def make_model(case, **over):
    from vae_npvc_amd.model.vqvae2 import Model
    m = Model(config(case, **over)).cuda()
    m.load_state_dict(state_dict(case))
    return m.train()


def quantized_levels(model):
    return [i for i in reversed(range(model.levels)) if hasattr(model.quantizers[i], "embeddings")]  # run order


def record_indices(model, sink):
    """Each quantized level appends the indices of the input it receives to
    sink[level], from the forward's own launches; the codebook parameter, which
    those renormalise in place, gets its bits back before the forward proper."""
    hooks = []
    for i in quantized_levels(model):
        def pre(mod, inp, i=i):
            E = mod.embeddings.detach().clone()
            sink.setdefault(i, []).append(mod.forward_indices(inp[0].detach()).cpu())
            with torch.no_grad():
                mod.embeddings.copy_(E)
        hooks.append(model.quantizers[i].register_forward_pre_hook(pre))
    return hooks


@pytest.mark.parametrize("case", MODEL_CASES)
def test_train_steps_match_the_float64_reference(case):
    tmeta, tarr = train_fixture(case)
    assert tmeta["min_gap"] >= 2e-4 and min(min(g) for g in tmeta["gaps32"] + tmeta["gaps64"]) >= tmeta["min_gap"]
    assert min(tmeta["norms64"]) > tmeta["train"]["max_grad_norm"]  # the clip is active in every step
    tr = make_trainer(case)
    x, y = batch(case)
    ids = {}
    hooks = record_indices(tr.model, ids)
    got, want = {}, {}
    for s in range(tmeta["forwards"]):
        it, detail = tr.train_step((x, y))
        assert it == s + 1 and list(detail) == tmeta["loss_keys"]
        assert all(isinstance(v, float) for v in detail.values())
        for k, v in detail.items():
            got[f"{s}.{k}"] = torch.tensor(v, dtype=torch.float64)
            want[f"{s}.{k}"] = tarr[f"loss.{s}.{k}"]
        got[f"{s}.norm"] = tr.engine.sumsq.sqrt().reshape(())
        want[f"{s}.norm"] = tarr[f"norm.{s}"]
    for h in hooks:
        h.remove()
    levels = quantized_levels(tr.model)
    assert len(levels) == tmeta["levels"]
    for s in range(tmeta["forwards"]):
        for k, i in enumerate(levels):
            assert torch.equal(ids[i][s], torch.from_numpy(tarr[f"idx.{s}.{k}"].copy())), (s, k, i)
    report(f"vqtrain {case} fp32", ratios(got, want, tmeta["err32"]))
    assert int(tr.engine.opt_step) == tmeta["forwards"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_first_step_equals_the_reference_recipes_loop(dtype):
    case = "gst"
    tr = make_trainer(case, compute_dtype=dtype)
    m = make_model(case, compute_dtype=dtype)
    x, y = batch(case)
    cfg = config(case)
    opt = torch.optim.Adam(m.parameters(), lr=cfg["learning_rate"], betas=BETAS, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.StepLR(optimizer=opt, **cfg["lr_param"])
    _, d_tr = tr.train_step((x, y))
    m.zero_grad()
    _, loss, d_ref = m((x, y))
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), cfg["max_grad_norm"])
    opt.step()
    sched.step()
    assert d_tr == d_ref  # the same launches on the same bits
    assert float(norm) > cfg["max_grad_norm"]
    assert abs(float(tr.engine.sumsq.sqrt()) - float(norm)) <= 1e-6 * float(norm)
    e = tr.engine
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    names = [k for k, _ in tr.model.named_parameters()]
    for name, p_tr, p_ref, off in zip(names, e.params, m.parameters(), e._p_off):
        n = p_tr.numel()
        st = opt.state.get(p_ref, {})
        pairs = {"p": (p_tr.detach(), p_ref.detach()),
                 "m": (e.exp_avg[off:off + n].view_as(p_tr), st.get("exp_avg", torch.zeros_like(p_ref))),
                 "v": (e.exp_avg_sq[off:off + n].view_as(p_tr), st.get("exp_avg_sq", torch.zeros_like(p_ref)))}
        for k, (a, b) in pairs.items():
            err = relerr(a, b)
            worst[k] = max(worst[k], err)
            assert err < 1e-6, (name, k, err)
    print(f"trainer vs torch loop ({dtype}) worst p/m/v relative error:", worst)


def test_checkpoint_round_trip(tmp_path):
    from vae_npvc_amd.model.vqvae2 import Model
    from vae_npvc_amd.trainer.basic import Trainer
    case = "gst"
    tr = make_trainer(case)
    x, y = batch(case)
    for _ in range(2):
        tr.train_step((x, y))
    path = tmp_path / "ckpt.pt"
    tr.save_checkpoint(path)
    fresh = Trainer(config(case))
    assert fresh.load_checkpoint(path) == 2 and fresh.iteration == 2
    assert int(fresh.engine.opt_step) == 2 and fresh.engine.params_intact()
    keep = Trainer(config(case, reference_resume_counter=True))
    assert keep.load_checkpoint(path) == 2 and keep.iteration == 0
    assert keep.train_step((x, y))[0] == 1
    # the optimizer entry is torch.optim.Adam's, indexed in model.parameters() order
    data = torch.load(path, map_location="cpu", weights_only=True)
    other = Model(config(case))
    opt = torch.optim.Adam(other.parameters(), lr=1e-3, betas=BETAS)
    opt.load_state_dict(data["optimizer"])
    e = tr.engine
    for p, q, off in zip(other.parameters(), e.params, e._p_off):
        if p in opt.state:
            assert opt.state[p]["exp_avg"].shape == p.shape
            assert torch.equal(opt.state[p]["exp_avg"], e.exp_avg[off:off + q.numel()].view_as(q).cpu())
    assert data["optimizer"]["param_groups"][0]["lr"] == 1e-3 * 0.5 ** 2  # StepLR(1, 0.5) after two steps
    it_a, _ = tr.train_step((x, y))
    it_b, _ = fresh.train_step((x, y))
    assert it_a == it_b == 3
    for (name, a), b in zip(tr.model.named_parameters(), fresh.model.parameters()):
        assert relerr(a.detach(), b.detach()) < 1e-6, name


def test_valid_step_leaves_the_parameters_alone():
    case = "plain_top"
    tr = make_trainer(case)
    x, y = batch(case)
    _, d_train = tr.train_step((x, y))  # (so that the codebooks are no longer normalised)
    before = tr.engine.flat_p.clone()
    moments = tr.engine.exp_avg.clone(), tr.engine.exp_avg_sq.clone()
    d = tr.valid_step((x, y))
    assert list(d) == list(d_train) and all(isinstance(v, float) for v in d.values())
    assert torch.equal(tr.engine.flat_p, before)
    assert torch.equal(tr.engine.exp_avg, moments[0]) and torch.equal(tr.engine.exp_avg_sq, moments[1])
    assert tr.model.training and tr.engine.params_intact()
    assert tr.valid([(x, y), (x, y)])["Total"] == [d["Total"]] * 2


def test_flat_views_and_radam():
    from oracle.vqvae_cpu import ORAdam
    case = "gst"
    tr = make_trainer(case)
    x, y = batch(case)
    for _ in range(2):
        tr.train_step((x, y))
    e = tr.engine
    assert e.params_intact()
    lo, hi = e.flat_p.data_ptr(), e.flat_p.data_ptr() + 4 * e.flat_p.numel()
    assert all(lo <= p.data_ptr() and p.data_ptr() + 4 * p.numel() <= hi for p in tr.model.parameters())
    assert sum(p.numel() for p in tr.model.parameters()) == e.flat_p.numel()  # dense, no padding

    ra = make_trainer(case, optim_type="RAdam")
    assert ra.engine.opt_kind == "radam"
    twin = make_model(case)  # the same launches on the same bits: the step's gradients
    _, loss, _ = twin((x, y))
    loss.backward()
    ra.train_step((x, y))
    coef = (torch.tensor(0.5) / (ra.engine.sumsq.cpu().sqrt() + 1e-6)).clamp(max=1.0)
    assert float(coef) < 1.0
    cpu = [p.detach().cpu().clone().requires_grad_(True) for p in twin.parameters()]
    opt = ORAdam(cpu, lr=1e-3, betas=BETAS, eps=1e-8)
    for c, p in zip(cpu, twin.parameters()):
        c.grad = None if p.grad is None else p.grad.cpu() * coef
    opt.step()
    for (name, a), b in zip(ra.model.named_parameters(), cpu):
        assert relerr(a.detach(), b.detach()) < 1e-6, name
    ra.train_step((x, y))
    assert all(bool(torch.isfinite(p).all()) for p in ra.model.parameters())
    assert int(ra.engine.opt_step) == 2
    sd = ra.optimizer.state_dict()
    assert isinstance(sd["state"][0]["step"], int) and "amsgrad" not in sd["param_groups"][0]


def test_data_parallel_is_refused():
    from vae_npvc_amd.model.vqvae2 import Model
    eng = Model(config("gst")).cuda().engine()
    with pytest.raises(NotImplementedError, match="data parallel"):
        eng.attach_comm(object())
