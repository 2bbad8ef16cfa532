"""`vqvae2.Model` on the MI355X against the reference's float64 fixtures
(tests/golden/make_golden_vqvae2_model.py, vqmodel_<case>), the reference
trainer's loop on it, and the configurations that are not built.  Bound as
tests/test_gpu_hier_encoder.py; `mha.linear_k.bias` has a mathematically zero
gradient, so its bound is absolute (tests/test_gpu_gst.py)."""
import numpy as np
import pytest
import torch

from tests.hier_model_ref import MODEL_CASES, ULP16, fixture
from tests.test_gpu_hier_encoder import ratios, report

pytestmark = pytest.mark.gpu


def build_model(meta, arr, **over):
    from vae_npvc_amd.model.vqvae2 import Model
    m = Model(dict(meta["arch"], **over))
    assert list(m.state_dict().keys()) == meta["keys"]
    m.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]})
    return m.cuda()


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_fp32_matches_the_float64_reference(case):
    meta, arr = fixture("vqmodel", case)
    m = build_model(meta, arr)
    x, y = torch.from_numpy(arr["x"].copy()).cuda(), torch.from_numpy(arr["y"].copy()).cuda()
    levels = [i for i in reversed(range(3)) if hasattr(m.quantizers[i], "embeddings")]  # the order they run in
    seen, hooks = {}, []
    for i in levels:
        hooks.append(m.quantizers[i].register_forward_pre_hook(
            lambda mod, inp, i=i: seen.__setitem__(i, inp[0].detach().clone())))
    xhat, loss, detail = m((x, y))
    for h in hooks:
        h.remove()
    assert list(detail) == meta["loss_keys"] and all(isinstance(v, float) for v in detail.values())
    loss.backward()
    # indices of every quantized level, from the forward's launches on the input the level received
    assert meta["gap"] >= 1e-3 and len(levels) == len(meta["gaps64"])
    for k, i in enumerate(levels):
        idx = m.quantizers[i].forward_indices(seen[i])
        assert torch.equal(idx.cpu(), torch.from_numpy(arr[f"idx.{k}"].copy())), (k, i)
    got = {"xhat": xhat.detach()}
    got.update({k: torch.tensor(v) for k, v in detail.items()})
    got.update({k: p.grad for k, p in m.named_parameters()})
    want = {"xhat": arr["xhat"]}
    want.update({k: arr["loss." + k] for k in meta["loss_keys"]})
    want.update({k: arr["grad." + k] for k in meta["params"] if k not in meta["abs32"]})
    report(f"vqmodel {case} fp32", ratios(got, want, meta["err32"]))
    for k, a32 in meta["abs32"].items():  # exactly zero in exact arithmetic
        scale = float(np.abs(arr["grad." + k[:-4] + "weight"]).max())
        assert float(got[k].abs().max()) <= max(8 * a32, ULP16 * scale), k
    assert float(loss.detach()) == detail["Total"]


def test_reference_trainer_loop_runs():
    meta, arr = fixture("vqmodel", "gst")
    m = build_model(meta, arr)
    x, y = torch.from_numpy(arr["x"].copy()).cuda(), torch.from_numpy(arr["y"].copy()).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    totals = []
    for _ in range(2):
        opt.zero_grad()
        _, loss, detail = m((x, y))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10)
        opt.step()
        totals.append(detail["Total"])
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert totals[0] != totals[1] and all(np.isfinite(totals))


def test_unbuilt_configurations_raise():
    from vae_npvc_amd.model.vqvae2 import Model
    meta, arr = fixture("vqmodel", "gst")
    with pytest.raises(NotImplementedError, match="EMAVectorQuantizer.forward"):
        Model(dict(meta["arch"], use_ema=True))
    with pytest.raises(NotImplementedError):
        Model(dict(meta["arch"], jitter_p=0.1))
    m = Model(meta["arch"])
    for f in (m.encode, m.decode, m.infer):
        with pytest.raises(NotImplementedError):
            f(None)
