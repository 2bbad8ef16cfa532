"""The hierarchical model without a GPU: the new entry points are declared,
exported and in _SIGS with the ABI still 130; the module trees equal the
fixtures' key lists; and the float64 plain-torch restatement
(tests/hier_model_ref.py) reproduces every fixture of
tests/golden/make_golden_vqvae2_model.py within 1e-10 relative."""
import re

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, ROOT
from tests.hier_model_ref import (ENC_CASES, LEVEL_CASES, MODEL_CASES, embed_norm, fixture, restated_model,
                                  restated_quantizer, run_restated_encoder, tensors)

NEW = ("vqx_nct_to_ntc_lrelu_bwd", "vqx_vq_plain_bwd_g", "vqx_ntc_to_nct_scale")


def close(got, want, what):
    """1e-10 relative; the perplexity ("entropy") within 4 float32 ulp: the reference builds its one-hot
    matrix in float32 whatever z's dtype (layers_vq.py:112), so its float64 run rounds that value to float32."""
    want = np.asarray(want, dtype=np.float64)
    got = got.detach().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, what
    rtol = 4 * 2.0 ** -23 if what.startswith("entropy") else 1e-10
    assert np.abs(got - want).max() <= rtol * max(np.abs(want).max(), 1e-300), what


def test_new_symbols_are_declared_exported_and_the_abi_is_130():
    from vae_npvc_amd import _lib as L
    lib = L.load()
    header = (ROOT / "include" / "vqx.h").read_text()
    for fn in NEW:
        assert re.search(rf"\bint {fn}\(", header), fn
        assert fn in L._SIGS and hasattr(lib, fn), fn
    assert L.ABI_VERSION == 130 and lib.vqx_version() == 130
    assert "#define VQX_ABI_VERSION 130" in header


def test_masked_layout_validation_is_loud():
    from vae_npvc_amd import _lib as L
    lib = L.load()
    one = 16  # a non-null address; validation fails before any launch
    for args in ((0, 1, 1, 1, one, 1, 0, 0.2, one, 1, 0), (one, 0, 1, 1, one, 1, 0, 0.2, one, 1, 0),
                 (one, 1, 4, 1, one, 3, 0, 0.2, one, 4, 0), (one, 1, 1, 1, one, 1, 7, 0.2, one, 1, 0)):
        assert lib.vqx_nct_to_ntc_lrelu_bwd(*args, None) != 0


@pytest.mark.parametrize("case", ENC_CASES)
def test_encoder_tree_and_restatement(case):
    from vae_npvc_amd.model.vqvae2 import Encoder
    meta, arr = fixture("vqenc", case)
    enc = Encoder(**meta["encoder"])
    assert list(enc.state_dict().keys()) == meta["keys"]
    assert [k for k, _ in enc.named_parameters()] == meta["params"]
    sd = {k: arr["param." + k] for k in meta["keys"]}
    got = run_restated_encoder(meta["encoder"], sd, arr["x"], arr.get("dz"), arr.get("dfeat"))
    for k in ("z", "feat", "dx"):
        close(got[k], arr[k], k)
    for k in meta["grads"]:
        close(got[k], arr["grad." + k], k)


@pytest.mark.parametrize("case", LEVEL_CASES)
def test_level_restatement(case):
    meta, arr = fixture("vqlevel", case)
    E = torch.from_numpy(arr["param.embeddings"].copy()).double()
    E = (embed_norm(E) if meta["normalize"] else E).requires_grad_()
    z = torch.from_numpy(arr["z"].copy()).double().requires_grad_()
    z_vq, qut, enc, perp, idx, gap = restated_quantizer(E, z, meta["normalize"])
    w = meta["loss_weights"]
    ((z_vq * torch.from_numpy(arr["go"].copy()).double()).sum() + w[0] * qut + w[1] * enc).backward()
    assert np.array_equal(idx.numpy(), arr["idx"]) and abs(gap - meta["gap64"]) <= 1e-9 and meta["gap"] >= 1e-3
    for k, v in (("z_vq", z_vq), ("z_qut_loss", qut), ("z_enc_loss", enc), ("entropy", perp), ("dz", z.grad),
                 ("dE", E.grad)):
        close(v, arr[k], k)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_tree_and_restatement(case):
    from vae_npvc_amd.model.vqvae2 import Model
    meta, arr = fixture("vqmodel", case)
    m = Model(meta["arch"])
    assert list(m.state_dict().keys()) == meta["keys"]
    assert [k for k, _ in m.named_parameters()] == meta["params"]
    assert [n for n, _ in m.named_children()] == ["encoders", "quantizers", "decoders", "embeds", "jitter"]
    params = tensors(arr, meta["keys"], "param.", torch.float64, grad=False)
    for k in params:
        if k.endswith(".embeddings") and meta["arch"]["quantizer." + k.split(".")[1]].get("normalize"):
            params[k] = embed_norm(params[k])
    params = {k: v.requires_grad_() for k, v in params.items()}
    x, y = torch.from_numpy(arr["x"].copy()).double(), torch.from_numpy(arr["y"].copy())
    xhat, loss, detail, ids, gaps = restated_model(meta["arch"], params, x, y)
    loss.backward()
    assert list(detail) == meta["loss_keys"]
    close(xhat, arr["xhat"], "xhat")
    for k in meta["loss_keys"]:
        close(detail[k], arr["loss." + k], k)
    for k, idx in enumerate(ids):
        assert np.array_equal(idx.numpy(), arr[f"idx.{k}"])
    for k in meta["params"]:
        if k not in meta["abs32"]:
            close(params[k].grad, arr["grad." + k], k)


def test_new_fixtures_stay_below_the_committed_file_limit():
    files = list(GOLD.glob("vqenc_*")) + list(GOLD.glob("vqlevel_*")) + list(GOLD.glob("vqmodel_*"))
    names = {f.name for f in files}
    for kind, cases in (("vqenc", ENC_CASES), ("vqlevel", LEVEL_CASES), ("vqmodel", MODEL_CASES)):
        for case in cases:
            assert {f"{kind}_{case}.json", f"{kind}_{case}.npz"} <= names, (kind, case)
            assert set(fixture(kind, case)[0]["files"]) <= names
    for f in files:
        assert f.stat().st_size < 1 << 20, f.name
