"""The vqvae2a family without a GPU: the new entry points are declared and in
_SIGS with the ABI still 130; Jitter.draw and the codebook-row helper draw
what the reference draws; vqvae2a.Model's tree equals the fixtures' key lists
(tests/golden/make_golden_vqvae2a.py); the refusals are loud."""
import json
import re

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, ROOT
from tests.hier_model_ref import fixture

NEW = ("vqx_ntc_to_nct_gather", "vqx_nct_to_ntc_keep", "vqx_vq_commit_bwd_g")
MODEL_CASES = ("ema_gst", "plain_shared", "single_ema")


def test_new_symbols_are_declared_and_the_abi_is_130():
    from vae_npvc_amd import _lib as L
    header = (ROOT / "include" / "vqx.h").read_text()
    for fn in NEW:
        assert re.search(rf"\bint {fn}\(", header), fn
        assert fn in L._SIGS and fn in L.EXPORTS, fn
    assert L.ABI_VERSION == 130 and "#define VQX_ABI_VERSION 130" in header


def test_new_symbols_are_exported_and_validate_before_launching():
    from vae_npvc_amd import _lib as L
    lib = L.load()
    one = 16  # a non-null address; validation fails before any launch
    for fn in NEW:
        assert hasattr(lib, fn), fn
    F32 = L.VQX_F32
    # (y, ldy, dtype, B, C, T, src_t, x): null y, null x, T < 1, C < 1, B*T*C >= 2^31, ldy < C, bad dtype
    for args in ((0, 4, F32, 1, 4, 2, 0, one), (one, 4, F32, 1, 4, 2, 0, 0), (one, 4, F32, 1, 4, 0, 0, one),
                 (one, 4, F32, 1, 0, 2, 0, one), (one, 1 << 20, F32, 2, 1 << 20, 1 << 10, 0, one),
                 (one, 3, F32, 1, 4, 2, 0, one), (one, 4, 7, 1, 4, 2, 0, one)):
        assert lib.vqx_ntc_to_nct_gather(*args, None) != 0, args
        assert b"vqx_ntc_to_nct_gather" in lib.vqx_last_error()
    # (g, B, C, T, src_t, y, ldy, dtype)
    for args in ((0, 1, 4, 2, 0, one, 4, F32), (one, 1, 4, 2, 0, 0, 4, F32), (one, 1, 4, 0, 0, one, 4, F32),
                 (one, 1, 0, 2, 0, one, 4, F32), (one, 2, 1 << 20, 1 << 10, 0, one, 1 << 20, F32),
                 (one, 1, 4, 2, 0, one, 3, F32)):
        assert lib.vqx_nct_to_ntc_keep(*args, None) != 0, args
        assert b"vqx_nct_to_ntc_keep" in lib.vqx_last_error()
    # (z, zq, B, D, T, s, g, nct, dz)
    for args in ((0, one, 1, 4, 2, 1.0, 0, 1, one), (one, 0, 1, 4, 2, 1.0, 0, 1, one), (one, one, 1, 4, 2, 1.0, 0, 1, 0),
                 (one, one, 1, 4, 0, 1.0, 0, 0, one), (one, one, 1, 0, 2, 1.0, 0, 0, one),
                 (one, one, 2, 1 << 20, 1 << 10, 1.0, 0, 0, one)):
        assert lib.vqx_vq_commit_bwd_g(*args, None) != 0, args
        assert b"vqx_vq_commit_bwd_g" in lib.vqx_last_error()


# ------------------------------------------------------------------ jitter
def _draw(p, T, seed):
    from vae_npvc_amd.model.layers_vq import Jitter
    jit = Jitter(p).train()
    np.random.seed(seed)
    src = jit.draw(T)
    return src, float(np.random.random_sample())


def test_draw_reproduces_the_recorded_maps_and_consumes_the_same_uniforms():
    for rec in json.load(open(GOLD / "jitter.json")).values():
        src, nxt = _draw(rec["p"], rec["T"], rec["seed"])
        assert src.dtype == np.int32 and src.tolist() == rec["src"]
        assert nxt == rec["next_uniform"]
    for case in ("jitter", "plain_jitter"):
        meta, arr = fixture("vqjit", case)
        src, nxt = _draw(meta["p"], meta["T"], meta["run_seed"])
        assert src.tolist() == arr["map"].tolist() and nxt == meta["next_uniform"], case
        moved = arr["map"] != np.arange(meta["T"])
        assert moved.any() and not moved.all()


def test_draw_returns_none_without_jitter_and_refuses_one_frame():
    from vae_npvc_amd.model.layers_vq import Jitter
    np.random.seed(3)
    want = float(np.random.random_sample())
    np.random.seed(3)
    assert Jitter(0.12).eval().draw(8) is None and Jitter(0.0).train().draw(8) is None
    assert Jitter(0.0).train().draw(1) is None
    assert float(np.random.random_sample()) == want  # nothing was drawn
    with pytest.raises(ValueError, match="one frame"):
        Jitter(0.12).train().draw(1)
    assert Jitter(0.12).train().draw(2).tolist() in ([0, 1], [1, 1], [0, 0], [1, 0])
    x = torch.zeros(1, 4, 3)
    assert Jitter(0.12).eval()(x) is x


# ------------------------------------------------------------------ codebook rows
@pytest.mark.parametrize("case", ["init_k16", "tile_k64"])
def test_code_rows_are_the_reference_codebook(case):
    """init_emb's codebook of step 1 from the stored z under the stored seed: z[perm] exactly, or the tiled noisy
    rows within float32 rounding of the float64 run's (which adds the same float32 noise in float64)."""
    from vae_npvc_amd.model.layers_vq import draw_code_rows
    meta, arr = fixture("vqema", case)
    K, D = meta["K"], meta["D"]
    zf = torch.from_numpy(arr["s1.z"].copy()).transpose(1, 2).reshape(-1, D)
    torch.manual_seed(meta["run_seed"])
    perm, rows = draw_code_rows(zf, K)
    want = arr["s1.codebook"]
    if zf.shape[0] >= K:
        assert rows is None and perm.dtype == torch.int32 and tuple(perm.shape) == (K,)
        assert np.array_equal(zf[perm.long()].double().numpy(), want)
    else:
        assert perm is None and rows.dtype == torch.float32 and tuple(rows.shape) == (K, D)
        assert np.abs(rows.double().numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max()


# ------------------------------------------------------------------ model
def _model(meta):
    from vae_npvc_amd.model.vqvae2a import Model
    return Model(meta["arch"])


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_tree_is_the_reference_tree(case):
    meta, arr = fixture("vq2a", case)
    m = _model(meta)
    assert list(m.state_dict().keys()) == meta["keys"]
    assert [k for k, _ in m.named_parameters()] == meta["params"]
    assert [k for k, _ in m.named_buffers()] == meta["buffers"]
    m.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, strict=True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), arr["param." + k]), k
    assert meta["gap"] >= 1e-3


def test_refused_configurations_raise_at_construction():
    from vae_npvc_amd.model.vqvae2a import Model
    arch = fixture("vq2a", "plain_shared")[0]["arch"]
    with pytest.raises(NotImplementedError, match="jitter_p"):
        Model(dict(arch, pooling_last=True))  # a pooled quantized top with jitter
    Model(dict(arch, pooling_last=True, jitter_p=0.0))
    with pytest.raises(NotImplementedError, match="resampling"):
        Model(dict(arch, **{"decoder.1": dict(arch["decoder.1"], upsample_scales=[2])}))
    with pytest.raises(NotImplementedError, match="shared"):
        Model(dict(arch, use_gst=True))
    with pytest.raises(ValueError, match="compute_dtype"):
        Model(dict(arch, compute_dtype="fp16"))
    with pytest.raises(ValueError, match="levels"):
        Model(dict(arch, levels=4))
    gst = fixture("vq2a", "ema_gst")[0]["arch"]
    assert Model(dict(gst, levels=1)).use_gst is False  # forced off at one level
    assert Model(gst).pooling_last is True


def test_cpu_inputs_and_undefined_methods_raise():
    from vae_npvc_amd._lib import VqxError
    from vae_npvc_amd.model.layers_vq import EMAVectorQuantizer, Jitter, VectorQuantizer
    meta, arr = fixture("vq2a", "single_ema")
    m = _model(meta)
    x, y = torch.from_numpy(arr["x"].copy()), torch.from_numpy(arr["y"].copy())
    for f in (lambda: m((x, y)), lambda: m.encode(x), lambda: m.convert((x, y))):
        with pytest.raises(VqxError):
            f()
    z = torch.zeros(2, 64, 4)
    with pytest.raises(VqxError):
        EMAVectorQuantizer(16, 64, 0.9)(z)
    with pytest.raises(VqxError):
        VectorQuantizer(16, 64)(z, src_t=np.arange(4, dtype=np.int32))
    np.random.seed(0)
    with pytest.raises(VqxError):
        Jitter(0.12).train()(z)
    for f in (m.decode, m.infer):
        with pytest.raises(NotImplementedError, match="undefined"):
            f(None)
    with pytest.raises(NotImplementedError, match="z_dim"):
        EMAVectorQuantizer(16, 32, 0.9)(torch.zeros(2, 32, 4))
    with pytest.raises(NotImplementedError, match="z_num"):
        EMAVectorQuantizer(24, 64, 0.9)(z)
    with pytest.raises(NotImplementedError, match="z_num"):
        EMAVectorQuantizer(4096, 64, 0.9)(z)
    q = EMAVectorQuantizer(16, 64, 0.9)
    q.quantize = False
    assert q(z)[0] is z
