"""The self-attention layer without a GPU: the fixtures of make_golden_attn.py
load and carry the reference's own error for every tensor; the C ABI declares
and exports vqx_attn_*, AttnArgs has gcc's layout of vqx_attn_args, the
envelope is validated before any launch; SelfAttention has the reference's
parameter tree under `mha.` and refuses what is not built; vqvae2a.Model keeps
its tree without `attention.{i}` and appends `attentions` with it."""
import ctypes
import math
import re

import pytest
import torch

from tests.attn_ref import CASES, KB, TENSORS, fixture
from tests.helpers import GOLD, ROOT
from tests.hier_model_ref import fixture as model_fixture
from tests.test_gst_host import _c_layout

HEADER = ROOT / "include" / "vqx.h"
ATTN_FUNCTIONS = ("vqx_attn_workspace", "vqx_attn_fwd", "vqx_attn_bwd")
MHA_KEYS = [f"linear_{n}.{p}" for n in ("q", "k", "v", "out") for p in ("weight", "bias")]


def _lib():
    from vae_npvc_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("case", CASES)
def test_fixture_loads_with_the_reference_errors_for_every_tensor(case):
    meta, arr = fixture(case)
    B, F, T = meta["B"], meta["F"], meta["T"]
    for k in ("x", "go", "out", "dx"):
        assert arr[k].shape == (B, F, T), k
    assert arr["out"].dtype == arr["dx"].dtype == "float64" and arr["x"].dtype == "float32"
    assert meta["keys"] == MHA_KEYS
    for k in MHA_KEYS:
        assert arr["param." + k].dtype == "float32" and arr["grad." + k].dtype == "float64"
        assert arr["param." + k].shape == arr["grad." + k].shape
    for t in TENSORS:
        assert math.isfinite(meta["err32"][t]) and math.isfinite(meta["l2_bf16"][t]), t
        zero = t in meta["zero_ref"]
        assert (meta["err32"][t] == 0) == zero or t in ("out", "dx"), t
        if not zero:
            assert 0 < meta["err32"][t] < 1e-4 and 0 < meta["l2_bf16"][t] < 0.1, t
    for k in [KB] + meta["zero_ref"]:
        assert meta["abs32"][k] >= 0 and meta["abs_bf16"][k] >= 0
        assert not arr["grad." + k].any() or k == KB
    if meta["lengths"] is not None:
        assert len(meta["lengths"]) == B
        for b, n in enumerate(meta["lengths"]):
            assert 1 <= n <= T
            assert not arr["go"][b, :, n:].any() and not arr["out"][b, :, n:].any() and not arr["dx"][b, :, n:].any()


def test_peaked_case_moves_the_row_maximum_in_a_later_tile():
    meta, _ = fixture("peaked")
    assert meta["attn_max"] > 0.9 and meta["argmax_from_128"] >= 0.25


def test_fixtures_stay_below_the_committed_file_limit():
    files = sorted(GOLD.glob("attn_*")) + sorted(GOLD.glob("vq2a_attn_*"))
    assert len(files) >= 2 * len(CASES)
    assert max(f.stat().st_size for f in files) < (1 << 20)


# ------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_attention_entry_points():
    L, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(vqx_\w+)\s*\(", text, flags=re.M))
    for f in ATTN_FUNCTIONS:
        assert f in declared and hasattr(lib, f) and f in L._SIGS and f in L.EXPORTS, f
    assert "vqx_attn_args" in text
    assert L.ABI_VERSION == 130 and "#define VQX_ABI_VERSION 130" in HEADER.read_text()  # additive


def test_attn_args_layout_matches_header():
    L, _ = _lib()
    names = [f[0] for f in L.AttnArgs._fields_]
    got = _c_layout("vqx_attn_args", names)
    assert got[0] == ctypes.sizeof(L.AttnArgs)
    assert got[1:] == [getattr(L.AttnArgs, n).offset for n in names]


def _valid_args(L):
    a = L.AttnArgs()
    for name in ("qkv", "ctx", "lse", "d_ctx", "d_qkv", "ws"):
        setattr(a, name, 0x1000)
    a.B, a.T, a.F, a.H, a.ldqkv, a.ldc, a.dtype = 2, 77, 128, 4, 384, 128, L.VQX_BF16
    return a


@pytest.mark.parametrize("fn", ["vqx_attn_fwd", "vqx_attn_bwd"])
def test_attention_validation_errors_are_loud(fn):
    """Bad arguments return non-zero with a message; nothing is launched."""
    L, lib = _lib()
    f = getattr(lib, fn)
    assert f(None, None) != 0
    assert b"null args" in lib.vqx_last_error()
    for field, value, word in (("H", 3, b"multiple of H"), ("H", 1, b"d_k"), ("H", 8, b"d_k"), ("dtype", 2, b"dtype"),
                               ("T", 0, b">= 1"), ("B", 1 << 30, b"2^31"), ("ldqkv", 383, b"ldqkv"),
                               ("ldqkv", 388, b"16-byte"), ("ldc", 120, b"ldc"), ("qkv", None, b"null pointer"),
                               ("ctx", 0x1008, b"aligned"), ("lse", None, b"null pointer")):
        a = _valid_args(L)
        setattr(a, field, value)
        assert f(ctypes.byref(a), None) != 0, field
        err = lib.vqx_last_error()
        assert fn.encode() in err and word in err, (field, err)
    for lens, word in (([77, 0], b"item 1"), ([78, 5], b"item 0")):  # every item, before the first launch
        a = _valid_args(L)
        arr = (ctypes.c_int32 * 2)(*lens)
        a.len = ctypes.cast(arr, ctypes.c_void_p)
        assert f(ctypes.byref(a), None) != 0
        assert word in lib.vqx_last_error()
    if fn == "vqx_attn_bwd":
        a = _valid_args(L)
        a.ws = None
        assert f(ctypes.byref(a), None) != 0 and b"null pointer" in lib.vqx_last_error()


def test_attention_workspace():
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd import ops
    assert ops.attn_workspace(2, 77, 128, 4, torch.float32) >= 2 * 4 * 77
    assert ops.attn_workspace(96, 256, 128, 4, torch.bfloat16) > ops.attn_workspace(2, 77, 128, 4, torch.bfloat16)
    with pytest.raises(L.VqxError, match="d_k"):
        ops.attn_workspace(2, 77, 128, 8, torch.float32)  # d_k 16
    with pytest.raises(L.VqxError, match="d_k"):
        ops.attn_workspace(2, 77, 128, 1, torch.float32)  # d_k 128
    with pytest.raises(L.VqxError):
        ops.attn_workspace(2, 77, 128, 4, torch.float16)


# ------------------------------------------------------------------ module
def test_module_has_the_reference_parameter_tree():
    from vae_npvc_amd.model.layers_attn import SelfAttention
    from vae_npvc_amd.model.layers_gst import MultiHeadedAttention
    meta, arr = fixture("one_tile")
    layer = SelfAttention(meta["F"], meta["H"])
    assert isinstance(layer.mha, MultiHeadedAttention)
    assert list(layer.state_dict().keys()) == ["mha." + k for k in meta["keys"]]
    sd = {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}
    layer.mha.load_state_dict(sd, strict=True)  # a reference MultiHeadedAttention state_dict, unchanged
    assert torch.equal(layer.mha.linear_out.weight.detach(), sd["linear_out.weight"])
    # initialisation draws the reference's numbers in its order: the fixture's parameters under its seed
    torch.manual_seed(meta["seed"])
    fresh = SelfAttention(meta["F"], meta["H"])
    for k in meta["keys"]:
        assert torch.equal(fresh.mha.state_dict()[k], sd[k]), k


def test_refusals_at_construction():
    from vae_npvc_amd.model.layers_attn import SelfAttention
    with pytest.raises(NotImplementedError, match="dropout"):
        SelfAttention(128, 4, dropout_rate=0.1)
    with pytest.raises(ValueError, match="multiple"):
        SelfAttention(128, 3)
    for n_feat, n_head in ((128, 1), (128, 8), (96, 2), (256, 2)):  # d_k 128, 16, 48, 128
        with pytest.raises(NotImplementedError, match="d_k"):
            SelfAttention(n_feat, n_head)
    with pytest.raises(ValueError, match="compute_dtype"):
        SelfAttention(128, 4, compute_dtype="fp16")
    for n_feat, n_head in ((128, 4), (128, 2), (64, 2), (64, 1), (256, 4)):
        SelfAttention(n_feat, n_head, compute_dtype="bf16")


def test_cpu_input_raises_and_bad_lengths_raise_first():
    """No CPU fallback; lengths are host values checked before the device is touched."""
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd.model.layers_attn import SelfAttention
    layer = SelfAttention(128, 4)
    x = torch.randn(2, 128, 8)
    with pytest.raises(L.VqxError):
        layer(x)
    with pytest.raises(L.VqxError):
        layer(x, lengths=[8, 3], residual=True)
    with pytest.raises(L.VqxError):
        layer.forward_rows(torch.randn(16, 128), 2, 8)
    for bad in ([8, 0], [9, 1], [8], [8, 2, 2], [8.0, 2], torch.tensor([8.0, 2.0]), []):
        with pytest.raises(ValueError):
            layer(x, lengths=bad)
        with pytest.raises(ValueError):
            layer.forward_rows(torch.randn(16, 128), 2, 8, lengths=bad)
    with pytest.raises(ValueError):
        layer(torch.randn(2, 64, 8))
    with pytest.raises(ValueError):
        layer.forward_rows(torch.randn(16, 64), 2, 8)


# ------------------------------------------------------------------ recipe key
@pytest.mark.parametrize("case", ["ema_gst", "plain_shared", "single_ema"])
def test_model_tree_without_and_with_the_key(case):
    from vae_npvc_amd.model.vqvae2a import Model
    meta, _ = model_fixture("vq2a", case)
    arch = meta["arch"]
    plain = Model(arch)
    assert list(plain.state_dict().keys()) == meta["keys"] and not hasattr(plain, "attentions")
    assert [k for k, _ in plain.named_parameters()] == meta["params"]
    torch.manual_seed(5)
    want = {k: v.clone() for k, v in Model(arch).state_dict().items()}
    torch.manual_seed(5)
    m = Model(dict(arch, **{"attention.0": {"n_head": 2}}))
    keys = list(m.state_dict().keys())
    new = [f"attentions.0.mha.linear_{n}.{p}" for n in ("q", "k", "v", "out") for p in ("weight", "bias")]
    assert keys == meta["keys"] + new
    assert [k for k, _ in m.named_parameters()] == meta["params"] + new
    assert [k for k, _ in m.named_buffers()] == meta["buffers"]
    for k, v in want.items():  # the existing modules draw what they drew without the key
        assert torch.equal(m.state_dict()[k], v), k
    assert m.attentions["0"].n_feat == arch["encoder.0"]["z_channels"] and m.attentions["0"].n_head == 2


def test_model_key_per_level_and_refusals():
    from vae_npvc_amd.model.vqvae2a import Model
    arch = model_fixture("vq2a", "ema_gst")[0]["arch"]
    m = Model(dict(arch, compute_dtype="bf16", **{"attention.0": {"n_head": 2}, "attention.2": {"n_head": 1}}))
    assert sorted(m.attentions.keys()) == ["0", "2"]
    assert m.attentions["2"].compute_dtype == "bf16" and m.attentions["2"].mha.d_k == 64
    assert m._attention(1) is None
    z = torch.zeros(1, 64, 4)
    assert m._attend(1, z) is z and m._attend_rows(1, z, 1, 4, [4]) is z
    with pytest.raises(NotImplementedError, match="d_k"):
        Model(dict(arch, **{"attention.1": {"n_head": 4}}))  # z_channels 64 / 4
    with pytest.raises(NotImplementedError, match="dropout"):
        Model(dict(arch, **{"attention.1": {"n_head": 2, "dropout_rate": 0.1}}))
    with pytest.raises(ValueError, match="n_head"):
        Model(dict(arch, **{"attention.1": {"heads": 2}}))
    with pytest.raises(ValueError, match="level"):
        Model(dict(arch, **{"attention.3": {"n_head": 2}}))


def test_other_hier_models_keep_the_identity_hooks():
    from vae_npvc_amd.model.hier_base import HierModelBase
    base = HierModelBase()
    z = torch.zeros(1, 64, 4)
    assert base._attend(0, z) is z and base._attend_rows(0, z, 1, 4, [4]) is z
