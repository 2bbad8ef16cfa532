"""The hierarchical decoder without a GPU: the `upsample` index map and the
conditioning-rate chooser against the reference's recorded behaviour, the
module tree against the fixtures' key lists, the C-ABI validation of
vqx_upsample_cat_* and vqx_conv_args.rowbias_T (no launch, no device), and
the float64 plain-torch restatement of the decoder (tests/hier_ref.py)
against every fixture of tests/golden/make_golden_vqvae2_dec.py."""
import ctypes
import json
import re

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, ROOT
from tests.hier_ref import CASES, expected, fixture, fixture_cond, run_restated
from tests.test_gst_host import _c_layout

HEADER = ROOT / "include" / "vqx.h"
FUNCTIONS = ("vqx_upsample_cat_fwd", "vqx_upsample_cat_bwd")


def _lib():
    from vae_npvc_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------ host logic
def test_index_map_equals_the_reference_upsample():
    from vae_npvc_amd.model.vqvae2 import src_index
    pairs = json.load(open(GOLD / "vqdec_index_maps.json"))["pairs"]
    assert {(p["T"], p["T_l"]) for p in pairs} == {(20, 3), (256, 64), (256, 1), (7, 7), (9, 2), (128, 3), (20, 8),
                                                   (256, 5)}
    for p in pairs:
        assert src_index(p["T"], p["T_l"]) == p["src"], (p["T"], p["T_l"])
    with pytest.raises(ValueError):
        src_index(4, 5)  # nothing is ever cropped


def test_conditioning_rate_chooser():
    from vae_npvc_amd.model.vqvae2 import choose_tc, src_index
    assert choose_tc(256, (1, 64)) == 64
    assert choose_tc(24, (1, 6)) == 6
    assert choose_tc(20, (1, 3)) == 3
    assert src_index(20, 3)[18:] == [2, 2]  # frames 18 and 19 sit in the last segment
    assert choose_tc(20, (3, 8)) == 20  # frame 4: level 0 directly, level 1 through 8 frames
    assert src_index(20, 3)[4] == 0 and src_index(8, 3)[src_index(20, 8)[4]] == 1
    assert choose_tc(20, (20,)) == 20 and choose_tc(16, (1,)) == 1


@pytest.mark.parametrize("case", CASES)
def test_module_tree_equals_the_reference(case):
    from vae_npvc_amd.model.vqvae2 import Decoder
    meta, arr = fixture(case)
    dec = Decoder(**meta["decoder"])
    assert list(dec.state_dict().keys()) == meta["keys"]
    assert [k for k, _ in dec.named_parameters()] == meta["params"]
    dec.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, strict=True)
    assert Decoder(**meta["decoder"], compute_dtype="bf16").compute_dtype == "bf16"


def test_unbuilt_configurations_raise():
    from vae_npvc_amd.model.vqvae2 import Decoder
    meta, _ = fixture("tail")
    with pytest.raises(NotImplementedError):
        Decoder(**dict(meta["decoder"], upsample_scales=[2]))
    with pytest.raises(ValueError):
        Decoder(**meta["decoder"], compute_dtype="fp16")


def test_cpu_input_raises():
    """No CPU fallback: the HIP kernels are the only implementation."""
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd.model.vqvae2 import Decoder, upsample
    meta, arr = fixture("tail")
    dec = Decoder(**meta["decoder"])
    x = torch.from_numpy(arr["x"].copy())
    with pytest.raises(L.VqxError):
        dec((x, [torch.from_numpy(c.copy()) for c in fixture_cond(meta, arr)]))
    with pytest.raises(L.VqxError):
        upsample(torch.randn(2, 8, 3), 20)
    with pytest.raises(ValueError):
        dec((x, [torch.randn(2, 8, 1)]))  # 8 channels, cond_channels is 24


def test_fixtures_stay_below_the_committed_file_limit():
    files = sorted(GOLD.glob("vqdec_*"))
    assert len(files) == 2 * len(CASES) + 1
    assert max(f.stat().st_size for f in files) < (1 << 20)


# ------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_entry_points():
    L, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(vqx_\w+)\s*\(", text, flags=re.M))
    for f in FUNCTIONS:
        assert f in declared and hasattr(lib, f) and f in L._SIGS, f
    assert "vqx_hier_level" in text and "rowbias_T" in text
    assert lib.vqx_version() == 130 == L.ABI_VERSION


def test_hier_level_layout_matches_header():
    L, _ = _lib()
    names = [f[0] for f in L.HierLevel._fields_]
    got = _c_layout("vqx_hier_level", names)
    assert got[0] == ctypes.sizeof(L.HierLevel)
    assert got[1:] == [getattr(L.HierLevel, n).offset for n in names]
    # rowbias_T is the last field of vqx_conv_args (appended: earlier offsets keep)
    assert L.ConvArgs._fields_[-1][0] == "rowbias_T"
    size, off = _c_layout("vqx_conv_args", ["rowbias_T"])
    assert off == L.ConvArgs.rowbias_T.offset and size == ctypes.sizeof(L.ConvArgs)


def _levels(L, n=2, T_l=(1, 3), C=(8, 16)):
    arr = (L.HierLevel * n)()
    for i in range(n):
        arr[i].z, arr[i].T_l, arr[i].C, arr[i].ld = 0x1000, T_l[i % len(T_l)], C[i % len(C)], C[i % len(C)]
    return arr


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_upsample_cat_validation_errors_are_loud(fn):
    """Bad arguments return -1 with a message; nothing is launched (dummy pointers)."""
    L, lib = _lib()
    f = getattr(lib, fn)
    B, T, ldo = 2, 20, 24

    def err(levels, n, B=B, T=T, out=0x2000, ldo=ldo, dtype=L.VQX_F32):
        assert f(levels, n, B, T, out, ldo, dtype, None) == -1
        msg = lib.vqx_last_error()
        assert fn.encode() in msg, msg
        return msg

    assert b"null levels" in err(None, 2)
    assert b"n_levels = 9" in err(_levels(L, 9), 9, ldo=512)
    assert b"n_levels = 0" in err(_levels(L), 0)
    lv = _levels(L)
    lv[1].T_l = 21
    assert b"T_l = 21 not in 1..T = 20" in err(lv, 2)
    lv = _levels(L)
    lv[0].T_l = 0
    assert b"T_l = 0" in err(lv, 2)
    lv = _levels(L)
    lv[1].z = None
    assert b"level 1: null" in err(lv, 2)
    assert b"full-rate pointer" in err(_levels(L), 2, out=None)
    assert b"full-rate pointer" in err(_levels(L), 2, out=0x2004)  # not 16-B aligned
    assert b"bad dtype" in err(_levels(L), 2, dtype=2)
    lv = _levels(L)
    lv[0].C = 6
    assert b"multiples of 4" in err(lv, 2)
    lv = _levels(L)
    lv[0].ld = 4
    assert b"ld >= C" in err(lv, 2)
    assert b"exceeds ldo = 20" in err(_levels(L), 2, ldo=20)
    assert b"B = 0" in err(_levels(L), 2, B=0)
    with pytest.raises(L.VqxError, match="n_levels = 9"):
        L.call(fn, _levels(L, 9), 9, B, T, 0x2000, 512, L.VQX_F32, None)


def _conv_args(L, rowbias_T):
    a = L.ConvArgs()
    a.x, a.w, a.y, a.rowbias = 0x1000, 0x2000, 0x3000, 0x4000
    a.n_rows, a.T, a.cin, a.cout, a.ntaps, a.pad, a.dil = 40, 20, 32, 64, 3, 1, 1
    a.ldx, a.ldy, a.dtype, a.epilogue = 32, 64, L.VQX_F32, L.EPI_ROWBIAS
    a.rowbias_T = rowbias_T
    return a


def test_rowbias_T_validation():
    L, lib = _lib()
    # a segmented row bias is a forward epilogue: the data gradient refuses it ...
    a = _conv_args(L, 3)
    assert lib.vqx_conv1d_dgrad(ctypes.byref(a), None) == -1
    assert b"rowbias_T 3" in lib.vqx_last_error() and b"dgrad" in lib.vqx_last_error()
    # ... alone and inside the fused data + weight gradient call
    w = L.WgradArgs()
    fused = ctypes.c_int32(7)
    assert lib.vqx_conv1d_dgrad_wgrad(ctypes.byref(a), ctypes.byref(w), ctypes.byref(fused), None) == -1
    assert b"rowbias_T 3" in lib.vqx_last_error() and fused.value == 7
    # forward: Tc <= T, and the flag must be set
    a = _conv_args(L, 21)
    assert lib.vqx_conv1d_fwd(ctypes.byref(a), None) == -1
    assert b"rowbias_T 21" in lib.vqx_last_error() and b"<= T 20" in lib.vqx_last_error()
    a = _conv_args(L, 3)
    a.epilogue = 0
    assert lib.vqx_conv1d_fwd(ctypes.byref(a), None) == -1
    assert b"needs ROWBIAS" in lib.vqx_last_error()
    a = _conv_args(L, -1)
    assert lib.vqx_conv1d_fwd(ctypes.byref(a), None) == -1
    assert b"rowbias_T -1" in lib.vqx_last_error()


def test_ops_conv_args_carries_rowbias_T():
    from vae_npvc_amd import ops
    x, w, y = torch.zeros(40, 32), torch.zeros(64, 96), torch.zeros(40, 64)
    rb = torch.zeros(6, 64)
    assert ops.conv_args(x, w, y, T=20, cin=32, cout=64, ntaps=3, pad=1, rowbias=rb).rowbias_T == 0
    a = ops.conv_args(x, w, y, T=20, cin=32, cout=64, ntaps=3, pad=1, rowbias=rb, rowbias_T=3)
    assert a.rowbias_T == 3 and a.epilogue & ops.L.EPI_ROWBIAS
    prev = ops.set_debug_checks(True)
    try:  # the debug extent check knows the segmented size: [B*Tc, cout]
        ops.conv_args(x, w, y, T=20, cin=32, cout=64, ntaps=3, pad=1, rowbias=rb, rowbias_T=3)
        with pytest.raises(ops.L.VqxError, match="rowbias"):
            ops.conv_args(x, w, y, T=20, cin=32, cout=64, ntaps=3, pad=1, rowbias=rb, rowbias_T=4)
    finally:
        ops.set_debug_checks(prev)


# ------------------------------------------------------------------ restatement
@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_equals_the_reference(case):
    """The plain-torch restatement, in float64 on the CPU, reproduces the
    reference's float64 output and every gradient to 1e-12 relative."""
    meta, arr = fixture(case)
    sd = {k: arr["param." + k] for k in meta["keys"]}
    got = run_restated(meta["decoder"], sd, arr["x"], fixture_cond(meta, arr), arr["go"])
    want = expected(meta, arr)
    assert set(got) == set(want)
    worst = 0.0
    for k, w in want.items():
        assert tuple(got[k].shape) == w.shape, k
        e = float(np.abs(got[k].numpy() - w).max() / np.abs(w).max())
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print(f"vqdec {case}: restatement worst relative error {worst:.2e}")
