"""Conversion with the hierarchical model without a GPU: the C-ABI plumbing and
host-side limits of vqx_codes_upsample_cat (no launch, no device), the
validation of `Model.synthesize` on CPU tensors (it raises before any libvqx launch),
the ragged stage arithmetic, and the vqinfer fixtures' bookkeeping."""
import ctypes
import json
import re

import pytest
import torch

from tests.helpers import GOLD, ROOT
from tests.hier_model_ref import MODEL_CASES, fixture
from tests.test_gst_host import _c_layout

HEADER = ROOT / "include" / "vqx.h"
FN = "vqx_codes_upsample_cat"


def _lib():
    from vae_npvc_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_entry_point():
    L, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(vqx_\w+)\s*\(", text, flags=re.M))
    assert FN in declared and hasattr(lib, FN) and FN in L._SIGS and FN in L.EXPORTS
    assert "vqx_codes_level" in text
    assert "#define VQX_ABI_VERSION 130" in HEADER.read_text()
    assert lib.vqx_version() == 130 == L.ABI_VERSION


def test_codes_level_layout_matches_header():
    L, _ = _lib()
    names = [f[0] for f in L.CodesLevel._fields_]
    got = _c_layout("vqx_codes_level", names)
    assert got[0] == ctypes.sizeof(L.CodesLevel)
    assert got[1:] == [getattr(L.CodesLevel, n).offset for n in names]


def _levels(L, n=2):
    """Level 0 dense (T_l 1, C 8), the others indexed (K 16, D 16, T_l 3); dummy aligned pointers."""
    arr = (L.CodesLevel * n)()
    for i in range(n):
        if i == 0:
            arr[i].z, arr[i].idx, arr[i].T_l, arr[i].C, arr[i].ld = 0x1000, None, 1, 8, 8
        else:
            arr[i].z, arr[i].idx, arr[i].T_l, arr[i].C, arr[i].ld = 0x3000, 0x5000, 3, 16, 16
            arr[i].K, arr[i].normalize = 16, 1
    return arr


def test_codes_upsample_cat_validation_errors_are_loud():
    """Every host-side limit returns -1 with its message; nothing is launched (dummy pointers)."""
    L, lib = _lib()
    f = getattr(lib, FN)
    B, T, ldo = 2, 20, 24

    def err(levels, n, B=B, T=T, out=0x2000, ldo=ldo, dtype=L.VQX_F32):
        assert f(levels, n, B, T, out, ldo, dtype, None) == -1
        msg = lib.vqx_last_error()
        assert FN.encode() in msg, msg
        return msg

    def changed(level, **kw):
        lv = _levels(L)
        for k, v in kw.items():
            setattr(lv[level], k, v)
        return lv

    assert b"null levels" in err(None, 2)
    assert b"n_levels = 9" in err(_levels(L, 9), 9, ldo=512)  # level count in 1..8
    assert b"n_levels = 0" in err(_levels(L), 0)
    assert b"bad dtype" in err(_levels(L), 2, dtype=2)  # dtypes valid
    assert b"out pointer" in err(_levels(L), 2, out=None)  # pointers non-NULL and 16-byte aligned
    assert b"out pointer" in err(_levels(L), 2, out=0x2004)
    assert b"level 0: null or unaligned (16 B) z" in err(changed(0, z=None), 2)
    assert b"level 0: null or unaligned (16 B) z" in err(changed(0, z=0x1008), 2)
    assert b"level 1: null or unaligned (16 B) codebook" in err(changed(1, z=None), 2)
    assert b"level 1: null or unaligned (16 B) codebook" in err(changed(1, z=0x3004), 2)
    assert b"level 1: unaligned (16 B) idx" in err(changed(1, idx=0x5008), 2)
    assert b"multiples of 4" in err(changed(0, C=6), 2)  # C_l, D_l, ld, ldo multiples of 4
    assert b"multiples of 4" in err(changed(1, C=10), 2)
    assert b"multiples of 4" in err(changed(1, ld=18), 2)
    assert b"ld >= C" in err(changed(1, ld=12), 2)
    assert b"ldo a multiple of 4" in err(_levels(L), 2, ldo=26)
    assert b"T_l = 21 not in 1..T = 20" in err(changed(1, T_l=21), 2)  # 1 <= T_l <= T
    assert b"T_l = 0" in err(changed(0, T_l=0), 2)
    assert b"exceeds ldo = 20" in err(_levels(L), 2, ldo=20)  # sum C_l <= ldo
    assert b"K = 0" in err(changed(1, K=0), 2)  # K_l >= 1
    assert b"B = 0" in err(_levels(L), 2, B=0)
    with pytest.raises(L.VqxError, match="n_levels = 9"):
        L.call(FN, _levels(L, 9), 9, B, T, 0x2000, 512, L.VQX_F32, None)


def test_ops_wrapper_refuses_host_tensors_and_bad_levels():
    from vae_npvc_amd import ops
    out = torch.zeros(10, 8)
    with pytest.raises(ops.L.VqxError):
        ops.codes_upsample_cat([torch.zeros(2, 8)], 2, 5, out)  # no CPU path
    with pytest.raises(ValueError):
        ops.codes_upsample_cat([], 2, 5, out)
    with pytest.raises(ValueError):
        ops.codes_upsample_cat([torch.zeros(2, 8)] * 9, 2, 5, out)


# ------------------------------------------------------------------ model
def test_stage_frames_are_the_strided_convs_output_lengths():
    """kernel 2s, stride s, padding s//2 + s%2 against torch's conv on the CPU, ragged lengths included."""
    from vae_npvc_amd.model.hier_encoder import stage_frames as _stage_frames
    for s in (2, 3, 4, 5):
        conv = torch.nn.Conv1d(1, 1, 2 * s, stride=s, padding=s // 2 + s % 2)
        for T in range(s, 4 * s + 2):
            assert _stage_frames(T, s) == conv(torch.zeros(1, 1, T)).shape[2], (s, T)
    assert [_stage_frames(T, 2) for T in (70, 35)] == [35, 17]
    assert [_stage_frames(T, 4) for T in (17, 4)] == [4, 1]
    assert _stage_frames(9, 1) == 9


@pytest.mark.parametrize("case", MODEL_CASES)
def test_synthesize_validation_raises_before_any_launch(case):
    """CPU model, CPU tensors: every refusal is a ValueError from the host checks
    (a launch, or the device check after them, would raise VqxError instead)."""
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd.model.vqvae2 import Model
    meta, _ = fixture("vqmodel", case)
    m = Model(meta["arch"])
    B = 2
    top = torch.zeros(B, 32, 1) if case == "gst" else torch.zeros(B, 1, dtype=torch.int64)
    good = [torch.zeros(B, 64, dtype=torch.int64), torch.zeros(B, 16, dtype=torch.int64), top]
    y = torch.zeros(B, 1, dtype=torch.int64)
    before = {k: v.clone() for k, v in m.state_dict().items()}

    def bad(codes, y=y, time=None, match=None):
        with pytest.raises(ValueError, match=match):
            m.synthesize((codes, y), time=time)

    bad(good[:2], match="one tensor per level")
    c = [t.clone() for t in good]
    c[1][1, 3] = 16
    bad(c, match=r"level 1 has indices in 0..16, the codebook holds 0..15")  # K = 16
    c = [t.clone() for t in good]
    c[0][0, 0] = -1
    bad(c, match="level 0 has indices in -1")
    bad([good[0], good[1][:1], good[2]], match="batch size")
    bad(good, y=y[:1], match="y_idx")
    bad([good[0], torch.zeros(B, 65, dtype=torch.int64), good[2]], match="level 1 has 65 frames")  # T_l <= T = 64
    bad(good, time=10, match="level 0 has 64 frames")
    bad([good[0], good[1].float(), good[2]], match="level 1 is a quantized level")
    if case == "gst":
        bad([good[0], good[1], torch.zeros(B, 16, 1)], match="channels sum to 144")  # 64 + 64 + 16, wants 160
        bad([good[0], good[1], torch.zeros(B, 1, dtype=torch.int64)], match="style level")
    # the valid codes pass the host checks and stop at the device check: no CPU path
    with pytest.raises(L.VqxError):
        m.synthesize((good, y))
    with pytest.raises(L.VqxError):
        m.synthesize((iter(good), y))  # any iterable of codes: it is read once
    with pytest.raises(L.VqxError):
        m.analyze(torch.zeros(B, 24, 64))
    with pytest.raises(ValueError):
        m.analyze(torch.zeros(B, 23, 64))
    for f in (m.encode, m.decode, m.infer):
        with pytest.raises(NotImplementedError):
            f(None)
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_hier_decoder_driver_is_a_basic_decoder():
    from vae_npvc_amd.decoder import basic, hier
    assert issubclass(hier.Decoder, basic.Decoder)
    assert hier.Decoder.decode is basic.Decoder.decode
    assert hier.Decoder.decode_step is not basic.Decoder.decode_step


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("case", MODEL_CASES)
def test_infer_fixture_bookkeeping(case):
    meta = json.load(open(GOLD / f"vqinfer_{case}.json"))
    _, arr = fixture("vqinfer", case)
    assert (meta["B"], meta["T"], meta["level_lengths"]) == (1, 70, [70, 17, 1])
    assert meta["gap"] >= 1e-3 and min(meta["gaps32"] + meta["gaps64"]) == meta["gap"]
    assert arr["x"].shape == (1, 24, 70) and arr["xhat"].shape == (1, 24, 70) and arr["xhat"].dtype.name == "float64"
    assert int(arr["y"][0, 0]) != int(arr["y_tgt"][0, 0])
    n_idx = 2 if case == "gst" else 3  # top first
    assert [arr[f"idx.{k}"].shape for k in range(n_idx)] == [(1, t) for t in ([17, 70] if case == "gst" else [1, 17, 70])]
    assert meta["arch"] == fixture("vqmodel", case)[0]["arch"]
    files = sorted(GOLD.glob(f"vqinfer_{case}*"))
    assert max(f.stat().st_size for f in files) < (1 << 20)
