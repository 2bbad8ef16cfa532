"""A batch of different lengths without a GPU: the C-ABI plumbing and the
host-side validation of the vqx_*_len entry points (dummy pointers: every call
fails validation first, so nothing is launched), `Model.level_lengths`, the
host checks of `analyze` / `synthesize` / `convert` with `lengths`, the decode
driver's configuration and the vqragged fixtures' bookkeeping."""
import ctypes
import json
import re

import pytest
import torch

from tests.helpers import GOLD, ROOT
from tests.hier_model_ref import MODEL_CASES, fixture

HEADER = ROOT / "include" / "vqx.h"
NEW = ("vqx_groupnorm_stats_len", "vqx_gn_lrelu_fwd_len", "vqx_gn_glu_fwd_len", "vqx_mask_tail",
       "vqx_codes_upsample_cat_len", "vqx_segment_mean")
P = 0x10000  # a dummy aligned pointer, never dereferenced


def _lib():
    from vae_npvc_amd import _lib as L
    return L, L.load()


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_header_declares_and_library_exports_the_entry_points():
    L, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(vqx_\w+)\s*\(", text, flags=re.M))
    for fn in NEW:
        assert fn in declared and hasattr(lib, fn) and fn in L._SIGS and fn in L.EXPORTS, fn
    assert lib.vqx_version() == 130 == L.ABI_VERSION  # additive: the ABI version did not change
    from vae_npvc_amd.csrc.build import SOURCES
    assert "vqx_varlen.hip" in SOURCES


def _calls(L):
    """name -> f(len array, **overrides) issuing a call that is valid but for its overrides (B = 3, T = 10)."""
    def stats(ln, x=P, ldx=16, dt=L.VQX_F32, n=30, T=10, C=16, G=2):
        return ("vqx_groupnorm_stats_len", (x, ldx, dt, n, T, C, G, ln, 1e-5, P, P, None))

    def lrelu(ln, h=P, ld=16, dt=L.VQX_F32, n=30, T=10, C=16):
        return ("vqx_gn_lrelu_fwd_len", (h, ld, P, ld, dt, n, T, C, ln, P, P, P, None))

    def glu(ln, u=P, ld=16, dt=L.VQX_F32, n=30, T=10, C=16):
        return ("vqx_gn_glu_fwd_len", (u, ld, P, ld, dt, n, T, C, ln, P, P, P, None))

    def mask(ln, x=P, ld=16, dt=L.VQX_F32, n=30, T=10, C=16):
        return ("vqx_mask_tail", (x, ld, dt, n, T, C, ln, None))

    def mean(ln, z=P, ld=16, n=30, T=10, C=16):
        return ("vqx_segment_mean", (z, ld, n, T, C, ln, P, ld, None))

    return dict(stats=stats, lrelu=lrelu, glu=glu, mask=mask, mean=mean)


@pytest.mark.parametrize("which", ["stats", "lrelu", "glu", "mask", "mean"])
def test_length_validation_names_the_item_and_launches_nothing(which):
    L, lib = _lib()
    make = _calls(L)[which]

    def err(ln, **kw):
        name, args = make(ln, **kw)
        assert getattr(lib, name)(*args) == -1
        msg = lib.vqx_last_error()
        assert name.encode() in msg, msg
        return msg

    assert b"item 1: len 0 outside [1, T = 10]" in err(i32(10, 0, 3))
    assert b"item 2: len 11 outside [1, T = 10]" in err(i32(10, 1, 11))
    assert b"item 0: len -4" in err(i32(-4, 1, 1))
    assert b"null len" in err(None)
    assert b"not a positive multiple of T" in err(i32(1, 1, 1), n=31)
    assert b"not a positive multiple of T" in err(i32(1, 1, 1), T=0)
    first = {"stats": "x", "lrelu": "h", "glu": "u", "mask": "x", "mean": "z"}[which]
    assert b"aligned" in err(i32(1, 1, 1), **{first: P + 4})
    assert b"multiples of" in err(i32(1, 1, 1), C=18)
    if which != "mean":
        assert b"bad dtype" in err(i32(1, 1, 1), dt=7)
        assert b"multiples of 8" in err(i32(1, 1, 1), dt=L.VQX_BF16, C=12, **({"G": 1} if which == "stats" else {}))
    if which == "stats":
        assert b"G = 3" in err(i32(1, 1, 1), G=3)
    # an item beyond the first launch's table is checked before that launch too
    big = [5] * 1000
    big[999] = 12
    name, args = make(i32(*big), n=1000 * 10)
    assert getattr(lib, name)(*args) == -1 and b"item 999: len 12" in lib.vqx_last_error()
    name, args = make(i32(10, 0, 3))
    with pytest.raises(L.VqxError, match="item 1: len 0"):
        L.call(name, *args)


def _levels(L, T1=5):
    """Level 0 dense (T_l 1, C 8), level 1 indexed (K 16, D 16, padded T_l = T1); dummy aligned pointers."""
    arr = (L.CodesLevel * 2)()
    arr[0].z, arr[0].idx, arr[0].T_l, arr[0].C, arr[0].ld = 0x1000, None, 1, 8, 8
    arr[1].z, arr[1].idx, arr[1].T_l, arr[1].C, arr[1].ld = 0x3000, 0x5000, T1, 16, 16
    arr[1].K, arr[1].normalize = 16, 1
    return arr


def test_codes_upsample_cat_len_validation_errors_are_loud():
    L, lib = _lib()
    fn = "vqx_codes_upsample_cat_len"
    f = getattr(lib, fn)
    B, T = 2, 20

    def err(n_len=i32(20, 9), m_len=i32(1, 5, 1, 2), levels=None, n=2, B=B, T=T, out=0x2000, ldo=24, dt=L.VQX_F32):
        assert f(levels if levels is not None else _levels(L), n, B, T, n_len, m_len, out, ldo, dt, None) == -1
        msg = lib.vqx_last_error()
        assert fn.encode() in msg, msg
        return msg

    assert b"item 1: length 21 outside [1, T = 20]" in err(n_len=i32(20, 21))
    assert b"item 0: length 0" in err(n_len=i32(0, 9))
    assert b"item 1: level 1: length 6 outside [1, min(9, T_l = 5)]" in err(m_len=i32(1, 5, 1, 6))
    assert b"item 0: level 0: length 2 outside [1, min(20, T_l = 1)]" in err(m_len=i32(2, 5, 1, 2))
    assert b"item 1: level 1: length 0" in err(m_len=i32(1, 5, 1, 0))
    assert b"item 1: level 1: length 4 outside [1, min(3, T_l = 5)]" in err(n_len=i32(20, 3), m_len=i32(1, 5, 1, 4))
    assert b"null levels or lengths" in err(n_len=None)
    assert b"null levels or lengths" in err(m_len=None)
    assert b"n_levels = 9" in err(n=9)
    assert b"bad dtype" in err(dt=3)
    assert b"out pointer" in err(out=0x2004)
    assert b"exceeds ldo = 20" in err(ldo=20)
    assert b"T_l = 21 not in 1..T = 20" in err(levels=_levels(L, 21))
    lv = _levels(L)
    lv[1].idx = 0x5008
    assert b"level 1: unaligned (16 B) idx" in err(levels=lv)
    # an item beyond the first launch's table (96 utterances) is checked before that launch
    nb = 200
    n_len, m_len = [20] * nb, [1, 5] * nb
    m_len[2 * 150 + 1] = 9  # above the level's padded T_l = 8
    assert f(_levels(L, 8), 2, nb, T, i32(*n_len), i32(*m_len), 0x2000, 24, L.VQX_F32, None) == -1
    assert b"item 150: level 1: length 9" in lib.vqx_last_error()


def test_ops_wrappers_refuse_host_tensors_and_device_lengths():
    from vae_npvc_amd import ops
    x = torch.zeros(20, 16)
    with pytest.raises(ops.L.VqxError):
        ops.mask_tail(x, 10, [3, 4])  # no CPU path
    with pytest.raises(ValueError, match="3 entries for a batch of 2"):
        ops.len_array([3, 4, 5], 2)
    with pytest.raises(ValueError, match="sequence of ints"):
        ops.len_array([3.0, 4])
    with pytest.raises(ValueError, match="sequence of ints"):
        ops.len_array([])
    with pytest.raises(ValueError, match="host values"):
        ops.len_array(torch.zeros(2))  # a float tensor
    assert list(ops.len_array(torch.tensor([7, 9]))) == [7, 9] and list(ops.len_array((7, 9), 2)) == [7, 9]
    arr = ops.len_array([1, 2])
    assert ops.len_array(arr, 2) is arr


# ------------------------------------------------------------------ model
def _strided(T, s):
    return torch.nn.functional.conv1d(torch.zeros(1, 1, T), torch.zeros(1, 1, 2 * s), stride=s,
                                      padding=s // 2 + s % 2).shape[2]


@pytest.mark.parametrize("case", MODEL_CASES)
def test_level_lengths_are_the_strided_convs_lengths(case):
    """64..200 frames through the architecture's stage convs (kernel 2s, stride s, padding s//2 + s%2) as
    torch's conv1d on the CPU computes their output lengths."""
    from vae_npvc_amd.model.vqvae2 import Model
    meta, _ = fixture("vqmodel", case)
    m = Model(meta["arch"])
    lens = list(range(64, 201))
    got = m.level_lengths(lens)
    assert len(got) == 3 and all(len(g) == len(lens) for g in got)
    for k, T in enumerate(lens):
        l1 = _strided(_strided(T, 2), 2)
        l2 = _strided(_strided(l1, 4), 4)
        assert [got[0][k], got[1][k], got[2][k]] == [T, l1, l2], T
    assert m.level_lengths([130, 70, 64, 97]) == [[130, 70, 64, 97], [32, 17, 16, 24], [2, 1, 1, 1]]
    assert m.level_lengths(torch.tensor([70])) == [[70], [17], [1]]
    with pytest.raises(ValueError, match="utterance 1 of 15 frames leaves level 2 without a frame"):
        m.level_lengths([64, 15])  # 15 -> 7 -> 3 -> 0
    with pytest.raises(ValueError):
        m.level_lengths([64.0])


@pytest.mark.parametrize("case", MODEL_CASES)
def test_lengths_are_validated_on_the_host_before_any_launch(case):
    """CPU model, CPU tensors: every refusal is a ValueError from the host checks; valid arguments pass them
    and stop at the device check (VqxError: there is no CPU path)."""
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd.model.vqvae2 import Model
    meta, _ = fixture("vqmodel", case)
    m = Model(meta["arch"])
    B = 2
    x, y = torch.zeros(B, 24, 100), torch.zeros(B, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="exceed x's 100 frames"):
        m.analyze(x, [100, 101])
    with pytest.raises(ValueError, match="without a frame"):
        m.analyze(x, [100, 15])
    with pytest.raises(ValueError, match="3 entries for a batch of 2"):
        m.analyze(x, [100, 70, 64])
    with pytest.raises(ValueError, match="sequence of ints"):
        m.convert((x, y), lengths=[100.0, 70])
    with pytest.raises(L.VqxError):
        m.analyze(x, [100, 70])
    with pytest.raises(L.VqxError):
        m.analyze(x, torch.tensor([100, 70]))
    top = torch.zeros(B, 32, 1) if case == "gst" else torch.zeros(B, 1, dtype=torch.int64)
    good = [torch.zeros(B, 100, dtype=torch.int64), torch.zeros(B, 25, dtype=torch.int64), top]

    def bad(codes, lengths=(100, 70), time=None, match=None):
        with pytest.raises(ValueError, match=match):
            m.synthesize((codes, y), time=time, lengths=list(lengths))

    bad(good, lengths=(100, 70, 64), match="3 entries for a batch of 2")
    bad(good, lengths=(100, 15), match="without a frame")
    bad(good, time=120, match="max\\(lengths\\) = 100")
    bad([good[0], good[1][:, :24], good[2]], match="level 1 holds 24 frames, the lengths need 25")
    bad([good[0][:, :99], good[1], good[2]], match="level 0 holds 99 frames, the lengths need 100")
    bad(good[:2], match="one tensor per level")
    c = [t.clone() for t in good]
    c[1][1, 3] = 16
    bad(c, match="level 1 has indices in 0..16")
    if case == "gst":
        bad([good[0], good[1], torch.zeros(B, 32, 2)], match="style level is \\(B, F, 1\\)")
    with pytest.raises(L.VqxError):
        m.synthesize((good, y), lengths=[100, 70])
    with pytest.raises(L.VqxError):
        m.synthesize((good, y), time=100, lengths=[100, 70])
    # without lengths nothing changed: a batch of a ragged length is still refused
    with pytest.raises(L.VqxError):
        m.analyze(torch.zeros(B, 24, 64))


def test_hier_decoder_reads_decode_batch_size():
    import inspect
    from vae_npvc_amd.decoder import basic, hier
    assert hier.Decoder.decode is basic.Decoder.decode  # one decode; batches are handed to decode_batched
    assert "decode_batch_size" in inspect.getsource(hier.Decoder.__init__)
    assert hier.WINDOW_BATCHES >= 1


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("case", MODEL_CASES)
def test_ragged_fixture_bookkeeping(case):
    meta = json.load(open(GOLD / f"vqragged_{case}.json"))
    _, arr = fixture("vqragged", case)
    assert meta["lengths"] == [130, 70, 64, 97]
    assert meta["level_lengths"] == [[130, 70, 64, 97], [32, 17, 16, 24], [2, 1, 1, 1]]
    assert meta["gap"] >= 1e-3 and min(meta["gaps"]) == meta["gap"]
    n_idx = 2 if case == "gst" else 3  # top first
    for b, T in enumerate(meta["lengths"]):
        assert arr[f"x.{b}"].shape == (24, T) and arr[f"xhat.{b}"].shape == (24, T)
        assert arr[f"xhat.{b}"].dtype.name == "float64" and 0 < meta["err32"][f"xhat.{b}"] < 1e-5
        want = [meta["level_lengths"][i][b] for i in ([1, 0] if case == "gst" else [2, 1, 0])]
        assert [arr[f"idx.{b}.{k}"].shape for k in range(n_idx)] == [(t,) for t in want]
        assert int(arr["y"][b, 0]) != int(arr["y_tgt"][b, 0])
    assert meta["arch"] == fixture("vqmodel", case)[0]["arch"]
    files = sorted(GOLD.glob(f"vqragged_{case}*"))
    assert max(f.stat().st_size for f in files) < (1 << 20)
