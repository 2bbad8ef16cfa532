"""The flat model's batches of different lengths without a GPU: the C-ABI
plumbing and host-side validation of vqx_nct_to_ntc_len / vqx_ntc_to_nct_len
(dummy pointers: every call fails validation first, so nothing is launched),
the host checks of Model.encode / decode / infer with `lengths` on CPU tensors,
and the two drivers' configuration."""
import ctypes
import re

import pytest
import torch

from tests.helpers import ROOT, cfg_of

HEADER = ROOT / "include" / "vqx.h"
NEW = ("vqx_nct_to_ntc_len", "vqx_ntc_to_nct_len")
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


@pytest.mark.parametrize("which", NEW)
def test_validation_names_the_item_and_launches_nothing(which):
    L, lib = _lib()

    def err(ln, x=P, y=P, B=3, C=16, T=10, ld=16, dt=None, T_out=10):
        dt = L.VQX_F32 if dt is None else dt
        if which == "vqx_nct_to_ntc_len":
            args = (x, B, C, T, ln, y, ld, dt, None)
        else:
            args = (y, ld, dt, B, C, T, ln, x, T_out, None)
        assert getattr(lib, which)(*args) == -1
        msg = lib.vqx_last_error()
        assert which.encode() in msg, msg
        return msg

    assert b"item 1: len 0 outside [1, T = 10]" in err(i32(10, 0, 3))
    assert b"item 2: len 11 outside [1, T = 10]" in err(i32(10, 1, 11))
    assert b"item 0: len -4" in err(i32(-4, 1, 1))
    assert b"null len" in err(None)
    assert b"B = 0" in err(i32(1, 1, 1), B=0)
    assert b"not a positive multiple of T" in err(i32(1, 1, 1), T=0)
    assert b"null or unaligned" in err(i32(1, 1, 1), x=None)
    assert b"null or unaligned" in err(i32(1, 1, 1), y=None)
    assert b"null or unaligned" in err(i32(1, 1, 1), x=P + 2)
    assert b"null or unaligned" in err(i32(1, 1, 1), y=P + 2)
    assert b"null or unaligned" in err(i32(1, 1, 1), y=P + 1, dt=L.VQX_BF16)
    assert b"bad dtype" in err(i32(1, 1, 1), dt=7)
    assert b"ldy >= C" in err(i32(1, 1, 1), ld=15)
    assert b"C = 0" in err(i32(1, 1, 1), C=0)
    if which == "vqx_ntc_to_nct_len":
        assert b"T_out = 11 outside [1, T = 10]" in err(i32(1, 1, 1), T_out=11)
        assert b"T_out = 0" in err(i32(1, 1, 1), T_out=0)
    # an item beyond the first launch's table (896 utterances) is checked before that launch too
    big = [5] * 1000
    big[999] = 12
    assert b"item 999: len 12" in err(i32(*big), B=1000)
    with pytest.raises(L.VqxError, match="item 1: len 0"):
        if which == "vqx_nct_to_ntc_len":
            L.call(which, P, 3, 16, 10, i32(10, 0, 3), P, 16, L.VQX_F32, None)
        else:
            L.call(which, P, 16, L.VQX_F32, 3, 16, 10, i32(10, 0, 3), P, 10, None)


def test_ops_wrappers_refuse_host_tensors():
    from vae_npvc_amd import ops
    with pytest.raises(ops.L.VqxError):
        ops.nct_to_ntc_len(torch.zeros(2, 8, 6), [6, 5], torch.zeros(12, 8))  # no CPU path
    with pytest.raises(ops.L.VqxError):
        ops.ntc_to_nct_len(torch.zeros(12, 8), 6, [6, 5], torch.zeros(2, 8, 6))


@pytest.mark.parametrize("name", ["vcc20", "vcc20_multi"])
def test_lengths_are_validated_on_the_host_before_any_launch(name):
    """CPU model, CPU tensors: every refusal is a ValueError from the host checks; valid arguments pass them
    and stop at the device check (VqxError: there is no CPU path)."""
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd.model.vqvae import Model
    cfg = cfg_of(name)
    m = Model(cfg)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    S, K = m.down_scale(), cfg["z_num"]
    assert S == (2 if name == "vcc20_multi" else 1)
    B, T = 2, 100
    x, y = torch.zeros(B, 80, T), torch.zeros(B, 1, dtype=torch.int64)
    for f in (m.encode, lambda a, lengths: m.infer((a, y), lengths=lengths)):
        with pytest.raises(ValueError, match="3 entries for a batch of 2"):
            f(x, lengths=[100, 70, 64])
        with pytest.raises(ValueError, match="utterance 1: length 102 outside 1..100"):
            f(x, lengths=[100, 102])
        with pytest.raises(ValueError, match="utterance 0: length 0 outside 1..100"):
            f(x, lengths=[0, 100])
        with pytest.raises(ValueError, match="sequence of ints"):
            f(x, lengths=[100.0, 70])
        with pytest.raises(ValueError, match="host values"):
            f(x, lengths=torch.tensor([100.0, 70.0]))
        if S > 1:
            with pytest.raises(ValueError, match="utterance 1: length 71 is not a multiple of the down-sampling scale 2"):
                f(x, lengths=[100, 71])
        with pytest.raises(L.VqxError):
            f(x, lengths=[100, 70])
        with pytest.raises(L.VqxError):
            f(x, lengths=torch.tensor([100, 70]))
    with pytest.raises(ValueError, match="x must be"):
        m.encode(torch.zeros(B, 79, T), lengths=[100, 70])
    idx = torch.zeros(B, T // S, dtype=torch.int64)

    def bad(z, lengths=(100, 70), match=None):
        with pytest.raises(ValueError, match=match):
            m.decode((z, y), lengths=list(lengths))

    bad(idx, lengths=(100, 70, 64), match="3 entries for a batch of 2")
    bad(idx, lengths=(100, 0), match="utterance 1: length 0")
    bad(idx[:, :T // S - 1], match=f"the indices hold {T // S - 1} frames, the lengths need {T // S}")
    bad(idx.float(), match="int64")
    if S > 1:
        bad(idx, lengths=(100, 71), match="utterance 1: length 71 is not a multiple")
    z = idx.clone()
    z[1, 70 // S - 1] = K  # the last valid position of utterance 1
    bad(z, match=f"indices in 0..{K}, the codebook holds 0..{K - 1}")
    z = idx.clone()
    z[0, 3] = -1
    bad(z, match="indices in -1..0")
    z = idx.clone()
    z[1, 70 // S] = K  # the first padded position of utterance 1: ignored
    with pytest.raises(L.VqxError):
        m.decode((z, y), lengths=[100, 70])
    with pytest.raises(L.VqxError):
        m.decode((idx, y), lengths=[100, 70])
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_decoder_refuses_bad_decode_batch_size():
    """Checked before the model is built, so no GPU is needed to be refused."""
    from vae_npvc_amd.decoder import basic, hier
    cfg = cfg_of("vcc20")
    for bad in (0, -2, True, "4", 2.0, None):
        with pytest.raises(ValueError, match="decode_batch_size"):
            basic.Decoder(dict(cfg, decode_batch_size=bad))
    assert hier.WINDOW_BATCHES is basic.WINDOW_BATCHES and hier.Decoder.decode_batched is basic.Decoder.decode_batched
    assert basic.length_batches([5, 3, 9, 3, 7], 2) == [[1, 3], [0, 4], [2]]  # stable: ties keep their order


def test_decoder_refuses_a_model_without_lengths():
    from vae_npvc_amd.decoder import basic
    cfg = dict(cfg_of("vcc20"), model_type="vae_npvc_amd.model.vqvae2a", decode_batch_size=4)
    with pytest.raises(NotImplementedError, match="takes no `lengths`"):
        basic.Decoder(cfg)


def test_extract_bnf_parses_batch_size():
    from vae_npvc_amd.bin.extract_bnf import bnf_of, parser
    import numpy as np
    p = parser()
    assert p.parse_args(["-c", "c.yaml", "in", "out"]).batch_size == 1
    assert p.parse_args(["-c", "c.yaml", "--batch_size", "16", "in", "out"]).batch_size == 16
    for bad in ("0", "-3", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["-c", "c.yaml", "--batch_size", bad, "in", "out"])
    ids = np.array([4, 4, 7, 7, 7, 4, 9], dtype=np.int64)
    assert bnf_of(ids, "id") is ids
    assert bnf_of(ids, "csid").tolist() == [4, 7, 4, 9]
    assert bnf_of(ids, "csid").tolist() == torch.from_numpy(ids).unique_consecutive().tolist()
    assert bnf_of(ids, "token").shape == (7, 1)
    with pytest.raises(ValueError, match="unknown bnf_kind"):
        bnf_of(ids, "nope")
