"""CPU-side checks of the conv GEMM instance table (tests/conv_cases.py), so a
missing or mislabelled case fails without a GPU: the table's expected info5
set is the enumerated instance list, every case's flags select the epilogue
kind it claims, its shape passes the dispatch conditions of its family, and
float32 torch stays under the per-element cap on every case's inputs."""
import pytest
import torch

import conv_cases as cc
from conv_cases import BF16, DGRAD, DUAL, F32, FWD, WGRAD

# vqx_gemm_kernel.h ek_mask / vqx_gemm_inst.h pick_ek, restated
_ELEM = cc.epi_bits(["bias", "rowbias", "mask", "res", "act", "act2", "outf32"])
EK_MASK = [cc.BITS["outf32"], _ELEM, _ELEM | cc.BITS["gnadd"], _ELEM | cc.BITS["split"], _ELEM | cc.BITS["colsum"],
           _ELEM | cc.BITS["gnstats"], _ELEM | cc.BITS["colsum"] | cc.BITS["gnbwd"]]


def pick_ek(epi):
    for ek, mask in enumerate(EK_MASK):
        if epi & ~mask == 0:
            return ek
    return cc.EK_ALL


def test_table_covers_exactly_the_enumerated_instances():
    expected = {e for c in cc.CASES for e in c.expect}
    inst = cc.instance_list()
    assert expected == inst, (sorted(inst - expected), sorted(expected - inst))
    assert len(inst) == 132


def test_every_largest_flag_set_selects_its_kind():
    for kind, flags in cc.KIND_FLAGS.items():
        assert pick_ek(cc.epi_bits(flags)) == cc.KIND_EK[kind], kind
    # ... and is the largest of its kind, ACT aside (ACT2 in its place): one more flag leaves the kind
    for kind in ("elem", "gnadd", "split", "colsum", "gnstats", "gnbwd"):
        have = cc.epi_bits(cc.KIND_FLAGS[kind]) | cc.BITS["act"] | cc.BITS["outf32"]
        assert have == EK_MASK[cc.KIND_EK[kind]], kind


@pytest.mark.parametrize("c", cc.CASES, ids=[c.id for c in cc.CASES])
def test_case_claims_the_kind_its_flags_select(c):
    ek = pick_ek(cc.epi_bits(c.flags))
    dgrad = c.expect[-1]                     # the FWD / DGRAD record (a refused dual call: the second)
    if c.mode == WGRAD:
        assert c.expect == ((c.dt, WGRAD, c.expect[0][2], c.expect[0][3], cc.EK_NONE),) and not c.flags
        return
    generic = c.dt == F32 or c.pro != 0 or (c.cin % 64 != 0 and dgrad[3] == cc.FAM_GEMM_GEN)
    assert dgrad[4] == (cc.EK_ALL if generic else ek), (c.id, ek, dgrad)
    assert dgrad[0] == c.dt and dgrad[1] == (DUAL if c.fused else DGRAD if c.mode == DUAL else c.mode)


@pytest.mark.parametrize("c", cc.CASES, ids=[c.id for c in cc.CASES])
def test_case_shape_meets_its_family(c):
    """The host-side argument rules (vqx_gemm.hip conv_prepare / wgrad_prepare) and the shape
    conditions of the family the case names."""
    fl, fam = c.flags, c.expect[-1][3]
    epc = 8 if c.dt == BF16 else 4
    assert c.cin % epc == 0 and c.cout % 8 == 0 and 1 <= c.k <= 8 and 0 <= c.pad <= (c.k - 1) * c.dil
    if c.mode == WGRAD:
        bk = 64 if c.dt == BF16 else 32
        gen = c.T % bk != 0 or c.N % bk != 0
        if fam == cc.FAM_TR:
            assert not gen and c.k == 3 and c.pad == 1 and c.cout % 64 == 0 and c.policy != cc.POL_IM2COL
        else:
            assert c.expect[0][3] == int(gen)
        return
    if "gnstats" in fl or "gnbwd" in fl:
        assert c.T % 128 == 0 and "gnadd" not in fl
        assert c.glu or (c.cout // c.G) % 128 == 0
    if c.rbT:
        assert c.mode == FWD and "rowbias" in fl and c.rbT <= c.T
    if fam in (cc.FAM_GEMM, cc.FAM_GEMM_GEN) and c.mode != DUAL:
        bk = 64 if c.dt == BF16 else 32
        assert c.expect[0][3] == int(c.cin % bk != 0)
    if fam in (cc.FAM_TR, cc.FAM_TR8, cc.FAM_PP):
        assert c.dt == BF16 and c.k == 3 and c.pad == 1 and c.dil == 1 and c.T % 128 == 0 and c.pro == 0
        slot = c.expect[-1][2]
        if fam == cc.FAM_TR:
            assert slot == (32 if c.cin % 32 == 0 else 16) and c.cin % 16 == 0 and c.cin % 64 in (0, 16, 48)
        else:
            assert c.T % 256 == 0 and c.N % (256 * slot if fam == cc.FAM_TR8 and not c.rbT else 512) == 0
    if fam == cc.FAM_GEMM3:
        assert c.k == 1 and c.policy == cc.POL_AUTO and c.cin % 64 == 0
        assert -(-c.N // 128) * -(-c.cout // 128) <= 3 * 64   # a grid no GPU of this family fills three per CU
    if c.mode == DUAL and c.fused and c.k == 1:
        assert (-(-c.N // 128) * -(-c.cout // 128)) % 8 == 0


@pytest.mark.parametrize("c", cc.CASES, ids=[c.id for c in cc.CASES])
def test_float32_torch_stays_under_the_cap(c):
    """The cap is a condition any correct fp32-accumulating implementation meets: stock float32
    torch, evaluating the same expression on the same inputs, stays under it (1.9 - 5.5 units of
    2^-24 S against caps of 2 (K + 16) units) -- with the fp32 form of the cap for every output,
    since torch rounds nothing to bf16."""
    inp = cc.make_inputs(c)
    ref = cc.evaluate(c, inp, torch.float64)
    got = cc.evaluate(c, inp, torch.float32)
    caps = cc.bounds(c, inp, ref)
    assert set(caps) == set(ref)
    for name in ref:
        cap, _, unit = caps[name]
        assert cap.shape == ref[name].shape, (name, cap.shape, ref[name].shape)
        ok, ratio, un = cc.check(got[name], ref[name], cap, False, unit)
        assert ok, (c.id, name, ratio)
        if un is not None:
            assert un < 8.0, (c.id, name, un)


def test_the_cap_catches_the_structural_bugs():
    """An utterance-edge frame reading its neighbour utterance on 8 output channels, and a frame
    missing the last 8 input channels of one tap: both pass a 2e-2 norm-wise bar and miss the
    per-element cap by a factor of 100 or more."""
    c = next(x for x in cc.CASES if x.id == "slots_gemm_bf16_outf32_act2")   # 3 taps, y kept in fp32
    d64 = torch.float64
    inp = cc.make_inputs(c)
    ref = cc.evaluate(c, inp, d64)
    cap, as_bf16, _ = cc.bounds(c, inp, ref)["y"]
    acc = cc.conv_acc(c, inp, d64, False)
    w, x, n = inp["w3"].double(), inp["x"].double(), c.T
    # bug 1: frame 0 of utterance 1, tap 0 reads the last frame of utterance 0 instead of padding
    edge = acc.clone()
    edge[n, :8] += w[:8, :, 0] @ x[n - 1]
    # bug 2: frame 5 misses the last 8 input channels of tap 1
    short = acc.clone()
    short[5] -= w[:, -8:, 1] @ x[5, -8:]
    for a in (edge, short):
        bad = cc.epilogue(c, inp, a, d64)["v"]
        ok, ratio, _ = cc.check(bad, ref["y"], cap, as_bf16)
        rel = float((bad - ref["y"]).norm() / ref["y"].norm())
        assert not ok and ratio > 100 and rel < 2e-2, (ratio, rel)
