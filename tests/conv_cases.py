"""Case table, float64 reference and per-element bound of the conv GEMM kernel
instances (tests/test_gpu_conv_instances.py runs them on the GPU,
tests/test_conv_instances_host.py checks the table on the CPU).

Every case names the launch-probe label(s) `info5 = (dtype, mode, prologue
slot, family, epilogue kind)` it must produce (ops.LaunchProbe.records()[i][4],
vqx_gemm_inst.h / vqx_gemm_dual.hip), so a change to a dispatch predicate that
moves a case onto another kernel fails the case instead of silently leaving an
instance uncovered.

Reference: the documented epilogue order (include/vqx.h: bias, row bias, mask,
split, residual, GroupNorm add, activation) restated once, generic over the
torch dtype: float64 gives the reference, float32 the error stock torch makes
on the same inputs.  `absv=True` evaluates the same expression with every
product and addend replaced by its absolute value: S.  The operands are the
values the kernel reads (bf16-rounded, the prologue applied in fp32 and
rounded to the operand type as the staging code does).

Left out on purpose: GNSTATS or GNBWD together with SPLIT.  include/vqx.h
defines the partials over "the stored fp32 values" of y, which end at
split_col, while tile_epilogue counts the out2 columns of a tile as zeros (and
the host check wants cout / gn_groups % 128 == 0 of the whole width).  No
caller combines them, the kernel is kept as it is, and no case pins either
reading.
"""
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from vae_npvc_amd import _lib as L

F32, BF16 = L.VQX_F32, L.VQX_BF16
FWD, DGRAD, WGRAD, DUAL = 0, 1, 2, 3              # info5 mode slot (3: one launch for DGRAD + WGRAD)
EK_NONE, EK_ELEM, EK_GNADD, EK_SPLIT, EK_COLSUM, EK_GNSTATS, EK_GNBWD, EK_ALL = range(8)
POL_AUTO, POL_IM2COL, POL_TALL256, POL_TALL512, POL_TR128, POL_K1_2PCU = range(6)
# info5 family slot
FAM_GEMM, FAM_GEMM_GEN, FAM_TR, FAM_TR8, FAM_GEMM3, FAM_DUAL, FAM_PP = 0, 1, 2, 3, 4, 5, 6

MASK_SLOPE, MASK_SCALE, PRO_SCALE = 0.2, 0.5, 0.5
SPLIT_COL = 136                                    # inside the second column tile: it holds y and out2 columns
U23, U24 = 2.0 ** -23, 2.0 ** -24

BITS = {"bias": L.EPI_BIAS, "rowbias": L.EPI_ROWBIAS, "mask": L.EPI_MASK, "res": L.EPI_RES, "gnadd": L.EPI_GNADD,
        "split": L.EPI_SPLIT, "outf32": L.EPI_OUTF32, "act": L.EPI_ACT, "act2": L.EPI_ACT2, "colsum": L.EPI_COLSUM,
        "gnstats": L.EPI_GNSTATS, "gnbwd": L.EPI_GNBWD}
ELEM = frozenset({"bias", "rowbias", "mask", "res", "act2"})
# the largest flag set of each epilogue kind (OUTF32 on the store-only kind: its only flag);
# "all_split" / "all_gnadd": flag sets no single kind covers, which select EK_ALL on the bf16 fast path
KIND_FLAGS = {"none": frozenset({"outf32"}), "elem": ELEM, "gnadd": ELEM | {"gnadd"}, "split": ELEM | {"split"},
              "colsum": ELEM | {"colsum"}, "gnstats": ELEM | {"gnstats"}, "gnbwd": ELEM | {"colsum", "gnbwd"},
              "all_split": ELEM | {"split", "colsum"}, "all_gnadd": ELEM | {"gnadd", "colsum"}}
KIND_EK = {"none": EK_NONE, "elem": EK_ELEM, "gnadd": EK_GNADD, "split": EK_SPLIT, "colsum": EK_COLSUM,
           "gnstats": EK_GNSTATS, "gnbwd": EK_GNBWD, "all_split": EK_ALL, "all_gnadd": EK_ALL}


def epi_bits(flags):
    e = 0
    for f in flags:
        e |= BITS[f]
    return e


@dataclass(frozen=True)
class Case:
    id: str
    fam: str             # kernel family (report key)
    mode: int            # FWD | DGRAD | WGRAD | DUAL
    expect: tuple        # the probe's info5 records, in launch order
    dt: int
    B: int
    T: int
    cin: int             # FWD/DGRAD: `cin` of the call (DGRAD: channels of dy); WGRAD: r_dim
    cout: int            # FWD/DGRAD: `cout` of the call; WGRAD: c_dim
    k: int = 1
    dil: int = 1
    pad: int = 0
    pro: int = 0
    policy: int = POL_AUTO
    flags: frozenset = frozenset()
    acc: bool = False    # out2_accumulate
    glu: bool = False
    G: int = 1
    rbT: int = 0
    act: int = L.PRO_LRELU
    splits: int = 1      # WGRAD / DUAL
    sign: int = 1
    slab: int = F32
    fixup: bool = False
    fused: object = None  # DUAL: the `fused` answer
    note: str = ""

    @property
    def N(self):
        return self.B * self.T

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())


# --------------------------------------------------------------- the table

def _shape(kind, B=3, T=72, cout=200):
    """Generic-kernel shape of a flag set: GroupNorm partials need T % 128 == 0 and 128-channel groups."""
    if kind in ("gnstats", "gnbwd"):
        return dict(B=2, T=128, cout=256)
    return dict(B=B, T=T, cout=cout)


def _variants(kind):
    """(id suffix, extra fields) of the runs a flag set asks for: SPLIT with both
    out2_accumulate values, GNBWD plain (two groups) and GLU."""
    if kind in ("split", "all_split"):
        return [("", {}), ("_acc", {"acc": True})]
    if kind == "gnbwd":
        return [("", {"G": 2}), ("_glu", {"glu": True, "G": 2})]
    return [("", {})]


KINDS8 = ["none", "elem", "gnadd", "split", "colsum", "gnstats", "gnbwd", "all_split", "all_gnadd"]
MODE_NAME = {FWD: "fwd", DGRAD: "dgrad", WGRAD: "wgrad", DUAL: "dual"}
# taps of the generic-kernel cases, in turn: (k, dil, pad): 1x1, centred 3 taps, causal 5 taps
# dilation 2 (pad = (k-1)*dil), 8 taps without padding, anti-causal 3 taps (pad 0)
TAPS = [(1, 1, 0), (3, 1, 1), (5, 2, 8), (8, 1, 0), (3, 1, 0), (5, 2, 4), (3, 1, 2), (8, 1, 7)]


def _add(out, **kw):
    kw["flags"] = frozenset(kw.get("flags", ()))
    kw["expect"] = tuple(tuple(e) for e in kw["expect"])
    out.append(Case(**kw))


def build_cases():
    out = []
    # ---- conv_gemm_kernel<float, ..., EK_ALL>: FWD x prologue x GEN (cin % 32), DGRAD x GEN
    rot = ["elem", "gnadd", "split", "colsum", "all_split", "all_gnadd", "gnstats", "gnbwd"]
    for gen in (0, 1):
        for pro in range(4):
            i = pro + 4 * gen
            kind, (k, dil, pad) = rot[i], TAPS[i]
            for suf, ex in _variants(kind)[:1]:
                _add(out, id=f"f32_fwd_pro{pro}_gen{gen}_{kind}", fam="gemm_f32", mode=FWD, dt=F32,
                     expect=[(F32, FWD, pro, gen, EK_ALL)], cin=36 if gen else 32, k=k, dil=dil, pad=pad, pro=pro,
                     flags=KIND_FLAGS[kind], **_shape(kind), **ex)
        kind = ("all_split", "gnbwd")[gen]
        suf, ex = _variants(kind)[1]
        _add(out, id=f"f32_dgrad_gen{gen}_{kind}{suf}", fam="gemm_f32", mode=DGRAD, dt=F32,
             expect=[(F32, DGRAD, 0, gen, EK_ALL)], cin=36 if gen else 32, k=3, dil=1, pad=gen, flags=KIND_FLAGS[kind],
             **_shape(kind), **ex)
    # ---- WGRAD of conv_gemm_kernel (EK_NONE), f32 and bf16: prologue x GEN (frames: T or N % BK != 0)
    for dt, dn, bk in ((F32, "f32", 32), (BF16, "bf16", 64)):
        for gen in (0, 1):
            for pro in range(4):
                k, dil, pad = TAPS[(pro + 4 * gen + 1) % 8]
                B, T = (3, 72) if gen else (3, 64)
                # 216 rows in 5 splits of 64: the last split is empty; 192 rows in 2 splits
                _add(out, id=f"{dn}_wgrad_pro{pro}_gen{gen}", fam=f"gemm_{dn}_wgrad", mode=WGRAD, dt=dt,
                     expect=[(dt, WGRAD, pro, gen, EK_NONE)], B=B, T=T, cin=136, cout=72, k=k, dil=dil, pad=pad,
                     pro=pro, policy=POL_IM2COL, splits=5 if gen else 2, sign=-1 if pro == 2 else 1,
                     slab=BF16 if (dt == BF16 and pro % 2 == 0) else F32)
    # ---- conv_gemm_kernel<bf16> under IM2COL: FWD/DGRAD x the 8 epilogue kinds (cin 64 / 192)
    for mode in (FWD, DGRAD):
        for i, kind in enumerate(KINDS8):
            k, dil, pad = TAPS[i % 8]
            for suf, ex in _variants(kind):
                _add(out, id=f"bf16_{MODE_NAME[mode]}_{kind}{suf}", fam="gemm_bf16", mode=mode, dt=BF16,
                     expect=[(BF16, mode, 0, 0, KIND_EK[kind])], cin=192 if i % 2 else 64, k=k, dil=dil, pad=pad,
                     policy=POL_IM2COL, flags=KIND_FLAGS[kind], **_shape(kind), **ex)
    # the receptive field (49 frames) longer than the utterance (40)
    _add(out, id="bf16_fwd_short_utt", fam="gemm_bf16", mode=FWD, dt=BF16, expect=[(BF16, FWD, 0, 0, EK_ELEM)],
         B=3, T=40, cin=64, cout=200, k=7, dil=8, pad=24, policy=POL_IM2COL, flags=ELEM)
    # segmented row bias (rowbias_T = 9 segments of 8 frames) on the prefetching kernel
    _add(out, id="bf16_fwd_rowbias_seg", fam="gemm_bf16", mode=FWD, dt=BF16, expect=[(BF16, FWD, 0, 0, EK_ELEM)],
         B=3, T=72, cin=64, cout=200, k=3, dil=1, pad=1, policy=POL_IM2COL, flags=ELEM, rbT=9)
    # FWD prologue 1-3 (EK_ALL), and GEN tiles (cin % 64 != 0): FWD prologue 0-3, DGRAD
    for pro in (1, 2, 3):
        kind = ("gnadd", "all_split", "colsum")[pro - 1]
        k, dil, pad = TAPS[pro]
        _add(out, id=f"bf16_fwd_pro{pro}_{kind}", fam="gemm_bf16_generic", mode=FWD, dt=BF16,
             expect=[(BF16, FWD, pro, 0, EK_ALL)], cin=64, k=k, dil=dil, pad=pad, pro=pro, policy=POL_IM2COL,
             flags=KIND_FLAGS[kind], **_shape(kind))
    for pro in range(4):
        kind = ("elem", "gnstats", "all_gnadd", "split")[pro]
        k, dil, pad = TAPS[pro + 3]
        _add(out, id=f"bf16_fwd_gen_pro{pro}_{kind}", fam="gemm_bf16_generic", mode=FWD, dt=BF16,
             expect=[(BF16, FWD, pro, 1, EK_ALL)], cin=96 if pro % 2 else 72, k=k, dil=dil, pad=pad, pro=pro,
             policy=POL_IM2COL, flags=KIND_FLAGS[kind], **_shape(kind), **({"acc": True} if kind == "split" else {}))
    _add(out, id="bf16_dgrad_gen_gnbwd_glu", fam="gemm_bf16_generic", mode=DGRAD, dt=BF16,
         expect=[(BF16, DGRAD, 0, 1, EK_ALL)], cin=72, k=3, dil=1, pad=1, policy=POL_IM2COL,
         flags=KIND_FLAGS["gnbwd"], glu=True, G=2, **_shape("gnbwd"))
    # cin = 96, 3 taps, T % 128 == 0 under AUTO: GEN with cin % 32 == 0, which tap_reuse_ok refuses
    for mode in (FWD, DGRAD):
        _add(out, id=f"bf16_{MODE_NAME[mode]}_cin96_auto", fam="gemm_bf16_generic", mode=mode, dt=BF16,
             expect=[(BF16, mode, 0, 1, EK_ALL)], B=2, T=128, cin=96, cout=200, k=3, dil=1, pad=1, policy=POL_AUTO,
             flags=ELEM)
    # ---- conv_gemm3_kernel: 1x1 under AUTO at a grid of at most three workgroups per CU.  The same
    # instances under K1_2PCU need a grid between 2 and 3 per CU, which depends on the CU count: they
    # are this code, covered here.
    for mode in (FWD, DGRAD):
        for kind in ("none", "elem", "split"):
            for suf, ex in _variants(kind):
                _add(out, id=f"gemm3_{MODE_NAME[mode]}_{kind}{suf}", fam="gemm3", mode=mode, dt=BF16,
                     expect=[(BF16, mode, 0, FAM_GEMM3, KIND_EK[kind])], B=3, T=72, cin=192 if mode else 64, cout=200,
                     policy=POL_AUTO, flags=KIND_FLAGS[kind], **ex)
    # a 1x1 GNADD call under AUTO stays on conv_gemm_kernel (its prefetch needs the two-per-CU registers)
    _add(out, id="bf16_fwd_1x1_gnadd_auto", fam="gemm_bf16", mode=FWD, dt=BF16, expect=[(BF16, FWD, 0, 0, EK_GNADD)],
         B=3, T=72, cin=64, cout=200, policy=POL_AUTO, flags=KIND_FLAGS["gnadd"])
    # ---- conv_tr_kernel<MODE, EK, 32> (policy TR128: independent of the CU count) and <..., 16>
    for bkc, cins, pol in ((32, (64, 64), POL_TR128), (16, (48, 80), POL_AUTO)):
        for mode in (FWD, DGRAD):
            for i, kind in enumerate(KINDS8):
                for j, (suf, ex) in enumerate(_variants(kind)):
                    B, T = ((2, 128), (1, 256))[(i + j) % 2]   # T = 256: the halo rows lie inside an utterance
                    _add(out, id=f"tr{bkc}_{MODE_NAME[mode]}_{kind}{suf}", fam=f"tr{bkc}", mode=mode, dt=BF16,
                         expect=[(BF16, mode, bkc, FAM_TR, KIND_EK[kind])], B=B, T=T, cin=cins[(i + j) % 2],
                         cout=256 if kind in ("gnstats", "gnbwd") else 200, k=3, dil=1, pad=1, policy=pol,
                         flags=KIND_FLAGS[kind], **ex)
    # ---- conv_tr8_kernel (TALL256) and conv_pp_kernel (TALL512).  Their automatic choice (tr8_segs:
    # 512-frame tiles where every CU still gets a workgroup) depends on the CU count and runs this code.
    for fam, pol, seg, famid, shapes in (("tr8", POL_TALL256, 1, FAM_TR8, ((2, 256), (1, 512))),
                                         ("pp", POL_TALL512, 2, FAM_PP, ((1, 512), (4, 256)))):
        for mode in (FWD, DGRAD):
            for i, kind in enumerate(KINDS8):
                for j, (suf, ex) in enumerate(_variants(kind)):
                    B, T = shapes[(i + j) % 2]
                    _add(out, id=f"{fam}_{MODE_NAME[mode]}_{kind}{suf}", fam=fam, mode=mode, dt=BF16,
                         expect=[(BF16, mode, seg, famid, KIND_EK[kind])], B=B, T=T, cin=64,
                         cout=256 if kind in ("gnstats", "gnbwd") else 200, k=3, dil=1, pad=1, policy=pol,
                         flags=KIND_FLAGS[kind], **ex)
    # segmented row bias: the ping-pong kernel's EK_ALL instance is built without it, so the call
    # takes 256-frame tiles (launch_tr); the specialised kinds keep the ping-pong kernel
    _add(out, id="pp_fwd_all_rowbias_seg", fam="tr8", mode=FWD, dt=BF16, expect=[(BF16, FWD, 1, FAM_TR8, EK_ALL)],
         B=1, T=512, cin=64, cout=200, k=3, dil=1, pad=1, policy=POL_TALL512, flags=KIND_FLAGS["all_split"], rbT=8)
    _add(out, id="pp_fwd_elem_rowbias_seg", fam="pp", mode=FWD, dt=BF16, expect=[(BF16, FWD, 2, FAM_PP, EK_ELEM)],
         B=1, T=512, cin=64, cout=200, k=3, dil=1, pad=1, policy=POL_TALL512, flags=ELEM, rbT=5)
    # ---- wgrad_tr_kernel: with / without the in-launch split-K reduction, shift sign +-1
    for sign in (1, -1):
        for fix in (False, True):
            _add(out, id=f"wgrad_tr_sign{sign}_fix{int(fix)}", fam="wgrad_tr", mode=WGRAD, dt=BF16,
                 expect=[(BF16, WGRAD, 1, FAM_TR, EK_NONE)], B=3, T=64, cin=136, cout=64, k=3, dil=1, pad=1,
                 splits=4 if fix else 2, sign=sign, slab=BF16 if fix else F32, fixup=fix)
    # ---- DGRAD + WGRAD in one launch: info5 = (bf16, 3, kind, 5, EK)
    for kind in ("none", "elem", "colsum"):
        _add(out, id=f"dual_tr_{kind}", fam="dual_tr", mode=DUAL, dt=BF16,
             expect=[(BF16, DUAL, 2, FAM_DUAL, KIND_EK[kind])], B=2, T=128, cin=64, cout=128, k=3, dil=1, pad=1,
             policy=POL_AUTO, flags=KIND_FLAGS[kind], splits=3, slab=BF16, fused=True)
    for pol, slot, fam in ((POL_AUTO, 4, "dual_k1_3"), (POL_K1_2PCU, 3, "dual_k1")):
        for kind in ("none", "elem", "colsum", "gnbwd"):
            for suf, ex in _variants(kind):
                # 1024 rows: 8 row tiles, so nd % 8 == 0 with any number of column tiles
                _add(out, id=f"{fam}_{kind}{suf}", fam=fam, mode=DUAL, dt=BF16,
                     expect=[(BF16, DUAL, slot, FAM_DUAL, KIND_EK[kind])], B=8, T=128, cin=64,
                     cout=256 if kind == "gnbwd" else 200, policy=pol, flags=KIND_FLAGS[kind], splits=5,
                     slab=BF16 if kind == "elem" else F32, fused=True, **ex)
    # the refusals: two launches, WGRAD then DGRAD
    _add(out, id="dual_refused_kind", fam="dual_refused", mode=DUAL, dt=BF16, B=2, T=128, cin=64, cout=128, k=3,
         pad=1, policy=POL_AUTO, flags=KIND_FLAGS["gnadd"], splits=2, fused=False,
         expect=[(BF16, WGRAD, 1, FAM_TR, EK_NONE), (BF16, DGRAD, 32, FAM_TR, EK_GNADD)],
         note="no dual instance of the GNADD epilogue kind")
    _add(out, id="dual_refused_nd", fam="dual_refused", mode=DUAL, dt=BF16, B=3, T=128, cin=64, cout=128,
         policy=POL_AUTO, flags=ELEM, splits=2, fused=False,
         expect=[(BF16, WGRAD, 0, FAM_GEMM, EK_NONE), (BF16, DGRAD, 0, FAM_GEMM3, EK_ELEM)],
         note="1x1 with nd = 3 data-gradient workgroups, not a multiple of 8")
    _add(out, id="dual_refused_gen", fam="dual_refused", mode=DUAL, dt=BF16, B=2, T=128, cin=80, cout=64, k=3, pad=1,
         policy=POL_AUTO, flags=ELEM, splits=2, fused=False,
         expect=[(BF16, WGRAD, 1, FAM_TR, EK_NONE), (BF16, DGRAD, 16, FAM_TR, EK_ELEM)],
         note="a GEN data gradient (80 channels of dy)")
    # ---- the slot-role table of epi_prefetch on a family that prefetches (conv_gemm_kernel bf16 FWD)
    # and one that does not (conv_tr_kernel): {no GN, GNADD, GNBWD, GNBWD+GLU} x MASK x RES
    for fam, pol, famid, slot in (("gemm_bf16", POL_IM2COL, FAM_GEMM, 0), ("tr32", POL_TR128, FAM_TR, 32)):
        for gn in ("nogn", "gnadd", "gnbwd", "gnbwdglu"):
            for mask in (0, 1):
                for res in (0, 1):
                    fl = {"bias"} | ({"mask"} if mask else set()) | ({"res"} if res else set())
                    fl |= {"nogn": set(), "gnadd": {"gnadd"}, "gnbwd": {"gnbwd"}, "gnbwdglu": {"gnbwd"}}[gn]
                    ek = {"nogn": EK_ELEM, "gnadd": EK_GNADD}.get(gn, EK_GNBWD)
                    glu = gn == "gnbwdglu"
                    # GLU sums need no 128-channel groups: 200 channels, a ragged second column tile
                    _add(out, id=f"slots_{fam}_{gn}_m{mask}_r{res}", fam=fam, mode=FWD, dt=BF16,
                         expect=[(BF16, FWD, slot, famid, ek)], B=2, T=128, cin=64,
                         cout=256 if gn == "gnbwd" else 200, k=3, dil=1, pad=1, policy=pol, flags=fl, glu=glu,
                         G=2 if glu else 1)
        for name, fl in (("act", {"bias", "mask", "res", "act"}), ("act_relu", {"bias", "res", "act"}),
                         ("outf32_act2", {"bias", "mask", "res", "act2", "outf32"})):
            _add(out, id=f"slots_{fam}_{name}", fam=fam, mode=FWD, dt=BF16, expect=[(BF16, FWD, slot, famid, EK_ELEM)],
                 B=2, T=128, cin=64, cout=200, k=3, dil=1, pad=1, policy=pol, flags=fl,
                 act=L.PRO_RELU if name == "act_relu" else L.PRO_LRELU)
    ids = [c.id for c in out]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    return out


CASES = build_cases()


def instance_list():
    """Every kernel instance the dispatcher can pick (vqx_gemm_inst.h, vqx_gemm_dual.hip) as info5,
    written as products with the stated exclusions."""
    s = set()
    eks = range(8)
    fd = (FWD, DGRAD)
    # conv_gemm_kernel<float>: FWD x prologue x GEN, DGRAD (no prologue) x GEN, all EK_ALL; WGRAD EK_NONE
    s |= {(F32, FWD, p, g, EK_ALL) for p in range(4) for g in (0, 1)}
    s |= {(F32, DGRAD, 0, g, EK_ALL) for g in (0, 1)}
    s |= {(dt, WGRAD, p, g, EK_NONE) for dt in (F32, BF16) for p in range(4) for g in (0, 1)}
    # conv_gemm_kernel<bf16>: one instance per kind without prologue and GEN; prologues and GEN: EK_ALL
    s |= {(BF16, m, 0, 0, ek) for m in fd for ek in eks}
    s |= {(BF16, FWD, p, 0, EK_ALL) for p in (1, 2, 3)}
    s |= {(BF16, FWD, p, 1, EK_ALL) for p in range(4)} | {(BF16, DGRAD, 0, 1, EK_ALL)}
    # conv_gemm3_kernel: NONE, ELEM, SPLIT only
    s |= {(BF16, m, 0, FAM_GEMM3, ek) for m in fd for ek in (EK_NONE, EK_ELEM, EK_SPLIT)}
    # tap reuse: 32- and 16-channel stages, tall (256-frame) and ping-pong (512-frame) tiles
    s |= {(BF16, m, slot, fam, ek) for m in fd for ek in eks
          for slot, fam in ((32, FAM_TR), (16, FAM_TR), (1, FAM_TR8), (2, FAM_PP))}
    s |= {(BF16, WGRAD, 1, FAM_TR, EK_NONE)}
    # dual launches: 3-tap (2) x {NONE, ELEM, COLSUM}; 1x1 two (3) / three (4) per CU: those and GNBWD
    s |= {(BF16, DUAL, 2, FAM_DUAL, ek) for ek in (EK_NONE, EK_ELEM, EK_COLSUM)}
    s |= {(BF16, DUAL, k, FAM_DUAL, ek) for k in (3, 4) for ek in (EK_NONE, EK_ELEM, EK_COLSUM, EK_GNBWD)}
    return s


# --------------------------------------------------------------- inputs

def tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def apply_pro(x, pro, scale):
    """The prologue as the staging code applies it: in fp32, rounded to the operand type."""
    xf = x.float()
    if pro == L.PRO_LRELU:
        xf = torch.where(xf > 0, xf, xf * 0.2)
    elif pro == L.PRO_RELU:
        xf = torch.relu(xf)
    elif pro == L.PRO_SCALE_RELU:
        xf = torch.relu(xf * scale)
    return xf.to(x.dtype)


def make_inputs(c):
    """CPU tensors of a case, in the types the kernel reads (all from torch.manual_seed)."""
    g = torch.Generator().manual_seed(c.seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    dt, N, fl = tdt(c.dt), c.N, c.flags
    d = {}
    if c.mode == WGRAD:
        d["p"], d["q"] = rn(N, c.cin).to(dt), rn(N, c.cout).to(dt)
        return d
    d["x"] = rn(N, c.cin).to(dt)
    # FWD: Conv1d weight [cout, cin, k]; DGRAD: the forward layer's [cout_f = cin, cin_f = cout, k]
    d["w3"] = (rn(c.cout, c.cin, c.k) if c.mode == FWD else rn(c.cin, c.cout, c.k)).div((c.k * c.cin) ** 0.5).to(dt)
    if c.mode == DUAL:
        d["q"] = rn(N, c.cout).to(dt)          # the forward layer's input
    ycols = SPLIT_COL if "split" in fl else c.cout
    if "bias" in fl:
        d["bias"] = rn(c.cout)
    if "rowbias" in fl:
        d["rowbias"] = rn(c.B * max(1, c.rbT), c.cout)
    if "mask" in fl:
        d["mask"] = rn(N, c.cout).to(dt)
    if "res" in fl:
        d["res"] = rn(N, ycols).to(dt)         # SPLIT: exactly split_col wide
    if "gnadd" in fl or "gnbwd" in fl:
        gc = c.cout * (2 if c.glu else 1)
        ng = c.G if "gnbwd" in fl else 1
        d["gn_h"] = rn(N, gc).to(dt)
        mr = torch.empty(c.B, ng, 2)
        mr[..., 0] = 0.1 * rn(c.B, ng)
        mr[..., 1] = 0.5 + torch.rand(c.B, ng, generator=g)
        d["gn_mr"], d["gn_gamma"], d["gn_beta"] = mr, rn(gc), rn(gc)
    if "split" in fl and c.acc:
        d["out2_prior"] = rn(N, c.cout - SPLIT_COL)
    return d


# --------------------------------------------------------------- reference

def _ntc(x, B, T):
    return x.view(B, T, -1).permute(0, 2, 1)


def _rows(y):
    return y.permute(0, 2, 1).reshape(y.shape[0] * y.shape[2], y.shape[1])


def conv_acc(c, inp, dt, absv):
    """The GEMM: FWD as F.conv1d, DGRAD as F.conv_transpose1d (the tap-flipped conv), frames
    outside an utterance read as zero."""
    f = (lambda t: t.to(dt).abs()) if absv else (lambda t: t.to(dt))
    x = _ntc(f(apply_pro(inp["x"], c.pro, PRO_SCALE)), c.B, c.T)
    w = f(inp["w3"])
    span = (c.k - 1) * c.dil
    if c.mode == FWD:
        return _rows(F.conv1d(F.pad(x, (c.pad, span - c.pad)), w, dilation=c.dil))
    full = F.conv_transpose1d(x, w, dilation=c.dil)     # [m] = sum_j w[..j] dy[m - j*dil]
    pf = span - c.pad                                     # the forward layer's padding
    return _rows(full[..., pf:pf + c.T])


def act_fn(v, act):
    return torch.where(v > 0, v, v * 0.2) if act == L.PRO_LRELU else torch.relu(v)


def epilogue(c, inp, acc, dt, absv=False):
    """{'v': the value y stores (before rounding; out2 columns dropped), 'y2', 'out2'} in `dt`."""
    fl = c.flags
    f = (lambda t: t.to(dt).abs()) if absv else (lambda t: t.to(dt))
    v = acc
    rows = torch.arange(c.N)
    b = rows // c.T
    if "bias" in fl:
        v = v + f(inp["bias"])
    if "rowbias" in fl:
        ridx = b
        if c.rbT > 1:
            ridx = b * c.rbT + torch.clamp((rows - b * c.T) // (c.T // c.rbT), max=c.rbT - 1)
        v = v + f(inp["rowbias"])[ridx]
    if "mask" in fl:
        m = inp["mask"].float() > 0
        one, slope = torch.tensor(1.0), torch.tensor(MASK_SLOPE, dtype=torch.float32)
        v = v * (torch.where(m, one, slope) * torch.tensor(MASK_SCALE, dtype=torch.float32)).to(dt)
    out = {}
    if "split" in fl:
        o2 = v[:, SPLIT_COL:]
        if c.acc:
            o2 = o2 + f(inp["out2_prior"])
        out["out2"] = o2
        v = v[:, :SPLIT_COL]
    if "res" in fl:
        v = v + f(inp["res"])
    if "gnadd" in fl:
        mr = inp["gn_mr"].to(dt)[b, 0]
        h, ga, be = f(inp["gn_h"]), f(inp["gn_gamma"]), f(inp["gn_beta"])
        mean, rstd = mr[:, :1], mr[:, 1:]
        v = v + (((h + mean.abs()) * rstd * ga + be) if absv else ((h - mean) * rstd * ga + be))
    if "act2" in fl:
        out["y2"] = v if absv else act_fn(v, c.act)
    elif "act" in fl and not absv:
        v = act_fn(v, c.act)
    out["v"] = v
    return out


def _gn_coeff(c, inp, dt, absv):
    """Coefficients c_k[n][col] with GNBWD sum k = sum over the tile of c_k * dy (vqx_gemm_kernel.h gnbwd8)."""
    f = (lambda t: t.to(dt).abs()) if absv else (lambda t: t.to(dt))
    b = torch.arange(c.N) // c.T
    u, ga_all, mr = f(inp["gn_h"]), f(inp["gn_gamma"]), inp["gn_mr"].to(dt)
    C = c.cout
    sub = (lambda a, m: a + m.abs()) if absv else (lambda a, m: a - m)
    if not c.glu:
        grp = torch.arange(C) // (C // c.G)
        m, r = mr[b][:, grp, 0], mr[b][:, grp, 1]
        xh = sub(u, m) * r
        return [ga_all.expand_as(xh), ga_all * xh, None, None]
    be_all = f(inp["gn_beta"])
    ga, gb, ba, bb = ga_all[:C], ga_all[C:], be_all[:C], be_all[C:]
    xa = sub(u[:, :C], mr[b, 0, :1]) * mr[b, 0, 1:]
    xb = sub(u[:, C:], mr[b, 1, :1]) * mr[b, 1, 1:]
    # the gates themselves are bounded functions: evaluated on the true operands in either mode
    t = inp["gn_h"].to(dt)
    g0, b0 = inp["gn_gamma"].to(dt), inp["gn_beta"].to(dt)
    ta = torch.tanh((t[:, :C] - mr[b, 0, :1]) * mr[b, 0, 1:] * g0[:C] + b0[:C])
    sb = torch.sigmoid((t[:, C:] - mr[b, 1, :1]) * mr[b, 1, 1:] * g0[C:] + b0[C:])
    if absv:
        dga, dgb = ga * sb * (1 + ta * ta), gb * ta.abs() * sb * (1 + sb)
    else:
        dga, dgb = ga * sb * (1 - ta * ta), gb * ta * sb * (1 - sb)
    return [dga, dga * xa, dgb, dgb * xb]


def _tiles(t, rows=128, cols=128):
    """[N, C] -> list over (row tile, column tile) of blocks (ragged at the ends)."""
    return [[blk for blk in torch.split(rt, cols, dim=1)] for rt in torch.split(t, rows, dim=0)]


def derived(c, inp, v, dt):
    """COLSUM rows, GNSTATS moments and GNBWD sums of the stored values `v`, in `dt`."""
    fl, out = c.flags, {}
    if "colsum" in fl:
        cs = torch.stack([rt.sum(0) for rt in torch.split(v, 128, dim=0)])
        if "split" in fl:                                  # out2 columns contribute zero
            cs = torch.cat([cs, torch.zeros(cs.shape[0], c.cout - SPLIT_COL, dtype=dt)], 1)
        out["colsum"] = cs
    if "gnstats" in fl:
        st = []
        for row in _tiles(v):
            st.append([])
            for blk in row:
                mean = blk.mean()
                st[-1].append(torch.stack([torch.tensor(float(blk.numel()), dtype=dt), mean,
                                           ((blk - mean) ** 2).sum(), torch.tensor(0.0, dtype=dt)]))
        out["stats"] = torch.stack([torch.stack(r) for r in st])
    if "gnbwd" in fl:
        co = _gn_coeff(c, inp, dt, False)
        zero = torch.tensor(0.0, dtype=dt)
        tl = [_tiles(v)] + [(_tiles(k) if k is not None else None) for k in co]
        st = [[torch.stack([(tl[1 + k][i][j] * blk).sum() if tl[1 + k] is not None else zero for k in range(4)])
               for j, blk in enumerate(row)] for i, row in enumerate(tl[0])]
        out["stats"] = torch.stack([torch.stack(r) for r in st])
    return out


def wgrad_slabs(c, p, q, dt, absv, r_dim=None, c_dim=None, pad=None):
    """slabs[s][r][j*c_dim + c] = sum_{n in split s} p[n][r] * pro(q[n + sign*(j*dil - pad)][c]); also
    the frames of each split."""
    f = (lambda t: t.to(dt).abs()) if absv else (lambda t: t.to(dt))
    pad = c.pad if pad is None else pad
    pro = c.pro if c.mode == WGRAD else 0
    pp, qq = f(p), f(apply_pro(q, pro, PRO_SCALE)).view(c.B, c.T, -1)
    taps = []
    for j in range(c.k):
        sh = c.sign * (j * c.dil - pad)
        s = torch.zeros_like(qq)
        lo, hi = max(0, -sh), min(c.T, c.T - sh)
        if hi > lo:
            s[:, lo:hi] = qq[:, lo + sh:hi + sh]
        taps.append(s.reshape(c.N, -1))
    qs = torch.stack(taps, 1)                              # [N, k, c_dim]
    kround = 64 if c.dt == BF16 else 32
    kps = -(-(-(-c.N // c.splits)) // kround) * kround     # frames per split, whole K-tiles
    slabs, frames = [], []
    for s in range(c.splits):
        a, b = min(c.N, s * kps), min(c.N, (s + 1) * kps)
        slabs.append(torch.einsum("nr,njc->rjc", pp[a:b], qs[a:b]).reshape(pp.shape[1], -1))
        frames.append(b - a)
    return torch.stack(slabs), frames


def evaluate(c, inp, dt):
    """Every output of the case computed in `dt`: {name: tensor}."""
    out = {}
    if c.mode == WGRAD:
        out["slabs"], _ = wgrad_slabs(c, inp["p"], inp["q"], dt, False)
        if c.fixup:
            out["fixup_dw"] = out["slabs"].sum(0)
        return out
    e = epilogue(c, inp, conv_acc(c, inp, dt, False), dt)
    out["y"] = e["v"]
    for k in ("y2", "out2"):
        if k in e:
            out[k] = e[k]
    out.update(derived(c, inp, e["v"], dt))
    if c.mode == DUAL:  # the weight gradient of the same layer: p = dy, q = the layer's input
        out["slabs"], _ = wgrad_slabs(c, inp["x"], inp["q"], dt, False, pad=(c.k - 1) * c.dil - c.pad)
    return out


def bounds(c, inp, ref):
    """{name: (fp32 cap, stored as bf16?)} for the float64 outputs `ref` of evaluate(): per element
    |y - y64| <= (K + 16) 2^-23 S for a value kept in fp32, K the number of products and S the
    expression on absolute values; a bf16 store adds one rounding, 2^-8 (|y64| + cap), bf16's unit
    roundoff.  2^-23 (not 2^-24) assumes no round-to-nearest inside the MFMA.  Reductions of
    stored values (COLSUM, GNBWD, GNSTATS) add their term count to K and sum S over the tile."""
    d64 = torch.float64
    bf = c.dt == BF16
    out = {}
    if c.mode == WGRAD or c.mode == DUAL:
        p, q = (inp["p"], inp["q"]) if c.mode == WGRAD else (inp["x"], inp["q"])
        S, frames = wgrad_slabs(c, p, q, d64, True, pad=None if c.mode == WGRAD else (c.k - 1) * c.dil - c.pad)
        K = torch.tensor(frames, dtype=d64).view(-1, 1, 1)
        cap = (K + 16) * U23 * S
        out["slabs"] = (cap, c.slab == BF16, U24 * S)
        if c.fixup:   # the splits' stored (bf16) slabs summed in fp32
            capb = cap + 2.0 ** -8 * (ref["slabs"].abs() + cap)
            out["fixup_dw"] = (capb.sum(0) + c.splits * U23 * (ref["slabs"].abs() + capb).sum(0), False, None)
        if c.mode == WGRAD:
            return out
    K = c.k * c.cin
    S = epilogue(c, inp, conv_acc(c, inp, d64, True), d64, absv=True)
    cap = (K + 16) * U23 * S["v"]
    out["y"] = (cap, bf and "outf32" not in c.flags, U24 * S["v"])
    if "y2" in S:
        out["y2"] = ((K + 16) * U23 * S["y2"], bf, U24 * S["y2"])
    if "out2" in S:
        out["out2"] = ((K + 16) * U23 * S["out2"], False, U24 * S["out2"])
    fl = c.flags
    if "colsum" in fl:
        cs = torch.stack([(K + rt.shape[0] + 16) * U23 * rt.sum(0) for rt in torch.split(S["v"], 128, dim=0)])
        if "split" in fl:
            cs = torch.cat([cs, torch.zeros(cs.shape[0], c.cout - SPLIT_COL, dtype=d64)], 1)
        out["colsum"] = (cs, False, None)
    if "gnstats" in fl:
        st = []
        for rv, rs in zip(_tiles(ref["y"]), _tiles(S["v"])):
            st.append([])
            for bv, bs in zip(rv, rs):
                n = bv.numel()
                e = (K + 16) * U23 * bs                          # each value
                em = (K + n + 16) * U23 * bs.mean()              # their mean
                dv = (bv - bv.mean()).abs()
                em2 = (2 * dv * (e + em) + (e + em) ** 2).sum() + (n + 16) * U23 * ((dv + e + em) ** 2).sum()
                st[-1].append(torch.stack([torch.tensor(0.0, dtype=d64), em, em2, torch.tensor(0.0, dtype=d64)]))
        out["stats"] = (torch.stack([torch.stack(r) for r in st]), False, None)
    if "gnbwd" in fl:
        co = _gn_coeff(c, inp, d64, True)
        zero = torch.tensor(0.0, dtype=d64)
        tS = _tiles(S["v"])
        tl = [(_tiles(k) if k is not None else None) for k in co]
        st = [[torch.stack([(K + blk.numel() + 16) * U23 * (tl[k][i][j] * blk).sum() if tl[k] is not None else zero
                            for k in range(4)]) for j, blk in enumerate(row)] for i, row in enumerate(tS)]
        out["stats"] = (torch.stack([torch.stack(r) for r in st]), False, None)
    return out


def check(got, ref, cap, stored_bf16, unit=None):
    """(every element within its bound, worst error / bound, worst error in units of 2^-24 S or None)
    of one output.  An element whose bound is zero (an empty split, a zero count) must be exact."""
    got, ref = got.double(), ref.double()
    lim = cap + (2.0 ** -8 * (ref.abs() + cap) if stored_bf16 else 0.0)
    err = (got - ref).abs()
    ok = bool((err <= lim).all())
    nz = lim > 0
    ratio = float((err[nz] / lim[nz]).max()) if bool(nz.any()) else 0.0
    un = None
    if unit is not None and not stored_bf16 and bool((unit > 0).any()):
        un = float((err[unit > 0] / unit[unit > 0]).max())
    return ok, ratio, un
