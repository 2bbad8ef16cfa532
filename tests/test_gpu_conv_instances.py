"""Every conv GEMM kernel instance against a per-element float64 bound.

One or more cases per instance the dispatcher can pick (tests/conv_cases.py:
conv_gemm_kernel by dtype / mode / prologue / GEN tiles / epilogue kind,
conv_gemm3_kernel, conv_tr_kernel with 32- and 16-channel stages,
conv_tr8_kernel, conv_pp_kernel, wgrad_tr_kernel, the three dual kernels and
their refusals).  Each case

  * pins the instance it ran on: the launch probe's info5 records must equal
    the case's `expect` exactly (two records, WGRAD then DGRAD, for a dual call
    that fell back), and the record's flops must be 2 * N * cout * K;
  * checks every output element against the float64 restatement of the
    documented epilogue order: |y - y64| <= (K + 16) 2^-23 S for fp32 values
    (S: the same expression on absolute values), one more rounding
    2^-8 (|y64| + cap) for bf16 stores, term counts added to K for the COLSUM /
    GNBWD / GNSTATS reductions (conv_cases.bounds);
  * NaN-fills every pure output, gives it a leading dimension of cols + 8 and
    trailing sentinel rows, and afterwards wants every logical element finite
    and every sentinel still NaN; the row operands (mask, res, gn_h) carry NaN
    pad columns too, so a read past their width shows; ops' host extent checks
    stay on.

The bound is a condition, not a measurement: one missed tap, a frame reading
across an utterance edge or 8 missing channels exceed it 100-fold and more.
Measured beside it on the MI355X (test_report_worst_errors prints the table):
per family the cases, the worst error/bound over every output, the worst
error of the values kept in fp32 (OUTF32 y, out2, fp32 slabs) in units of
2^-24 S, and float32 torch's worst on the same inputs in the same units
(tests/test_conv_instances_host.py).  The bf16 stores sit at 0.96 - 0.99 of
their bound by construction: it is one bf16 rounding, 2^-8 |y|, and
round-to-nearest-even uses all of it.  Caps are 2 (K + 16) units, 160 and more.

  family             cases  worst error/bound  fp32 units  float32 torch
  gemm_f32             10        0.024            3.88         2.38
  gemm_f32_wgrad        8        0.060            5.72         5.42
  gemm_bf16            46        0.991            1.66         2.43
  gemm_bf16_generic    10        0.982            1.31         2.27
  gemm_bf16_wgrad       8        0.991            1.91         2.72
  gemm3                 8        0.992            1.30         2.21
  tr32                 43        0.987            1.62         2.21
  tr16                 24        0.988            1.47         2.81
  tr8                  25        0.987            1.41         2.10
  pp                   25        0.988            1.65         2.22
  wgrad_tr              4        0.990            1.34         2.17
  dual_tr               3        0.978            1.27         2.83
  dual_k1_3             5        0.993            1.60         2.19
  dual_k1               5        0.993            1.88         2.21
  dual_refused          3        0.985            1.79         1.90

(gemm_*: conv_gemm_kernel, "generic" its prologue / GEN-tile EK_ALL instances;
gemm3: conv_gemm3_kernel; tr32 / tr16: conv_tr_kernel; tr8: conv_tr8_kernel;
pp: conv_pp_kernel; dual_*: vqx_gemm_dual.hip.)  233 tests, 4 s on the GPU.
No case failed: no kernel was changed.
"""
import ctypes
import math

import pytest
import torch

import conv_cases as cc
from conv_cases import BF16, DGRAD, DUAL, FWD, SPLIT_COL, WGRAD

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")

_worst = {}  # family: [cases, worst error / bound, worst fp32 error in units of 2^-24 S] of this run


def _ops():
    from vae_npvc_amd import ops
    return ops


class Guarded:
    """A NaN-filled allocation with `pad` sentinel columns per row and two sentinel rows behind a
    [rows, cols] buffer (the guarded / intact pattern of tests/test_gpu_vq_plain.py).  `live` narrows
    the columns a call is expected to write (SPLIT: y2 is cout wide, written below split_col only)."""

    def __init__(self, rows, cols, dtype, pad=8, init=None, live=None):
        ops = _ops()
        self.whole = torch.full((rows + 2, cols + pad), NAN, device=DEV, dtype=dtype)
        self.view = self.whole[:rows, :cols]
        self.rows, self.cols, self.live = rows, cols, cols if live is None else live
        if init is not None:
            self.view.copy_(init)
        st = self.whole.untyped_storage()
        self.key = st.data_ptr()
        ops._logical_end[self.key] = rows * (cols + pad) * self.whole.element_size()  # extent checks stop here

    def release(self):
        _ops()._logical_end.pop(self.key, None)

    def intact(self):
        w = torch.isnan(self.whole)
        w[:self.rows, :self.live] = True
        return bool(w.all()) and bool(torch.isfinite(self.view[:, :self.live]).all())


def _dev(t):
    return t.to(DEV).contiguous()


def _padded(t):
    """A row operand with 8 NaN pad columns per row."""
    whole = torch.full((t.shape[0], t.shape[1] + 8), NAN, device=DEV, dtype=t.dtype)
    whole[:, :t.shape[1]] = t.to(DEV)
    return whole[:, :t.shape[1]]


def _pack(w3):
    return w3.permute(0, 2, 1).reshape(w3.shape[0], -1).contiguous()


def _conv_call(c, inp, bufs):
    """(x, w, y, kwargs) of the FWD / DGRAD call of a case; allocates its outputs into bufs."""
    fl, N, dt = c.flags, c.N, cc.tdt(c.dt)
    ycols = SPLIT_COL if "split" in fl else c.cout
    kw = dict(T=c.T, cin=c.cin, cout=c.cout, ntaps=c.k, pad=c.pad, dil=c.dil, prologue=c.pro, pro_scale=cc.PRO_SCALE,
              policy=c.policy)
    bufs["y"] = Guarded(N, ycols, torch.float32 if "outf32" in fl else dt)
    if "bias" in fl:
        kw["bias"] = _dev(inp["bias"])
    if "rowbias" in fl:
        kw.update(rowbias=_dev(inp["rowbias"]), rowbias_T=c.rbT)
    if "mask" in fl:
        kw.update(mask=_padded(inp["mask"]), mask_slope=cc.MASK_SLOPE, mask_scale=cc.MASK_SCALE)
    if "res" in fl:
        kw["res"] = _padded(inp["res"])
    if "gnadd" in fl or "gnbwd" in fl:
        kw.update(gn_h=_padded(inp["gn_h"]), gn_mr=_dev(inp["gn_mr"]).view(-1), gn_gamma=_dev(inp["gn_gamma"]),
                  gn_beta=_dev(inp["gn_beta"]))
    if "split" in fl:
        bufs["out2"] = Guarded(N, c.cout - SPLIT_COL, torch.float32, init=inp.get("out2_prior"))
        kw.update(out2=bufs["out2"].view, split_col=SPLIT_COL, out2_accumulate=c.acc)
    if "outf32" in fl:
        kw["out_f32"] = True
    if "act" in fl or "act2" in fl:
        kw["act"] = c.act
    if "act2" in fl:
        bufs["y2"] = Guarded(N, c.cout, dt, live=ycols)
        kw["y2"] = bufs["y2"].view
    tm, tn = (N + 127) // 128, (c.cout + 127) // 128
    if "colsum" in fl:
        bufs["colsum"] = Guarded(tm, c.cout, torch.float32, pad=0)
        kw["colsum"] = bufs["colsum"].view
    if "gnstats" in fl or "gnbwd" in fl:
        bufs["stats"] = Guarded(N // 128 * tn, 4, torch.float32, pad=0)
        kw["gn_stats" if "gnstats" in fl else "gn_bwd"] = bufs["stats"].view
        kw.update(gn_groups=c.G, gn_glu=c.glu)
    return _dev(inp["x"]), _dev(_pack(inp["w3"])), bufs["y"].view, kw


def _wgrad_call(c, bufs, r_dim, c_dim, pad, ops):
    sdt = cc.tdt(c.slab)
    bufs["slabs"] = Guarded(c.splits * r_dim, c.k * c_dim, sdt, pad=0)
    kw = dict(T=c.T, r_dim=r_dim, c_dim=c_dim, ntaps=c.k, pad=pad, shift_sign=c.sign, splits=c.splits, dil=c.dil,
              policy=c.policy)
    if c.mode == WGRAD:
        kw.update(q_prologue=c.pro, pro_scale=cc.PRO_SCALE)
    counters = None
    if c.fixup:
        assert ops.wgrad_fixup_ok(c.N, c.T, r_dim, c_dim, c.k, pad, c.dt, c.slab, policy=c.policy)
        bufs["fixup_dw"] = Guarded(r_dim, c.k * c_dim, torch.float32, pad=0)
        counters = torch.zeros(ops.wgrad_tiles(c.N, c.T, r_dim, c_dim, c.k, pad, c.dt, policy=c.policy),
                               device=DEV, dtype=torch.int32)
        kw.update(fixup_dw=bufs["fixup_dw"].view, fixup_counters=counters)
    return bufs["slabs"].view.view(c.splits, r_dim, c.k * c_dim), kw, counters


def _flops(c):
    conv = 2.0 * c.N * c.cout * c.k * c.cin
    wg = 2.0 * c.N * c.cin * c.k * c.cout
    if c.mode == WGRAD:
        return [wg]
    if c.mode == DUAL:
        return [conv + wg] if c.fused else [wg, conv]
    return [conv]


@pytest.mark.parametrize("c", cc.CASES, ids=[c.id for c in cc.CASES])
def test_conv_instance(c):
    ops = _ops()
    inp = cc.make_inputs(c)
    ref = cc.evaluate(c, inp, torch.float64)
    caps = cc.bounds(c, inp, ref)
    bufs, counters, fused = {}, None, None
    probe = ops.LaunchProbe()
    prev = ops.set_debug_checks(True)
    try:
        probe.select(None)
        probe.clear()
        ops.set_probe(probe)
        if c.mode == WGRAD:
            slabs, kw, counters = _wgrad_call(c, bufs, c.cin, c.cout, c.pad, ops)
            ops.conv_wgrad(_dev(inp["p"]), _dev(inp["q"]), slabs, **kw)
        else:
            x, w, y, kw = _conv_call(c, inp, bufs)
            if c.mode == FWD:
                ops.conv_fwd(x, w, y, **kw)
            elif c.mode == DGRAD:
                ops.conv_dgrad(x, w, y, **kw)
            else:  # the layer's weight gradient: p = dy, q = its input, the forward padding
                slabs, wkw, counters = _wgrad_call(c, bufs, c.cin, c.cout, (c.k - 1) * c.dil - c.pad, ops)
                fused = ops.conv_dgrad_wgrad(x, w, y, kw, x, _dev(inp["q"]), slabs, wkw)
        recs = probe.records()
    except RuntimeError as e:
        from vae_npvc_amd._lib import VqxError
        if isinstance(e, VqxError):     # a refused argument: this case fails
            raise
        # a device error: nothing more may be launched on this GPU in this session
        pytest.exit(f"device error in {c.id}: {e}", returncode=3)
    finally:
        ops.set_probe(None)
        ops.set_debug_checks(prev)
        for g in bufs.values():
            g.release()
    assert [r[4] for r in recs] == list(c.expect), (c.id, [r[4] for r in recs], c.expect)
    assert [r[1] for r in recs] == _flops(c), (c.id, [r[1] for r in recs], _flops(c))
    if c.mode == DUAL:
        assert fused == c.fused, (c.id, fused)
    if counters is not None:
        assert int(counters.abs().sum()) == 0, "fixup counters must be left zero"
    assert set(bufs) == set(ref), (set(bufs), set(ref))
    fam = _worst.setdefault(c.fam, [0, 0.0, 0.0])
    fam[0] += 1
    fails = []
    for name, g in bufs.items():
        assert g.intact(), f"{c.id}: {name}: a sentinel was written or a logical element is not finite"
        cap, as_bf16, unit = caps[name]
        got = g.view[:, :g.live].cpu().reshape(ref[name].shape)
        ok, ratio, un = cc.check(got, ref[name], cap, as_bf16, unit)
        print(f"CONV {c.fam} {c.id} {name}: worst error/bound {ratio:.3g}" +
              (f", {un:.2f} units of 2^-24 S" if un is not None else ""))
        fam[1], fam[2] = max(fam[1], ratio), max(fam[2], un or 0.0)
        if not ok:
            fails.append((name, ratio))
    assert not fails, (c.id, fails)


def test_report_worst_errors():
    """Prints the per-family figures of this run (cases, worst error / bound, worst fp32 error in
    units of 2^-24 S); asserts nothing beyond the cases above."""
    for fam, (n, ratio, un) in sorted(_worst.items()):
        print(f"CONVFAM {fam}: {n} cases, worst error/bound {ratio:.4f}, worst fp32 error {un:.2f} units of 2^-24 S")


# ------------------------------------------------------------------ the probe's entry points

def _one_conv(ops, kind, policy=cc.POL_IM2COL, N=128, cin=64, cout=128):
    """A 1x1 bf16 FWD conv on conv_gemm_kernel: store-only (info5 ek 0) or with a bias (ek 1)."""
    x = torch.randn(N, cin, device=DEV).bfloat16()
    w = torch.randn(cout, cin, device=DEV).bfloat16()
    y = torch.empty(N, cout, device=DEV, dtype=torch.bfloat16)
    bias = torch.zeros(cout, device=DEV) if kind == "elem" else None
    ops.conv_fwd(x, w, y, T=N, cin=cin, cout=cout, ntaps=1, pad=0, policy=policy, bias=bias)


@pytest.fixture
def probe():
    ops = _ops()
    p = ops.LaunchProbe()
    p.select(None)
    p.clear()
    ops.set_probe(p)
    try:
        yield p
    finally:
        p.select(None)
        ops.set_probe(None)
        p.clear()


def _count():
    from vae_npvc_amd._lib import call
    n = ctypes.c_int64(-1)
    call("vqx_probe_count", ctypes.byref(n))
    return n.value


def test_probe_select_records_only_the_chosen_info5(probe):
    ops = _ops()
    probe.select((BF16, FWD, 0, 0, cc.EK_ELEM))
    _one_conv(ops, "none")
    _one_conv(ops, "elem")
    _one_conv(ops, "none")
    assert [r[4] for r in probe.records()] == [(BF16, FWD, 0, 0, cc.EK_ELEM)]
    probe.select(None)
    _one_conv(ops, "none")
    assert [r[4] for r in probe.records()] == [(BF16, FWD, 0, 0, cc.EK_ELEM), (BF16, FWD, 0, 0, cc.EK_NONE)]


def test_probe_enable_zero_pauses_and_keeps_the_log(probe):
    from vae_npvc_amd._lib import call
    ops = _ops()
    _one_conv(ops, "elem")
    call("vqx_probe_enable", 0)
    _one_conv(ops, "none")
    assert _count() == 1
    call("vqx_probe_enable", 1)
    _one_conv(ops, "none")
    assert [r[4][4] for r in probe.records()] == [cc.EK_ELEM, cc.EK_NONE]


def test_probe_clear_empties_the_log(probe):
    from vae_npvc_amd._lib import call
    ops = _ops()
    _one_conv(ops, "elem")
    _one_conv(ops, "none")
    assert _count() == 2
    torch.cuda.synchronize()
    call("vqx_probe_clear")
    assert _count() == 0 and probe.records() == []
    _one_conv(ops, "none")
    assert [r[4][4] for r in probe.records()] == [cc.EK_NONE]


def test_probe_read_rejects_a_bad_index(probe):
    from vae_npvc_amd import _lib as L
    ops = _ops()
    _one_conv(ops, "elem")
    torch.cuda.synchronize()
    info, fl, ms = (ctypes.c_int32 * 5)(), ctypes.c_double(), ctypes.c_float()
    for bad in (1, -1):
        with pytest.raises(L.VqxError, match=f"vqx_probe_read: bad index {bad}"):
            L.call("vqx_probe_read", bad, info, ctypes.byref(fl), ctypes.byref(ms))
    L.call("vqx_probe_read", 0, info, ctypes.byref(fl), ctypes.byref(ms))
    assert tuple(info) == (BF16, FWD, 0, 0, cc.EK_ELEM) and ms.value > 0 and math.isfinite(ms.value)
    with pytest.raises(L.VqxError, match="vqx_probe_count: null"):
        L.call("vqx_probe_count", None)


def test_probe_flops_are_two_n_cout_k(probe):
    ops = _ops()
    _one_conv(ops, "elem", N=384, cin=192, cout=136)
    x = torch.randn(256, 64, device=DEV).bfloat16()
    w = torch.randn(72, 5 * 64, device=DEV).bfloat16()
    ops.conv_fwd(x, w, torch.empty(256, 72, device=DEV, dtype=torch.bfloat16), T=128, cin=64, cout=72, ntaps=5, pad=2,
                 policy=cc.POL_IM2COL)
    assert [r[1] for r in probe.records()] == [2.0 * 384 * 136 * 192, 2.0 * 256 * 72 * 5 * 64]
