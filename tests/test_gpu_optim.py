"""Kernel-level tests of the optimizer launches (csrc/vqx_optim.hip) that the
step fixtures reach only through whole training steps: vqx_adam_step_wn
against vqx_adam_step + vqx_weight_norm_fwd bit for bit (and, through them,
torch.optim.Adam), vqx_radam_hyper against include/vqx.h's formulas in Python
floats and vqx_radam_step against the CPU oracle's RAdam.  Every in/out buffer
carries NaN past its logical end, every pure output is NaN-filled before the
launch.  Runs on the MI355X only (-m gpu)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _ops():
    from vae_npvc_amd import ops
    return ops


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def guarded(n, dtype=torch.float32, pad=8):
    """(whole, view): `n` elements followed by `pad` NaN sentinels."""
    whole = torch.full((n + pad,), NAN, device=DEV, dtype=dtype)
    return whole, whole[:n]


def intact(whole, n):
    """The sentinels past `n` are still NaN and nothing before them is."""
    return bool(torch.isnan(whole[n:]).all()) and not bool(torch.isnan(whole[:n]).any())


# ---- vqx_adam_step_wn

# kind, cout, cin, k: block-per-row (240 columns; kWnRow = 4096 columns), wave-per-row (two 256-column halves
# with idle waves in the last block; one half), ConvTranspose1d (70 rows of 400 columns, norms only)
LAYERS = [(0, 96, 80, 3), (0, 2, 1024, 4), (0, 6, 512, 1), (0, 8, 128, 1), (1, 100, 70, 4)]
# the flat buffer in order: ("v" | "g", layer) rows and gains, ("seg", name, length) everything else
ORDER = [("seg", "X", 3), ("g", 1), ("seg", "S1", 4096 + 3), ("v", 0), ("v", 1), ("seg", "S2", 4096), ("v", 2),
         ("seg", "S3", 2 * 4096 + 6), ("g", 4), ("v", 4), ("g", 0), ("seg", "S4", 0), ("v", 3), ("g", 3), ("g", 2),
         ("seg", "S5", 5)]
SEG_TABLE = ["X", "S1", "S2", "S4", "S3", "S5"]  # the zero-length one in the middle of the table


def _rows_cols(kind, cout, cin, k):
    return (cout, cin * k) if kind == 0 else (cin, cout * k)


def _layout():
    """n, {("v" | "g", layer): offset}, {segment: (offset, length)} of ORDER."""
    off, at, segs = 0, {}, {}
    for it in ORDER:
        if it[0] == "seg":
            segs[it[1]] = (off, it[2])
            off += it[2]
        else:
            rows, cols = _rows_cols(*LAYERS[it[1]])
            at[it] = off
            off += rows * cols if it[0] == "v" else rows
    # what the issue's layout asks for
    assert all(at[("v", i)] % 4 == 0 for i in range(len(LAYERS)))
    assert segs["S1"][0] % 4 == 1 and segs["S2"][0] % 4 == 0 and segs["S3"][0] % 4 == 0
    assert segs["S5"][0] + 5 == off
    assert {at[("g", i)] % 4 for i in range(len(LAYERS))} >= {0, 2, 3}  # aligned and unaligned gains
    return off, at, segs


def _seg_tensors(pairs):
    sh = torch.tensor(pairs, dtype=torch.int64).view(-1, 2)
    return sh, sh.to(DEV)


class _AdamSide:
    """One copy of the flat p / m / v with its weight-norm outputs and table."""

    def __init__(self, p0, dtype, at):
        ops = _ops()
        n = p0.numel()
        self.n = n
        self.whole, self.view = {}, {}
        for k in ("p", "m", "v"):
            self.whole[k], self.view[k] = guarded(n)
            self.view[k].zero_()
        self.view["p"].copy_(p0.to(DEV))
        self.ents, self.outs = [], []
        for i, (kind, cout, cin, k) in enumerate(LAYERS):
            rows, cols = _rows_cols(kind, cout, cin, k)
            norm_w, norm = guarded(rows)
            wp_w, wp = guarded(cout * k * cin, dtype, pad=k * cin)  # one more packed row
            vo, go = at[("v", i)], at[("g", i)]
            self.ents.append(dict(v=self.view["p"][vo:vo + rows * cols], g=self.view["p"][go:go + rows], w_packed=wp,
                                  norm=norm, kind=kind, cout=cout, cin=cin, k=k, dtype=ops.dt_code(dtype)))
            self.outs.append((norm_w, rows, wp_w, cout * k * cin))
        self.table = ops.wn_table(self.ents)

    def poison(self):
        for norm_w, _, wp_w, _ in self.outs:
            norm_w.fill_(NAN)
            wp_w.fill_(NAN)


def _adam_inputs(seed):
    n, at, segs = _layout()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    for i, spec in enumerate(LAYERS):  # gains like weight_norm's: positive, O(1)
        rows, _ = _rows_cols(*spec)
        p0[at[("g", i)]:at[("g", i)] + rows] = torch.rand(rows, generator=gen) + 0.5
    return n, at, segs, gen, p0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_adam_step_wn_equals_adam_step_then_weight_norm_fwd(dtype):
    """vqx_adam_step_wn over one flat buffer of 79911 floats that holds the
    five layers of LAYERS (every row path of adam_wn_kernel) between flat
    segments on the scalar path (offset % 4 == 1, two blocks), the 16-B path
    (exactly one block; two blocks and a ragged 6-element tail; 3 and 5
    elements) and one empty segment, gains at offsets % 4 in {0, 2, 3}; three
    steps, each clipped (max_norm 1, gradient scales 0.01 / 3 / 0.01).  After
    every step, with torch.equal: p, m, v = a twin updated by vqx_adam_step
    over the whole range from the same hyper and sumsq; norm and w_packed of
    the Conv1d layers = vqx_weight_norm_fwd on the twin; the ConvTranspose1d
    layer's norm likewise, its w_packed untouched, and
    vqx_weight_norm_fwd_flags(NORMS_READY) on the fused side then gives the
    twin's pack.  The twin against torch.optim.Adam (CPU fp32, single-tensor)
    after the third step, 1e-6 relative as
    test_adam_step_vector_and_scalar_paths_track_torch (measured on the
    MI355X: 4.7e-10 / 0 / 3.9e-8 for p / m / v); bit equality carries that to
    the fused launch."""
    ops = _ops()
    lr, betas, eps, max_norm = 2e-4, (0.5, 0.999), 1e-8, 1.0
    n, at, segs, gen, p0 = _adam_inputs(4100)
    fused, twin = _AdamSide(p0, dtype, at), _AdamSide(p0, dtype, at)
    convt = ops.wn_table([e for e in fused.ents if e["kind"] == 1])
    seg_t = _seg_tensors([segs[s] for s in SEG_TABLE])
    g = torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    hyper, part, sumsq = torch.zeros(16, device=DEV), torch.zeros(2048, device=DEV), torch.zeros(1, device=DEV)
    pc = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pc], lr=lr, betas=betas, eps=eps, foreach=False)
    for s in range(3):
        gs = torch.randn(n, generator=gen) * (3.0 if s == 1 else 0.01)
        g.copy_(gs.to(DEV))
        ops.grad_sq_norm(g, part, sumsq)
        ops.adam_hyper(step, lr, 1.0, 10 ** 9, betas[0], betas[1], eps, hyper)
        fused.poison()
        twin.poison()
        ops.adam_step_wn(fused.view["p"], g, fused.view["m"], fused.view["v"], hyper, sumsq, max_norm, fused.table,
                         seg_t)
        ops.adam_step(twin.view["p"], g, twin.view["m"], twin.view["v"], hyper, sumsq, max_norm)
        ops.weight_norm_fwd(twin.table)
        torch.cuda.synchronize()
        assert float(sumsq.sqrt()) > max_norm, s  # the clip is active
        for k in ("p", "m", "v"):
            assert intact(fused.whole[k], n) and intact(twin.whole[k], n), (s, k)
            assert torch.equal(fused.view[k], twin.view[k]), (s, k)
        for i, (spec, fo, to) in enumerate(zip(LAYERS, fused.outs, twin.outs)):
            (norm_f, rows, wp_f, nw), (norm_t, _, wp_t, _) = fo, to
            assert intact(norm_f, rows) and intact(norm_t, rows) and intact(wp_t, nw), (s, spec)
            assert torch.equal(norm_f[:rows], norm_t[:rows]), (s, spec)
            if spec[0] == 0:
                assert intact(wp_f, nw), (s, spec)
                assert torch.equal(wp_f[:nw], wp_t[:nw]), (s, spec)
            else:
                assert bool(torch.isnan(wp_f).all()), (s, spec)  # norms only
        ops.weight_norm_fwd(convt, flags=ops.WNF_NORMS_READY)
        torch.cuda.synchronize()
        for spec, (norm_f, rows, wp_f, nw), (norm_t, _, wp_t, _) in zip(LAYERS, fused.outs, twin.outs):
            if spec[0] == 1:
                assert intact(wp_f, nw) and torch.equal(wp_f[:nw], wp_t[:nw]), (s, spec)
                assert torch.equal(norm_f[:rows], norm_t[:rows]), (s, spec)
        coef = (torch.tensor(max_norm) / (sumsq.cpu().sqrt() + 1e-6)).clamp(max=1.0)
        pc.grad = gs * coef
        opt.step()
    st = opt.state[pc]
    errs = (relerr(twin.view["p"], pc.detach()), relerr(twin.view["m"], st["exp_avg"]),
            relerr(twin.view["v"], st["exp_avg_sq"]))
    print("adam_step_wn twin vs torch.optim.Adam p/m/v:", errs)
    assert max(errs) < 1e-6, errs


def _reject_cases():
    _, _, segs = _layout()
    base = [segs[s] for s in SEG_TABLE]
    ix = {s: i for i, s in enumerate(SEG_TABLE)}

    def with_segs(**changes):
        out = list(base)
        for s, pair in changes.items():
            out[ix[s]] = pair
        return out

    s2, s3, s5 = segs["S2"], segs["S3"], segs["S5"]
    # S2 runs one element into the rows after it while S5 gives one up: the count still adds up to n
    overlap = with_segs(S2=(s2[0], s2[1] + 1), S5=(s5[0] + 1, s5[1] - 1))
    short = with_segs(S5=(s5[0], s5[1] - 1))
    pieces = [(s3[0] + 66 * i, 66) for i in range(123)] + [(s3[0] + 66 * 123, s3[1] - 66 * 123)]
    many = [p for p in base if p != s3] + pieces
    assert len(many) == 129 and sum(l for _, l in many) == sum(l for _, l in base)
    return {"overlap": dict(segs=overlap), "short": dict(segs=short), "p_offset": dict(segs=base, p_off=1),
            "cols": dict(segs=base, bad_cols=True), "segs129": dict(segs=many)}


@pytest.mark.parametrize("case", ["overlap", "short", "p_offset", "cols", "segs129"])
def test_adam_step_wn_host_rejections(case):
    """What vqx_adam_step_wn refuses on the host before any launch (the checks
    precede hipLaunchKernelGGL in csrc/vqx_optim.hip): two overlapping
    segments whose lengths still add up to n, coverage short by one element,
    p offset by one float (not 16-B aligned), a layer of 127 columns and 129
    segments.  Each raises VqxError and leaves p, m and v as they were."""
    ops = _ops()
    from vae_npvc_amd._lib import VqxError
    spec = _reject_cases()[case]
    n, at, segs, gen, p0 = _adam_inputs(4101)
    side = _AdamSide(p0, torch.float32, at)
    table = side.table
    if spec.get("bad_cols"):
        ents = [dict(e) for e in side.ents]
        ents[3]["cin"] = 127
        table = ops.wn_table(ents)
    g = (torch.randn(n + 8, generator=gen) * 0.01).to(DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    hyper, part, sumsq = torch.zeros(16, device=DEV), torch.zeros(2048, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_sq_norm(g[:n], part, sumsq)
    ops.adam_hyper(step, 2e-4, 1.0, 10 ** 9, 0.5, 0.999, 1e-8, hyper)
    before = {k: side.whole[k].clone() for k in ("p", "m", "v")}
    off = spec.get("p_off", 0)
    p = side.whole["p"][off:off + n]
    with pytest.raises(VqxError):
        ops.adam_step_wn(p, g[:n], side.view["m"], side.view["v"], hyper, sumsq, 1.0, table, _seg_tensors(spec["segs"]))
    torch.cuda.synchronize()
    for k in ("p", "m", "v"):
        assert torch.equal(side.whole[k][:n], before[k][:n]) and intact(side.whole[k], n), k
    side.poison()  # (keeps the table's tensors alive to here)


# ---- vqx_radam_hyper / vqx_radam_step

RADAM = dict(lr0=2e-4, gamma=0.5, step_size=3, b1=0.5, b2=0.999, eps=1e-8, max_norm=1.0, steps=8, big_step=4)


def _radam_hyper_ref(t):
    """hyper[0..9) of include/vqx.h in Python floats, rounded to float32."""
    c = RADAM
    lr = c["lr0"] * c["gamma"] ** ((t - 1) // c["step_size"])
    b2t = c["b2"] ** t
    nmax = 2 / (1 - c["b2"]) - 1
    nsma = nmax - 2 * t * b2t / (1 - b2t)
    rect = nsma >= 5
    if rect:
        ss = math.sqrt((1 - b2t) * (nsma - 4) / (nmax - 4) * (nsma - 2) / nsma * nmax / (nmax - 2)) / (1 - c["b1"] ** t)
    else:
        ss = 1.0 / (1 - c["b1"] ** t)
    return np.array([lr, -ss * lr, 1.0 if rect else 0.0, t, c["b1"], 1 - c["b1"], c["b2"], 1 - c["b2"], c["eps"]],
                    dtype=np.float32), lr


@pytest.mark.parametrize("n", [257, 4099])
def test_radam_hyper_and_step_track_the_oracle(n):
    """vqx_grad_sq_norm + vqx_radam_hyper + vqx_radam_step for 8 steps (betas
    (0.5, 0.999), eps 1e-8, lr 2e-4, StepLR gamma 0.5 every 3 steps: one drop
    before and one after the rectification switch at step 6; max_norm 1,
    gradient scale 3 at step 4 and 0.01 elsewhere).  hyper[0..9) of every step
    against the header's formulas in Python floats rounded to float32: equal,
    or one float32 ulp apart (device pow against Python **); measured on the
    MI355X: 0 of the 72 values differ.  hyper[2] is 0 for steps 1-5 and 1 from
    step 6, hyper[3] the step number.  p, m, v after every step against
    oracle.vqvae_cpu.ORAdam (CPU fp32, lr stepped by hand, the same clipped
    gradient) to 1e-6 relative, the Adam test's bound for the same kind of
    comparison (measured worst 9.1e-8 at n = 257, 7.8e-8 at n = 4099)."""
    ops = _ops()
    from oracle.vqvae_cpu import ORAdam
    c = RADAM
    gen = torch.Generator(device="cpu").manual_seed(600 + n)
    p0 = torch.randn(n, generator=gen)
    buf = {k: guarded(n) for k in ("p", "m", "v")}
    for k in buf:
        buf[k][1].zero_()
    buf["p"][1].copy_(p0.to(DEV))
    g = torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    part, sumsq = torch.zeros(2048, device=DEV), torch.zeros(1, device=DEV)
    pc = p0.clone().requires_grad_(True)
    opt = ORAdam([pc], lr=c["lr0"], betas=(c["b1"], c["b2"]), eps=c["eps"])
    inexact, worst = 0, 0.0
    for t in range(1, c["steps"] + 1):
        gs = torch.randn(n, generator=gen) * (3.0 if t == c["big_step"] else 0.01)
        g.copy_(gs.to(DEV))
        hyper_w, hyper = guarded(9)
        ops.grad_sq_norm(g, part, sumsq)
        ops.radam_hyper(step, c["lr0"], c["gamma"], c["step_size"], c["b1"], c["b2"], c["eps"], hyper)
        ops.radam_step(buf["p"][1], g, buf["m"][1], buf["v"][1], hyper, sumsq, c["max_norm"])
        torch.cuda.synchronize()
        assert intact(hyper_w, 9) and int(step) == t
        want, lr = _radam_hyper_ref(t)
        got = hyper.cpu().numpy()
        for i in range(9):
            near = {want[i], np.nextafter(want[i], np.float32(np.inf)), np.nextafter(want[i], np.float32(-np.inf))}
            assert got[i] in near, (t, i, got[i], want[i])
            inexact += int(got[i] != want[i])
        assert got[2] == (1.0 if t >= 6 else 0.0) and got[3] == t, (t, got)
        coef = (torch.tensor(c["max_norm"]) / (sumsq.cpu().sqrt() + 1e-6)).clamp(max=1.0)
        assert (float(coef) < 1.0) == (t == c["big_step"]), (t, float(coef))
        opt.param_groups[0]["lr"] = lr
        pc.grad = gs * coef
        opt.step()
        st = opt.state[pc]
        for k, ref in (("p", pc.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            assert intact(buf[k][0], n), (t, k)
            e = relerr(buf[k][1], ref)
            worst = max(worst, e)
            assert e < 1e-6, (t, k, e)
    print(f"radam n={n}: {inexact} of 72 hyper values not exactly equal; worst p/m/v relative error {worst:.3g}")


@pytest.mark.parametrize("t_steps", [1, 7], ids=["plain", "rectified"])
def test_radam_step_without_clipping(t_steps):
    """max_norm = 0 (sumsq given) and sumsq = NULL (max_norm 1) both give the
    unclipped update: the bits of a run whose max_norm (1e30) cannot clip, and
    ORAdam fed the raw gradient to 1e-6 relative; before (t = 1) and after
    (t = 7) the rectification switch, gradient norm ~ 190.  n = 0 returns
    without a launch and touches nothing."""
    ops = _ops()
    from oracle.vqvae_cpu import ORAdam
    c, n = RADAM, 4099
    gen = torch.Generator(device="cpu").manual_seed(77)
    p0, m0, gs = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 3.0
    v0 = torch.rand(n, generator=gen) * 0.01
    g = gs.to(DEV)
    step = torch.full((1,), t_steps - 1, dtype=torch.int64, device=DEV)
    hyper, part, sumsq = torch.zeros(16, device=DEV), torch.zeros(2048, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_sq_norm(g, part, sumsq)
    ops.radam_hyper(step, c["lr0"], c["gamma"], c["step_size"], c["b1"], c["b2"], c["eps"], hyper)
    runs = []
    for max_norm, sq in ((0.0, sumsq), (1.0, None), (1e30, sumsq)):
        buf = {k: guarded(n) for k in ("p", "m", "v")}
        for k, src in (("p", p0), ("m", m0), ("v", v0)):
            buf[k][1].copy_(src.to(DEV))
        ops.radam_step(buf["p"][1], g, buf["m"][1], buf["v"][1], hyper, sq, max_norm)
        runs.append(buf)
    torch.cuda.synchronize()
    assert float(sumsq.sqrt()) > 100.0 and float(hyper[2]) == (1.0 if t_steps >= 6 else 0.0)
    for k in ("p", "m", "v"):
        assert all(intact(r[k][0], n) for r in runs), k
        assert torch.equal(runs[0][k][1], runs[2][k][1]) and torch.equal(runs[1][k][1], runs[2][k][1]), k
    pc = p0.clone().requires_grad_(True)
    opt = ORAdam([pc], lr=_radam_hyper_ref(t_steps)[1], betas=(c["b1"], c["b2"]), eps=c["eps"])
    opt.state[pc].update(step=t_steps - 1, exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    pc.grad = gs.clone()
    opt.step()
    st = opt.state[pc]
    for k, ref in (("p", pc.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
        assert relerr(runs[0][k][1], ref) < 1e-6, k
    # n = 0
    buf = {k: guarded(0) for k in ("p", "m", "v")}
    ops.radam_step(buf["p"][1], g[:0], buf["m"][1], buf["v"][1], hyper, sumsq, 1.0)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(buf[k][0]).all()) for k in buf)
