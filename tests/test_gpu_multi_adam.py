"""The multi-tensor optimizer pair (csrc/vqx_optim.hip: vqx_multi_sq_norm,
vqx_multi_adam_step) against the flat launches on the dense concatenation of
the same gradients, bit for bit.  Tensor lists, the smallest that reach each
branch:

A  numels 1, 3, 4, 5, 4095, 4096, 4097, 8193: the chunk edges, the 16-B tail,
   flat offsets that are no multiple of 4 (scalar path) and that are (16-B path)
B  MULTI_MAX_TENSORS + 2 tensors of 1..7 elements and one of 4097: two launch groups
C  A with every gradient a view at element offset 1, 2 or 3 of a larger
   buffer (4-B aligned only)
D  A with the 3rd and the last gradient missing

The flat p / m / v carry canary values before and after.  Runs on the MI355X
only (-m gpu)."""
import pytest
import torch

from tests.test_gpu_optim import RADAM
from tests.test_multi_tensor_host import LIST_A, list_b

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY, PAD = -1234.5, 8
CASES = ["A", "B", "C", "D"]


def _ops():
    from vae_npvc_amd import ops
    return ops


def make_case(case, seed, scale=1.0):
    """numels, the gradient list (None where missing) and the dense gradient
    (zeros where missing); C's gradients are views into `keep`."""
    ops = _ops()
    numels = list_b(ops) if case == "B" else list(LIST_A)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    grads, keep = [], []
    for i, n in enumerate(numels):
        g = (torch.randn(n, generator=gen) * scale).to(DEV)
        if case == "C":
            shift = 1 + i % 3
            buf = torch.zeros(n + 8, device=DEV)
            buf[shift:shift + n] = g
            keep.append(buf)
            g = buf[shift:shift + n]
            assert g.data_ptr() % 16 == 4 * shift and g.is_contiguous()
        grads.append(g)
    if case == "D":
        grads[2] = None
        grads[-1] = None
    dense = torch.cat([g if g is not None else torch.zeros(n, device=DEV) for g, n in zip(grads, numels)])
    return numels, grads, dense, keep


def flat_buffers(n, seed):
    """{p, m, v}: (whole, view) with PAD canaries on both sides; p random, m and v zero."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    out = {}
    for k in ("p", "m", "v"):
        whole = torch.full((n + 2 * PAD,), CANARY, device=DEV)
        view = whole[PAD:PAD + n]
        view.copy_(torch.randn(n, generator=gen).to(DEV) if k == "p" else torch.zeros(n, device=DEV))
        out[k] = (whole, view)
    return out


def canaries_intact(whole, n):
    return bool((whole[:PAD] == CANARY).all()) and bool((whole[PAD + n:] == CANARY).all())


@pytest.mark.parametrize("case", CASES)
def test_multi_sq_norm(case):
    """sumsq within 1e-6 relative of the float64 sum, two calls equal bit for
    bit (partials and total), a missing gradient contributes zeros, and an
    unaligned gradient gives the aligned one's partials."""
    ops = _ops()
    numels, grads, dense, keep = make_case(case, 31)
    plan = ops.MultiTensorPlan(numels)
    plan.set_grads(grads)
    _, first, n_part = ops.multi_layout(numels)
    runs = []
    for _ in range(2):
        whole = torch.full((n_part + 2 * PAD,), CANARY, device=DEV)
        part = whole[PAD:PAD + n_part]
        sumsq, scratch = torch.full((1,), CANARY, device=DEV), torch.zeros(256, device=DEV)
        ops.multi_sq_norm(plan, part)
        ops.sq_norm_finish(part, None, None, sumsq, scratch)
        torch.cuda.synchronize()
        assert canaries_intact(whole, n_part)
        runs.append((part.clone(), sumsq.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    want = float(dense.double().pow(2).sum())
    got = float(runs[0][1])
    print(f"multi_sq_norm {case}: relative error {abs(got - want) / want:.3g}")
    assert abs(got - want) <= 1e-6 * want
    part = runs[0][0].cpu()
    for i, (g, n) in enumerate(zip(grads, numels)):
        mine = part[first[i]:first[i] + -(-n // ops.MULTI_CHUNK)]
        if g is None:
            assert bool((mine == 0).all()), i
        else:  # each partial is its own chunk's sum
            for c in range(mine.numel()):
                w = float(g[c * ops.MULTI_CHUNK:(c + 1) * ops.MULTI_CHUNK].double().pow(2).sum())
                assert abs(float(mine[c]) - w) <= 1e-6 * w, (i, c)
    if case == "D":  # the dropped tensors would have counted
        assert float(make_case("A", 31)[2].double().pow(2).sum()) > want * (1 + 1e-3)
    if case == "C":  # the same values 16-B aligned: the same partials
        aligned = [g.clone() for g in grads]
        assert all(a.data_ptr() % 16 == 0 for a in aligned)
        plan.set_grads(aligned)
        part2 = torch.empty(n_part, device=DEV)
        ops.multi_sq_norm(plan, part2)
        assert torch.equal(part2.cpu(), part)


def _run_steps(case, kind, steps, max_norm, scales, hyper_fn):
    """`steps` optimizer steps through the multi-tensor launch and through the
    flat launch on the dense concatenation, from the same hyper and sumsq
    buffers; p, m, v compared with torch.equal after every step."""
    ops = _ops()
    numels = make_case(case, 0)[0]
    n = sum(numels)
    offsets, _, n_part = ops.multi_layout(numels)
    multi, flat = flat_buffers(n, 77), flat_buffers(n, 77)
    plan = ops.MultiTensorPlan(numels)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    hyper, sumsq = torch.zeros(16, device=DEV), torch.zeros(1, device=DEV)
    part, scratch = torch.empty(n_part, device=DEV), torch.zeros(256, device=DEV)
    flat_step = ops.radam_step if kind else ops.adam_step
    clipped = []
    for s in range(steps):
        _, grads, dense, keep = make_case(case, 100 + s, scales[s])
        plan.set_grads(grads)
        ops.multi_sq_norm(plan, part)
        ops.sq_norm_finish(part, None, None, sumsq, scratch)
        hyper_fn(step, hyper)
        before = {k: multi[k][1].clone() for k in multi}
        ops.multi_adam_step(multi["p"][1], multi["m"][1], multi["v"][1], plan, hyper, sumsq, max_norm, kind)
        flat_step(flat["p"][1], dense, flat["m"][1], flat["v"][1], hyper, sumsq, max_norm)
        torch.cuda.synchronize()
        clipped.append(float(sumsq.sqrt()) > max_norm)
        for k in ("p", "m", "v"):
            assert canaries_intact(multi[k][0], n) and canaries_intact(flat[k][0], n), (s, k)
            got, want = multi[k][1], flat[k][1]
            for i, (g, off, ni) in enumerate(zip(grads, offsets, numels)):
                if g is None:  # untouched, while the flat twin moved it with a zero gradient
                    assert torch.equal(got[off:off + ni], before[k][off:off + ni]), (s, k, i)
                    want[off:off + ni] = got[off:off + ni]
            assert torch.equal(got, want), (s, k)
        assert not bool(torch.equal(multi["p"][1], before["p"]))
    return clipped


@pytest.mark.parametrize("clip", [True, False], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("case", CASES)
def test_multi_adam_equals_adam_step_on_the_concatenation(case, clip):
    """Three consecutive steps, StepLR dropping the rate at the third; max_norm
    0.5 clips every step (gradient norms of 60 and more), 1e6 clips none."""
    ops = _ops()
    max_norm = 0.5 if clip else 1e6
    clipped = _run_steps(case, 0, 3, max_norm, [1.0, 3.0, 1.0],
                         lambda step, hyper: ops.adam_hyper(step, 1e-3, 0.5, 2, 0.5, 0.999, 1e-8, hyper))
    assert clipped == [clip] * 3


@pytest.mark.parametrize("case", CASES)
def test_multi_radam_equals_radam_step_on_the_concatenation(case):
    """The 8 steps of tests/test_gpu_optim.py's RADAM case (the rectification
    switches on at step 6; the gradient scale is 3 at step 4, which clips, and
    0.004 elsewhere, which at these lengths does not)."""
    ops = _ops()
    c = RADAM
    scales = [3.0 if t == c["big_step"] else 0.004 for t in range(1, c["steps"] + 1)]
    clipped = _run_steps(case, 1, c["steps"], c["max_norm"], scales,
                         lambda step, hyper: ops.radam_hyper(step, c["lr0"], c["gamma"], c["step_size"], c["b1"],
                                                             c["b2"], c["eps"], hyper))
    assert clipped[c["big_step"] - 1] and not clipped[0]
