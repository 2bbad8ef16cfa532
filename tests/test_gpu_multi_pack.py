"""vqx_multi_pack on the MI355X: scattered gradient tensors copied into one
flat buffer at their offsets.  Lengths around the 4-element vector and the
4096-element chunk, a missing gradient (zero-filled), a source one float past
a 16-B boundary (destinations fall unaligned on their own after the odd
lengths), and 130 tensors, so that a second launch is needed.  It is a copy:
the result equals torch.cat bit for bit, and the NaN guard behind it stays."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 8193]
MISSING, SHIFTED = 3, 6  # the tensor of 5 elements has no gradient; the one of 4097 is a view off a 16-B boundary
GUARD = 1024


def test_pack_equals_cat_with_zeros_for_the_missing_gradient():
    from vae_npvc_amd import ops
    numels = LENGTHS + [1 + i % 7 for i in range(ops.MULTI_MAX_TENSORS + 2 - len(LENGTHS))]
    numels[ops.MULTI_MAX_TENSORS - 1] = 4097  # a multi-chunk tensor at the end of the first launch
    assert len(numels) == 130
    gen = torch.Generator(device="cuda").manual_seed(31)
    grads = []
    for i, n in enumerate(numels):
        if i == MISSING:
            grads.append(None)
        elif i == SHIFTED:
            base = torch.randn(n + 1, device="cuda", generator=gen)
            assert base.data_ptr() % 16 == 0
            grads.append(base[1:])
        else:
            grads.append(torch.randn(n, device="cuda", generator=gen))
    assert grads[SHIFTED].data_ptr() % 16 == 4 and grads[SHIFTED].is_contiguous()
    plan = ops.MultiTensorPlan(numels)
    total = sum(numels)
    buf = torch.full((total + GUARD,), float("nan"), device="cuda")
    flat = buf[:total]
    assert any((flat.data_ptr() + 4 * o) % 16 for o in plan.offsets)  # unaligned destinations
    assert any((flat.data_ptr() + 4 * o) % 16 == 0 and g is not None and g.data_ptr() % 16 == 0 and n >= 4
               for o, g, n in zip(plan.offsets, grads, numels))  # ... and tensors on the 16-B path
    plan.set_grads(grads)
    assert ops.multi_pack(plan, flat) is flat
    want = torch.cat([torch.zeros(n, device="cuda") if g is None else g for g, n in zip(grads, numels)])
    assert torch.equal(flat, want)
    assert bool(torch.isnan(buf[total:]).all())
    # packed again over the result: the same bits (nothing accumulates)
    ops.multi_pack(plan, flat)
    assert torch.equal(flat, want) and bool(torch.isnan(buf[total:]).all())


def test_pack_of_a_zero_length_tensor_and_an_empty_plan_write_nothing():
    from vae_npvc_amd import ops
    buf = torch.full((16,), float("nan"), device="cuda")
    plan = ops.MultiTensorPlan([0, 3, 0])
    g = torch.arange(3.0, device="cuda")
    plan.set_grads([torch.empty(0, device="cuda"), g, None])
    ops.multi_pack(plan, buf[:3])
    assert torch.equal(buf[:3], g) and bool(torch.isnan(buf[3:]).all())
    empty = ops.MultiTensorPlan([])
    empty.set_grads([])
    ops.multi_pack(empty, buf[:3])
    assert torch.equal(buf[:3], g)
