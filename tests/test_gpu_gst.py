"""The style-token (GST) layer on the MI355X against the float64 run of the
reference layer recorded in tests/golden/gst_<case>.* (make_golden_gst.py).

Bound: the kernels sum in another order than torch's CPU GEMMs, which moves a
result by the order of the reference's own float32 rounding.  `err32` (the
reference's float32 run against its float64 run) is one sample of that
rounding, so it gets a factor 8; the floor is 16 ulp, for dot products of up
to 512 terms:  max|got - f64| / max|f64| <= max(8 * err32, 16 * 2^-23).
`mha.linear_k.bias` has a mathematically zero gradient, so its bound is
absolute: max|got| <= max(8 * abs32, 16 * 2^-23 * max|f64 dWk|).

Worst ratios error / bound measured on the MI355X are in DESIGN.md
("Style-token layer").
"""
import json

import numpy as np
import pytest
import torch

from tests.helpers import GOLD

pytestmark = pytest.mark.gpu

CASES = ("vae2", "default", "odd", "batch96", "saturated")
ULP16 = 16 * 2.0 ** -23
KB = "mha.linear_k.bias"
_cache = {}


def fixture(case):
    """(meta, arrays) of a case, its .npz parts merged; loaded once and shared read-only."""
    if case not in _cache:
        meta = json.load(open(GOLD / f"gst_{case}.json"))
        arr = {}
        for name in meta["files"]:
            arr.update(np.load(GOLD / name, allow_pickle=False))
        for v in arr.values():
            v.setflags(write=False)
        _cache[case] = (meta, arr)
    return _cache[case]


def build_layer(meta, arr):
    from vae_npvc_amd.model.layers_gst import StyleTokenLayer
    layer = StyleTokenLayer(ref_embed_dim=meta["R"], gst_tokens=meta["N"], gst_token_dim=meta["F"],
                            gst_heads=meta["H"])
    layer.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, strict=True)
    return layer.cuda()


def run(layer, z, go, pooled):
    """(out, dz (B, R, T), {key: grad}) through forward(z.mean(-1)) or pool_forward(z)."""
    layer.zero_grad(set_to_none=True)
    z = z.clone().requires_grad_()
    out = layer.pool_forward(z) if pooled else layer(z.mean(-1))
    out.backward(go)
    return out.detach(), z.grad.detach(), {k: p.grad.detach().clone() for k, p in layer.named_parameters()}


def ratios(meta, arr, out, dz, grads):
    """{tensor: error / bound} by the module docstring's bounds."""
    def one(got, want, err32):
        err = np.abs(got.double().cpu().numpy() - want).max() / np.abs(want).max()
        return err / max(8 * err32, ULP16)
    r = {"out": one(out, arr["out"], meta["err32"]["out"]), "dz": one(dz, arr["dz"], meta["err32"]["dz"])}
    for k in meta["keys"]:
        if k == KB:
            bound = max(8 * meta["abs32"][k], ULP16 * np.abs(arr["grad.mha.linear_k.weight"]).max())
            r[k] = float(grads[k].abs().max()) / bound
        else:
            r[k] = one(grads[k], arr["grad." + k], meta["err32"][k])
    return r


@pytest.mark.parametrize("pooled", [False, True], ids=["forward_of_mean", "pool_forward"])
@pytest.mark.parametrize("case", CASES)
def test_gst_matches_the_float64_reference(case, pooled):
    meta, arr = fixture(case)
    layer = build_layer(meta, arr)
    z, go = torch.from_numpy(arr["z"].copy()).cuda(), torch.from_numpy(arr["go"].copy()).cuda()
    out, dz, grads = run(layer, z, go, pooled)
    assert out.shape == (meta["B"], meta["F"]) and dz.shape == z.shape
    assert set(grads) == set(meta["keys"])
    r = ratios(meta, arr, out, dz, grads)
    worst = max(r, key=r.get)
    print(f"gst {case} {'pool_forward' if pooled else 'forward(mean)'}: worst error/bound {r[worst]:.3f} ({worst}); "
          + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert all(np.isfinite(v) for v in r.values()), r
    assert r[worst] <= 1.0, r


def test_gst_is_deterministic():
    """Fixed-order sums over the batch and time: two runs give the same bits."""
    meta, arr = fixture("batch96")
    layer = build_layer(meta, arr)
    z, go = torch.from_numpy(arr["z"].copy()).cuda(), torch.from_numpy(arr["go"].copy()).cuda()
    out1, dz1, g1 = run(layer, z, go, True)
    out2, dz2, g2 = run(layer, z, go, True)
    assert torch.equal(out1, out2) and torch.equal(dz1, dz2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_gst_no_grad_and_eval_give_the_training_bits():
    meta, arr = fixture("vae2")
    layer = build_layer(meta, arr)
    z = torch.from_numpy(arr["z"].copy()).cuda()
    train = layer.pool_forward(z.clone().requires_grad_())
    assert train.requires_grad
    with torch.no_grad():
        quiet = layer.pool_forward(z)
    assert not quiet.requires_grad and quiet.grad_fn is None  # nothing kept for a backward
    assert torch.equal(train.detach(), quiet)
    layer.eval()
    for p in layer.parameters():
        p.requires_grad_(False)
    frozen = layer.pool_forward(z)
    assert frozen.grad_fn is None
    assert torch.equal(train.detach(), frozen)


def test_gst_reads_rows_of_a_wider_buffer_in_place():
    """ldz > R: the first 128 columns of a 192-wide buffer give the bits of their contiguous copy."""
    from vae_npvc_amd import ops
    meta, arr = fixture("vae2")
    layer = build_layer(meta, arr)
    B, R, T, F = meta["B"], meta["R"], meta["T"], meta["F"]
    # module level (T = 1): forward() of a strided view
    wide = torch.randn(B, 192, device="cuda")
    view = wide[:, :R]
    assert view.stride(0) == 192
    with torch.no_grad():
        assert torch.equal(layer(view), layer(view.contiguous()))
    # op level with pooling (T = 4): frame-major rows of a 192-wide buffer, forward and backward
    params = tuple(p.detach() for p in layer._params())
    rows = torch.randn(B * T, 192, device="cuda")
    go = torch.from_numpy(arr["go"].copy()).cuda()
    res = []
    for zz, dz in ((rows[:, :R], torch.zeros(B * T, 192, device="cuda")[:, :R]),
                   (rows[:, :R].contiguous(), torch.zeros(B * T, R, device="cuda"))):
        ws = torch.empty(ops.gst_workspace(B, meta["N"], F, meta["H"], R, params[0].shape[1]), device="cuda")
        style = torch.empty(B, F, device="cuda")
        grads = tuple(torch.empty_like(p) for p in params)
        ops.gst_fwd(zz, T, params, meta["H"], style, ws)
        ops.gst_bwd(zz, T, params, meta["H"], go, ws, dz, grads)
        res.append((style, dz, grads))
    (s1, d1, g1), (s2, d2, g2) = res
    assert torch.equal(s1, s2) and torch.equal(d1, d2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert d1.stride(0) == 192 and not d1._base[:, R:].any()  # nothing written beside the R columns
