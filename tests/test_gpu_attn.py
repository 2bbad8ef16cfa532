"""SelfAttention on the MI355X against the float64 run of the reference's
MultiHeadedAttention recorded in tests/golden/attn_<case>.* (make_golden_attn.py).

fp32 bound (that of tests/test_gpu_gst.py): the kernels sum in another order
than torch's CPU GEMMs, which moves a result by the order of the reference's
own float32 rounding.  `err32` is one sample of that rounding, so it gets a
factor 8; the floor is 16 ulp, for dot products of this length:
    max|got - f64| / max|f64| <= max(8 * err32, 16 * 2^-23).
`linear_k.bias` has a mathematically zero gradient, so its bound is absolute:
    max|got| <= max(8 * abs32, 16 * 2^-23 * max|f64 dWk|).
bf16 bound (the margin tests/test_gpu_hier.py gives this package's bf16 kernels
over torch's own bf16 autocast): per tensor, relative L2 <= 1.25 * l2_bf16;
`linear_k.bias` absolutely with abs_bf16.

A gradient whose float64 value is identically zero (`zero_ref`; T = 1, where
the softmax over one key is the constant 1 and nothing reaches q and k) has no
relative measure.  Like linear_k.bias it is bounded absolutely, against the
size of the value path's gradient of the same kind (linear_v.weight for a
weight, linear_v.bias for a bias), through which the same d_ctx flows:
    fp32: max|got| <= max(8 * abs32, 16 * 2^-23 * max|f64 dWv|)
    bf16: max|got| <= max(8 * abs_bf16, 2^-8 * max|f64 dWv|)   (one bf16 rounding)

Worst ratios error / bound measured on the MI355X are in DESIGN.md
("Self-attention layer").
"""
import numpy as np
import pytest
import torch

from tests.attn_ref import CASES, KB, fixture

pytestmark = pytest.mark.gpu

ULP16 = 16 * 2.0 ** -23
RAGGED = ("ragged", "ragged64")


def build_layer(meta, arr, dtype="fp32"):
    from vae_npvc_amd.model.layers_attn import SelfAttention
    layer = SelfAttention(meta["F"], meta["H"], compute_dtype=dtype)
    layer.mha.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, strict=True)
    return layer.cuda()


def inputs(arr):
    return torch.from_numpy(arr["x"].copy()).cuda(), torch.from_numpy(arr["go"].copy()).cuda()


def run(layer, x, go, lengths, residual=False):
    """(out, dx, {key: grad}) of one forward + backward; keys as the reference's MultiHeadedAttention."""
    layer.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    out = layer(x, lengths=lengths, residual=residual)
    out.backward(go)
    return out.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in layer.mha.named_parameters()}


def _scale_of(arr, k):
    return np.abs(arr["grad.linear_k.weight" if k == KB else "grad.linear_v." + k.split(".")[1]]).max()


def ratios(meta, arr, out, dx, grads, bf16):
    """{tensor: error / bound} by the module docstring's bounds."""
    def one(got, want, k):
        d = got.double().cpu().numpy() - want
        if bf16:
            return np.linalg.norm(d) / np.linalg.norm(want) / (1.25 * meta["l2_bf16"][k])
        return np.abs(d).max() / np.abs(want).max() / max(8 * meta["err32"][k], ULP16)

    def absolute(got, k):
        floor = ULP16 if (k == KB or not bf16) else 2.0 ** -8
        bound = max(8 * meta["abs_bf16" if bf16 else "abs32"][k], floor * _scale_of(arr, k))
        top = float(got.abs().max())
        if top == 0:
            return 0.0  # an exact zero meets a zero bound
        return top / bound if bound > 0 else float("inf")

    r = {"out": one(out, arr["out"], "out"), "dx": one(dx, arr["dx"], "dx")}
    for k in meta["keys"]:
        r[k] = absolute(grads[k], k) if k == KB or k in meta["zero_ref"] else one(grads[k], arr["grad." + k], k)
    return r


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_attention_matches_the_float64_reference(case, dtype):
    meta, arr = fixture(case)
    layer = build_layer(meta, arr, dtype)
    x, go = inputs(arr)
    out, dx, grads = run(layer, x, go, meta["lengths"])
    assert out.shape == x.shape and dx.shape == x.shape and out.dtype == dx.dtype == torch.float32
    assert set(grads) == set(meta["keys"])
    r = ratios(meta, arr, out, dx, grads, dtype == "bf16")
    worst = max(r, key=r.get)
    print(f"attn {case} {dtype}: worst error/bound {r[worst]:.3f} ({worst}); "
          + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert all(np.isfinite(v) for v in r.values()), r
    assert r[worst] <= 1.0, r


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", RAGGED)
def test_padding_is_zero_out_and_never_read(case, dtype):
    meta, arr = fixture(case)
    layer = build_layer(meta, arr, dtype)
    x, go = inputs(arr)
    lens = meta["lengths"]
    out, dx, grads = run(layer, x, go, lens)
    xn, gn = x.clone(), go.clone()
    for b, n in enumerate(lens):
        assert n == x.shape[2] or (not out[b, :, n:].any() and not dx[b, :, n:].any()), b
        xn[b, :, n:] = float("nan")
        gn[b, :, n:] = float("nan")
    for residual in (False, True):
        base = (out, dx, grads) if not residual else run(layer, x, go, lens, residual=True)
        got = run(layer, xn, gn, lens, residual=residual)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), residual
        for k in grads:
            assert torch.equal(got[2][k], base[2][k]), (k, residual)
        for b, n in enumerate(lens):  # exact zeros even with the residual, whatever x holds there
            assert not got[0][b, :, n:].any() and not got[1][b, :, n:].any()


@pytest.mark.parametrize("case", RAGGED)
def test_residual_is_x_plus_forward(case):
    """fp32, valid frames: out_res = x + out and dx_res = go + dx within the bound of the float64 test."""
    meta, arr = fixture(case)
    layer = build_layer(meta, arr)
    x, go = inputs(arr)
    lens = meta["lengths"]
    out, dx, grads = run(layer, x, go, lens, residual=True)
    keep = torch.zeros_like(x)
    for b, n in enumerate(lens):
        keep[b, :, :n] = 1
    xv = (x * keep).double().cpu().numpy()
    want = {"out": arr["out"] + xv, "dx": arr["dx"] + arr["go"]}
    for name, got in (("out", out), ("dx", dx)):
        err = np.abs(got.double().cpu().numpy() - want[name]).max() / np.abs(want[name]).max()
        bound = max(8 * meta["err32"][name], ULP16)
        print(f"attn {case} residual {name}: error/bound {err / bound:.3f}")
        assert err <= bound, name
    r = ratios(meta, arr, torch.from_numpy(arr["out"].copy()), torch.from_numpy(arr["dx"].copy()), grads, False)
    assert max(r.values()) <= 1.0, r  # the parameter gradients do not see the residual


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["ragged", "multi_tile"])
def test_attention_is_deterministic(case, dtype):
    """Every output has one owner and every sum a fixed order: two runs give the same bits."""
    meta, arr = fixture(case)
    layer = build_layer(meta, arr, dtype)
    x, go = inputs(arr)
    out1, dx1, g1 = run(layer, x, go, meta["lengths"])
    out2, dx2, g2 = run(layer, x, go, meta["lengths"])
    assert torch.equal(out1, out2) and torch.equal(dx1, dx2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["one_tile", "ragged"])
def test_no_grad_and_rows_give_the_training_bits(case, dtype):
    from vae_npvc_amd import ops
    meta, arr = fixture(case)
    layer = build_layer(meta, arr, dtype)
    x, _ = inputs(arr)
    lens = meta["lengths"]
    B, F, T = x.shape
    for residual in (False, True):
        train = layer(x.clone().requires_grad_(), lengths=lens, residual=residual)
        assert train.requires_grad
        with torch.no_grad():
            quiet = layer(x, lengths=lens, residual=residual)
        assert quiet.grad_fn is None and torch.equal(train.detach(), quiet)  # nothing kept for a backward
        rows = ops.nct_to_ntc(x, torch.empty(B * T, F, device="cuda"))
        if lens is not None:  # the rows past an utterance's end are undefined on this path
            for b, n in enumerate(lens):
                rows[b * T + n:(b + 1) * T] = float("nan")
        got = layer.forward_rows(rows, B, T, lengths=lens, residual=residual)
        assert got.grad_fn is None and got.shape == (B * T, F)
        assert torch.equal(ops.ntc_to_nct(got, torch.empty_like(x)), train.detach()), residual
    layer.eval()
    for p in layer.parameters():
        p.requires_grad_(False)
    frozen = layer(x, lengths=lens)
    assert frozen.grad_fn is None and torch.equal(frozen, layer(x, lengths=lens))
