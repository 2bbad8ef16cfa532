"""Plain-torch restatement of the hierarchical decoder (reference vqvae2.py
Decoder.forward + Model.upsample + layers.py DeConv1d_Layernorm_GLU_ResSkip)
for the tests: conv_transpose1d, group_norm, gated unit, index-map stretch.
tests/test_hier_host.py pins it to the reference's float64 fixtures; the GPU
tests use it for shapes the fixtures do not cover."""
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import GOLD

CASES = ("tail", "dilated", "fallback", "tensor")
ULP16 = 16 * 2.0 ** -23
_cache = {}


def as_numpy(a):
    """A fresh numpy copy of an array or a (CPU / device) tensor."""
    return a.detach().cpu().numpy().copy() if torch.is_tensor(a) else np.array(a)


def fixture(case):
    """(meta, arrays) of tests/golden/vqdec_<case>; loaded once and shared read-only."""
    if case not in _cache:
        meta = json.load(open(GOLD / f"vqdec_{case}.json"))
        arr = {}
        for name in meta["files"]:
            arr.update(np.load(GOLD / name, allow_pickle=False))
        for v in arr.values():
            v.setflags(write=False)
        _cache[case] = (meta, arr)
    return _cache[case]


def fixture_cond(meta, arr):
    """The conditioning of a case: a list of level arrays, or the tensor c."""
    if meta["levels"] is None:
        return arr["c"]
    return [arr[f"level.{i}"] for i in range(len(meta["levels"]))]


def cond_names(meta):
    return ["c"] if meta["levels"] is None else [f"level.{i}" for i in range(len(meta["levels"]))]


def stretch(z, T):
    """upsample(z, T) by its index map: frame t reads min(t // (T // T_l), T_l - 1)."""
    Tl = z.shape[-1]
    r = T // Tl
    idx = torch.clamp(torch.arange(T) // r, max=Tl - 1)
    return z[..., idx]


def restated_decoder(args, params, x, cond):
    """Decoder(**args) with parameters `params` ({state_dict key: tensor}) on
    (x, cond); cond a tensor (B, cond, T) or a list of levels.  Differentiable
    in every tensor given; runs in their dtype (or under an enclosing autocast)."""
    def conv_w(pre):
        if pre + ".weight_g" in params:
            return torch._weight_norm(params[pre + ".weight_v"], params[pre + ".weight_g"], 0)
        return params[pre + ".weight"]

    T = x.shape[-1]
    c = cond if torch.is_tensor(cond) else torch.cat([stretch(z, T) for z in cond], dim=1)
    k, ks = args["kernel_size"], args["stack_kernel_size"]
    i, skips = 0, 0.0
    for cout, us, nst in zip(args["out_channels"], args["upsample_scales"], args["stacks"]):
        assert us == 1
        x = F.conv_transpose1d(x, conv_w(f"layers.{i}"), params[f"layers.{i}.bias"], padding=(k - 1) // 2)
        i += 1
        for j in range(nst):
            d = 2 ** j if args["dilation"] else 1
            pre = f"layers.{i}"
            h = F.conv_transpose1d(x, conv_w(pre + ".conv_in"), params[pre + ".conv_in.bias"],
                                   padding=(ks - 1) // 2 * d, dilation=d)
            h = h + F.conv1d(c, conv_w(pre + ".conv_cond"), params[pre + ".conv_cond.bias"])
            h = F.group_norm(h, 2, params[pre + ".norm_layer.weight"], params[pre + ".norm_layer.bias"], eps=1e-5)
            g = torch.tanh(h[:, :cout]) * torch.sigmoid(h[:, cout:])
            rs = F.conv1d(g, conv_w(pre + ".res_skip_layers"), params[pre + ".res_skip_layers.bias"])
            x = rs[:, :cout] + x
            skips = skips + rs[:, cout:]
            i += 1
    y = skips * math.sqrt(1.0 / i)
    y = F.conv1d(F.relu(y), conv_w("final_layer.1"), params["final_layer.1.bias"])
    return F.conv1d(F.relu(y), conv_w("final_layer.3"), params["final_layer.3.bias"])


def run_restated(args, sd, x, cond, go, dtype=torch.float64, autocast=False):
    """Forward + backward of the restatement on numpy / tensor inputs:
    {"out", "dx", "d<cond name>"..., "<key>" gradient...} as `dtype` CPU tensors
    (float32 parameters under torch CPU bf16 autocast when `autocast`)."""
    t = lambda a: torch.from_numpy(as_numpy(a)).to(dtype)  # noqa: E731
    params = {k: t(v).requires_grad_() for k, v in sd.items()}
    xx = t(x).requires_grad_()
    tensor_c = torch.is_tensor(cond) or isinstance(cond, np.ndarray)
    cc = t(cond).requires_grad_() if tensor_c else [t(z).requires_grad_() for z in cond]
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = restated_decoder(args, params, xx, cc)
    out.float().backward(t(go).float()) if autocast else out.backward(t(go))
    res = {"out": out.detach(), "dx": xx.grad}
    if tensor_c:
        res["dc"] = cc.grad
    else:
        for n, z in enumerate(cc):
            res[f"dlevel.{n}"] = z.grad
    res.update({k: p.grad for k, p in params.items()})
    return res


def expected(meta, arr):
    """The fixture's float64 results under run_restated's names."""
    want = {"out": arr["out"], "dx": arr["dx"]}
    want.update({"d" + n: arr["d" + n] for n in cond_names(meta)})
    want.update({k: arr["grad." + k] for k in meta["keys"]})
    return want


def fast_case(seed=9300, B=2, T=256, C=128, lens=(1, 64)):
    """The fast-kernel decoder case (T % 128 == 0, C % 128 == 0): args, a seeded
    state_dict and inputs; levels of C channels each, cond = 2C."""
    from vae_npvc_amd.model.vqvae2 import Decoder
    args = dict(in_channels=[C], out_channels=[C], upsample_scales=[1], cond_channels=C * len(lens), skip_channels=C,
                final_channels=C, kernel_size=3, dilation=True, stack_kernel_size=3, stacks=[2],
                use_weight_norm=True, use_causal_conv=False)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    dec = Decoder(**args)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    for k, v in sd.items():  # move the GroupNorm affine and the biases off their 1 / 0 / tiny initial values
        if k.endswith("norm_layer.weight"):
            v.add_(0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith("norm_layer.bias"):
            v.add_(0.2 * torch.randn(v.shape, generator=g))
    x = torch.randn(B, C, T, generator=g)
    levels = [torch.randn(B, C, Tl, generator=g) for Tl in lens]
    go = torch.randn(B, C, T, generator=g)
    return args, sd, x, levels, go
