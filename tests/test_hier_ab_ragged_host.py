"""vqvae2a / vqvae2b batched conversion of different lengths, host side (no
GPU): `level_lengths` against the six fixtures of
tests/golden/make_golden_vqvae2ab_ragged.py, the validation that runs before
the device is touched (ValueError; valid arguments on CPU tensors then raise
VqxError, and nothing is written), the signatures, the two new ops wrappers
and the bench tool's --model option."""
import inspect
import json

import numpy as np
import pytest
import torch

from tests.helpers import GOLD

CASES = [("vq2a", n) for n in ("ema_gst", "plain_shared", "single_ema")] + \
        [("vq2b", n) for n in ("ema_gst", "plain_last", "pooled_ema")]
IDS = [f"{k}_{n}" for k, n in CASES]
LENGTHS = [130, 70, 64, 97]
_cache = {}


def fixture(kind, case):
    key = f"{kind}_ragged_{case}"
    if key not in _cache:
        meta = json.load(open(GOLD / f"{key}.json"))
        arr = {}
        for name in meta["files"]:
            arr.update(np.load(GOLD / name, allow_pickle=False))
        for v in arr.values():
            v.setflags(write=False)
        _cache[key] = (meta, arr)
    return _cache[key]


def cpu_model(kind, case, **over):
    from vae_npvc_amd.model import vqvae2a, vqvae2b
    meta, arr = fixture(kind, case)
    m = (vqvae2a if kind == "vq2a" else vqvae2b).Model(dict(meta["arch"], **over))
    assert list(m.state_dict().keys()) == meta["keys"]
    m.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, strict=True)
    return m, meta, arr


def padded_input(arr, T, fill=0.0):
    x = torch.full((len(LENGTHS), 24, T), fill)
    for b, n in enumerate(LENGTHS):
        x[b, :, :n] = torch.from_numpy(arr[f"x.{b}"].copy())
    return x


def fixture_codes(m, meta, arr, picks=range(4)):
    """The fixture's codes as encode(x, lengths) returns them for the utterances `picks`."""
    lv, codes = meta["level_lengths"], []
    for i in range(m.levels):
        if m._is_style(i):
            codes.append(torch.stack([torch.from_numpy(arr[f"style.{b}"].copy()).float() for b in picks]).unsqueeze(-1))
        else:
            c = torch.zeros(len(picks), max(lv[i][b] for b in picks), dtype=torch.int64)
            for k, b in enumerate(picks):
                c[k, :lv[i][b]] = torch.from_numpy(arr[f"idx.{b}.{i}"].copy())
            codes.append(c)
    return codes


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_level_lengths_equal_the_fixtures(kind, case):
    m, meta, _ = cpu_model(kind, case)
    assert meta["lengths"] == LENGTHS and meta["gap"] >= 1e-3 and meta["top_rule"] == "absolute"
    assert m.level_lengths(LENGTHS) == meta["level_lengths"]
    assert m.level_lengths(torch.tensor(LENGTHS)) == meta["level_lengths"]
    assert m.level_lengths([64]) == [lv[2:3] for lv in meta["level_lengths"]]


def test_an_utterance_too_short_for_a_level_is_named():
    m, _, _ = cpu_model("vq2a", "ema_gst")  # level 1 divides by 4, level 2 by 16 more
    with pytest.raises(ValueError, match=r"utterance 1 of 3 frames leaves level 1 without a frame"):
        m.level_lengths([130, 3, 64])
    with pytest.raises(ValueError, match=r"utterance 2 of 20 frames leaves level 2 without a frame"):
        m.level_lengths([130, 64, 20])
    m, _, _ = cpu_model("vq2b", "pooled_ema")  # the pooled top still needs a frame to pool
    with pytest.raises(ValueError, match=r"utterance 0 of 2 frames leaves level 1 without a frame"):
        m.level_lengths([2, 64])


@pytest.mark.parametrize("kind,case", [("vq2a", "ema_gst"), ("vq2a", "plain_shared"), ("vq2b", "ema_gst"),
                                       ("vq2b", "pooled_ema")])
def test_bad_lengths_are_refused_before_the_device(kind, case):
    from vae_npvc_amd._lib import VqxError
    m, meta, arr = cpu_model(kind, case)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    x, y = padded_input(arr, 130), torch.from_numpy(arr["y_tgt"].copy())
    calls = [lambda n: m.encode(x, n), lambda n: m.convert((x, y), lengths=n)]
    if kind == "vq2b":
        ys = torch.from_numpy(arr["ys"].copy())
        calls.append(lambda n: m.infer((x, ys), lengths=n))
    bad = [[130, 70, 64], [130, 70, 64, 97, 5], [130, 0, 64, 97], [131, 70, 64, 97], [130, 70, 64, -1],
           torch.tensor([130.0, 70.0, 64.0, 97.0]), [130, 70, 64, 97.0], torch.tensor([[130, 70, 64, 97]]),
           [130, 70, 64, True], [130, 70, 64, 3]]
    for call in calls:
        for n in bad:
            with pytest.raises(ValueError):
                call(n)
        with pytest.raises(VqxError, match="MI355X"):  # valid arguments, CPU tensors: after the host checks
            call(LENGTHS)
        with pytest.raises(VqxError, match="MI355X"):
            call(torch.tensor(LENGTHS, dtype=torch.int32))
    with pytest.raises(ValueError, match="x must be"):
        m.encode(x[:, :20], LENGTHS)
    with pytest.raises(ValueError, match="y_idx"):
        m.convert((x, y[:3]), lengths=LENGTHS)
    with pytest.raises(ValueError, match="y_idx"):
        m.convert((x, y.float()), lengths=LENGTHS)
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())


class _CudaTyped(torch.Tensor):
    """A CPU tensor that reports itself as a device tensor: what `lengths` must never be."""
    is_cuda = True


def test_a_device_typed_lengths_tensor_is_refused():
    m, _, arr = cpu_model("vq2b", "ema_gst")
    x, y = padded_input(arr, 130), torch.from_numpy(arr["y_tgt"].copy())
    n = torch.tensor(LENGTHS).as_subclass(_CudaTyped)
    assert n.is_cuda
    for call in (lambda: m.encode(x, n), lambda: m.convert((x, y), lengths=n), lambda: m.level_lengths(n),
                 lambda: m.infer((x, torch.from_numpy(arr["ys"].copy())), lengths=n)):
        with pytest.raises(ValueError, match="never a device tensor"):
            call()


@pytest.mark.parametrize("case", ["ema_gst", "plain_last", "pooled_ema"])
def test_vqvae2b_decode_validates_codes_on_the_host(case):
    from vae_npvc_amd._lib import VqxError
    m, meta, arr = cpu_model("vq2b", case)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    codes, ys = fixture_codes(m, meta, arr), torch.from_numpy(arr["ys"].copy())

    def swap(i, c):
        return [c if k == i else z for k, z in enumerate(codes)]
    bad = [
        dict(zs=codes[:-1]), dict(zs=codes, time=129), dict(zs=codes, time=200),
        dict(zs=swap(0, codes[0][:, :100])), dict(zs=swap(0, torch.zeros(4, 131, dtype=torch.int64))),
        dict(zs=swap(0, codes[0].int())), dict(zs=swap(0, codes[0].float())), dict(zs=swap(0, codes[0][:3])),
        dict(zs=swap(0, codes[0].unsqueeze(1))),
        dict(zs=swap(0, codes[0] + 16)), dict(zs=swap(0, codes[0] - 17)),  # the codebooks hold 0..15
        dict(zs=codes, ys=ys[:, :1]), dict(zs=codes, ys=ys.float()), dict(zs=codes, ys=ys + 4), dict(zs=codes, ys=ys[:3]),
        dict(zs=codes, lengths=[130, 70, 64]), dict(zs=codes, lengths=[130, 70, 64, 0]),
        dict(zs=codes, lengths=[130, 70, 64, 96.0]), dict(zs=codes, lengths=[129, 70, 64, 97]),
    ]
    top = m.levels - 1
    if m._is_style(top):
        bad += [dict(zs=swap(top, codes[top].squeeze(-1))), dict(zs=swap(top, codes[top].long())),
                dict(zs=swap(top, codes[top].expand(-1, -1, 2))), dict(zs=swap(top, codes[top][:, :16]))]
    else:
        bad += [dict(zs=swap(top, torch.cat([codes[top], codes[top]], 1)))]
    for kw in bad:
        kw = dict(dict(ys=ys, time=None, lengths=LENGTHS), **kw)
        with pytest.raises(ValueError):
            m.decode((kw["zs"], kw["ys"]), time=kw["time"], lengths=kw["lengths"])
    for time in (None, 130):
        with pytest.raises(VqxError, match="MI355X"):
            m.decode((codes, ys), time=time, lengths=LENGTHS)
    with pytest.raises(ValueError, match="ys must be"):
        m.infer((padded_input(arr, 130), ys[:, :1]), lengths=LENGTHS)
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())


def test_signatures():
    from vae_npvc_amd.model import vqvae2a, vqvae2b
    from vae_npvc_amd.model.hier_base import HierModelBase
    sig = lambda f: inspect.signature(f).parameters  # noqa: E731
    for f in (HierModelBase.encode, HierModelBase.convert, vqvae2b.Model.decode, vqvae2b.Model.infer,
              vqvae2a.Model.encode, vqvae2a.Model.convert, vqvae2b.Model.encode, vqvae2b.Model.convert):
        assert sig(f)["lengths"].default is None, f
    assert list(sig(vqvae2b.Model.decode)) == ["self", "input", "time", "lengths"]
    assert list(sig(vqvae2a.Model.infer)) == ["self", "input"]
    assert list(sig(vqvae2a.Model.decode)) == ["self", "input", "time"]
    assert callable(HierModelBase.level_lengths)
    m, _, arr = cpu_model("vq2a", "ema_gst")
    with pytest.raises(NotImplementedError, match="undefined `x`"):
        m.decode(([], None))
    with pytest.raises(NotImplementedError, match="undefined `x`"):
        m.infer((padded_input(arr, 130), None))


def test_the_two_entry_points_are_declared_and_exported():
    import re

    from vae_npvc_amd import _lib as L
    from tests.helpers import ROOT
    header = (ROOT / "include" / "vqx.h").read_text()
    lib = L.load()
    for fn in ("vqx_nct_to_ntc_pad_len", "vqx_index_mask_len"):
        assert re.search(rf"\bint {fn}\(", header) and hasattr(lib, fn) and fn in L._SIGS and fn in L.EXPORTS, fn
    assert L.ABI_VERSION == 130 and lib.vqx_version() == 130
    assert len(L._SIGS["vqx_nct_to_ntc_pad_len"]) == 10 and len(L._SIGS["vqx_index_mask_len"]) == 7


def test_ops_wrappers_refuse_bad_shapes_and_dtypes():
    from vae_npvc_amd import ops
    x, y = torch.zeros(2, 8, 6), torch.zeros(16, 8)
    bad = [(x[0], 8, [6, 5], y), (x.double(), 8, [6, 5], y), (x.transpose(1, 2), 8, [6, 5], y), (x, 5, [6, 5], y),
           (x, 8.0, [6, 5], y), (x, True, [6, 5], y), (x, 8, [6], y), (x, 8, [6, 5.0], y), (x, 8, [6, 5], y[:12]),
           (x, 8, [6, 5], torch.zeros(16, 4)), (x, 8, [6, 5], y.half()), (x, 8, [6, 5], y.t().contiguous().t()),
           (x, 8, [6, 5], y.view(2, 8, 8))]
    for args in bad:
        with pytest.raises(ValueError):
            ops.nct_to_ntc_pad_len(*args)
    idx, out = torch.zeros(3, 5, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int64)
    bad = [(idx.int(), [4, 1, 3], out), (idx.view(-1), [4, 1, 3], out), (idx.t(), [4, 1, 3], out.t()),
           (idx, [4, 1, 3], out.int()), (idx, [4, 1, 3], out[:2]), (idx, [4, 1, 3], torch.zeros(3, 6, dtype=torch.int64)),
           (idx, [4, 1, 3], torch.zeros(3, 0, dtype=torch.int64)), (idx, [4, 1], out), (idx, [4, 1, 3.0], out),
           (idx, torch.tensor([4.0, 1.0, 3.0]), out)]
    for args in bad:
        with pytest.raises(ValueError):
            ops.index_mask_len(*args)
    with pytest.raises(ops.L.VqxError):  # no CPU path
        ops.nct_to_ntc_pad_len(x, 8, [6, 5], y)
    with pytest.raises(ops.L.VqxError):
        ops.index_mask_len(idx, [4, 1, 3], out)


def test_bench_tool_model_option_parses():
    import importlib.util

    from tests.helpers import ROOT
    spec = importlib.util.spec_from_file_location("hier_convert_bench", ROOT / "tools" / "hier_convert_bench.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ap = tool.parser()
    assert ap.parse_args([]).model == "vqvae2"
    for name in ("vqvae2", "vqvae2a", "vqvae2b"):
        assert ap.parse_args(["--model", name]).model == name
        arch = tool.model_arch(name, "bf16")
        assert arch["compute_dtype"] == "bf16" and arch["levels"] == 3
    with pytest.raises(SystemExit):
        ap.parse_args(["--model", "vqvae"])
    a, b = tool.model_arch("vqvae2a", "fp32"), tool.model_arch("vqvae2b", "fp32")
    assert a["use_ema"] is True and b["use_ema"] is True
    assert all(b[f"decoder.{i}"]["final_channels"] == 128 for i in range(3))
    assert not b["final_decoder"].get("cond_channels") and b["final_decoder"]["in_channels"] == [384]
