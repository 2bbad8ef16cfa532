"""Conversion with the hierarchical model on the MI355X: `Model.analyze`,
`synthesize` and `convert` against the reference's float64 `forward`
(tests/golden/make_golden_vqvae2_model.py: vqmodel_<case>, B = 2, T = 64, and
make_golden_vqvae2_infer.py: vqinfer_<case>, B = 1, T = 70 with a target speaker
that is not the source's), and the decode driver `decoder.hier.Decoder`.

xhat of forward((x, y')) is x rendered with y'; the codes do not depend on y.
Bound as tests/test_gpu_hier_encoder.py: max|got - f64| / max|f64| <=
max(8 * err32, 16 * 2^-23) with the fixture's err32["xhat"]; every fixture's
smallest top-2 distance gap is >= 1e-3, so the indices must be exact."""
import copy

import numpy as np
import pytest
import torch

from tests.hier_model_ref import MODEL_CASES, fixture
from tests.test_gpu_hier_encoder import ratios, report
from tests.test_gpu_hier_model import build_model

pytestmark = pytest.mark.gpu
FIXTURES = [(kind, case) for kind in ("vqmodel", "vqinfer") for case in MODEL_CASES]
_runs = {}


def quantized(m):
    """The quantized levels in the order they run (top first): the order of the fixtures' idx.{k}."""
    return [i for i in reversed(range(m.levels)) if hasattr(m.quantizers[i], "embeddings")]


def run(kind, case):
    """One model per fixture, its codes and its conversion to the fixture's target speaker; computed once,
    with gradients enabled and the parameters requiring them, as a caller that forgot no_grad would."""
    key = (kind, case)
    if key not in _runs:
        meta, arr = fixture(kind, case)
        m = build_model(meta, arr)
        x = torch.from_numpy(arr["x"].copy()).cuda()
        y = torch.from_numpy(arr["y_tgt" if kind == "vqinfer" else "y"].copy()).cuda()
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
        codes = m.analyze(x)
        out = m.convert((x, y))
        _runs[key] = dict(meta=meta, arr=arr, m=m, x=x, y=y, before=before, codes=codes, out=out)
    return _runs[key]


@pytest.mark.parametrize("kind,case", FIXTURES)
def test_analyze_gives_the_reference_indices(kind, case):
    r = run(kind, case)
    m, arr, codes = r["m"], r["arr"], r["codes"]
    B, T = r["x"].shape[0], r["x"].shape[2]
    assert r["meta"]["gap"] >= 1e-3 and isinstance(codes, list) and len(codes) == 3
    lengths = [T, {64: 16, 70: 17}[T], 1]
    for k, i in enumerate(quantized(m)):
        assert codes[i].dtype == torch.int64 and tuple(codes[i].shape) == (B, lengths[i])
        assert torch.equal(codes[i].cpu(), torch.from_numpy(arr[f"idx.{k}"].copy())), (k, i)
    if case == "gst":
        assert codes[2].dtype == torch.float32 and tuple(codes[2].shape) == (B, 32, 1)
        assert bool(torch.isfinite(codes[2]).all())
    assert not any(c.requires_grad for c in codes)


@pytest.mark.parametrize("kind,case", FIXTURES)
def test_convert_matches_the_float64_forward(kind, case):
    r = run(kind, case)
    assert tuple(r["out"].shape) == r["arr"]["xhat"].shape
    report(f"{kind} {case} convert fp32", ratios({"xhat": r["out"]}, {"xhat": r["arr"]["xhat"]}, r["meta"]["err32"]))


@pytest.mark.parametrize("kind,case", FIXTURES)
def test_synthesize_of_analyze_is_convert_and_nothing_is_modified(kind, case):
    r = run(kind, case)
    m = r["m"]
    again = m.synthesize((m.analyze(r["x"]), r["y"]))  # T from codes[0]: encoder 0 does not down-sample
    assert torch.equal(again, r["out"])
    assert torch.equal(m.synthesize((r["codes"], r["y"]), time=r["x"].shape[2]), r["out"])
    assert not r["out"].requires_grad and r["out"].grad_fn is None and not again.requires_grad
    after = m.state_dict()
    assert list(after) == list(r["before"])
    for k, v in r["before"].items():
        assert torch.equal(after[k], v), k  # forward renormalises the codebooks in place; these must not
    assert all(p.grad is None for p in m.parameters())


def test_codes_do_not_depend_on_the_speaker_and_the_output_does():
    r = run("vqinfer", "gst")
    m, arr = r["m"], r["arr"]
    y_src = torch.from_numpy(arr["y"].copy()).cuda()
    assert int(y_src) != int(r["y"])
    assert not torch.equal(m.convert((r["x"], y_src)), r["out"])


def test_ragged_length_with_a_batch_raises():
    r = run("vqinfer", "gst")
    m = r["m"]
    x2, y2 = r["x"].repeat(2, 1, 1), r["y"].repeat(2, 1)
    with pytest.raises(ValueError, match="B == 1"):
        m.analyze(x2)
    with pytest.raises(ValueError, match="B == 1"):
        m.convert((x2, y2))
    with pytest.raises(ValueError, match="without a frame"):
        m.analyze(r["x"][:, :, :15])  # the top level would keep no frame: 15 -> 7 -> 3 -> 0
    with pytest.raises(ValueError):  # Encoder.forward itself keeps refusing such a length
        m.encoders[1](torch.zeros(1, 32, 70, device="cuda"))


def test_encode_decode_infer_still_raise():
    m = run("vqmodel", "gst")["m"]
    for f in (m.encode, m.decode, m.infer):
        with pytest.raises(NotImplementedError):
            f(None)


def test_style_of_another_utterance():
    """codes from different analyze calls: utterance 0 with the style of utterance 1."""
    r = run("vqmodel", "gst")
    m, x, y = r["m"], r["x"], r["y"]
    a, b = m.analyze(x[:1]), m.analyze(x[1:])
    for i in range(2):  # one utterance alone picks the codes it picks inside the batch
        assert torch.equal(a[i], r["codes"][i][:1]) and torch.equal(b[i], r["codes"][i][1:])
    assert not torch.equal(a[2], b[2])
    plain = m.synthesize((a, y[:1]))
    mixed = m.synthesize(([a[0], a[1], b[2]], y[:1]))
    assert mixed.shape == plain.shape == (1, 24, 64) and bool(torch.isfinite(mixed).all())
    assert not torch.equal(mixed, plain)
    # slices of the batch's tensors, and an index tensor that starts 8 bytes into its buffer, work too
    want = m.synthesize((b, y[1:]))
    assert torch.equal(m.synthesize(([r["codes"][0][1:], r["codes"][1][1:], r["codes"][2][1:]], y[1:])), want)
    odd = torch.cat([b[1].new_zeros(1), b[1].reshape(-1)])[1:].view(1, -1)
    assert odd.data_ptr() % 16 == 8
    assert torch.equal(m.synthesize(([b[0], odd, b[2]], y[1:])), want)


def test_bf16_synthesize_within_autocast_error():
    """compute_dtype bf16, bounded as tests/test_gpu_hier.py and tests/test_gpu_hier_encoder.py bound bf16
    runs: relative L2 against float64 at most 1.25 x that of the plain-torch restatement under torch's CPU
    bf16 autocast on the same input.  The case is synthesize((the fixture's own indices, y')) on
    vqinfer_plain_top (B = 1, T = 70): every level is an index tensor, so bf16 cannot move an index, and
    the expected result is the fixture's float64 xhat.  The restatement is decoders[0]
    (tests/hier_ref.restated_decoder) on the stretched, normalised codebook rows, top level first, with
    the speaker embedding as conditioning; run in float32 first, it must reproduce the fixture, which
    shows that the two runs see the same input."""
    from tests.hier_ref import restated_decoder, stretch
    meta, arr = fixture("vqinfer", "plain_top")
    m = build_model(meta, arr, compute_dtype="bf16")
    T, order = meta["T"], quantized(m)
    assert order == [2, 1, 0]
    codes = [None] * 3
    for k, i in enumerate(order):
        codes[i] = torch.from_numpy(arr[f"idx.{k}"].copy()).cuda()
    y = torch.from_numpy(arr["y_tgt"].copy())
    out = m.synthesize((codes, y.cuda()))
    assert out.dtype == torch.float32 and tuple(out.shape) == arr["xhat"].shape and bool(torch.isfinite(out).all())
    params = {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}
    rows = []
    for i in order:  # top level first, as forward stacks them
        E = params[f"quantizers.{i}.embeddings"]
        En = E / E.norm(dim=1, keepdim=True)
        rows.append(stretch(En[codes[i].cpu()].transpose(1, 2), T))
    z_vq = torch.cat(rows, dim=1)
    cond = stretch(params["embeds._embedding.weight"][y[..., :1]].transpose(1, 2), T)
    dec = {k[len("decoders.0."):]: v for k, v in params.items() if k.startswith("decoders.0.")}
    want = torch.from_numpy(arr["xhat"].copy())
    l2 = lambda a: float((a.double().cpu() - want).norm() / want.norm())  # noqa: E731
    with torch.no_grad():
        f32 = restated_decoder(meta["arch"]["decoder.0"], dec, z_vq, cond)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ac = restated_decoder(meta["arch"]["decoder.0"], dec, z_vq, cond)
    hip, e_ac, e32 = l2(out), l2(ac), l2(f32)
    print(f"vqinfer plain_top synthesize bf16 rel L2 vs f64: HIP {hip:.3e}, torch autocast {e_ac:.3e} "
          f"(ratio {hip / e_ac:.3f}), restatement in float32 {e32:.3e}")
    assert e32 <= 1e-5  # the restatement's input is the fixture's
    assert hip <= 1.25 * e_ac


def test_bf16_analyze_picks_forwards_own_indices():
    """compute_dtype bf16 through analyze and convert: the output is finite, synthesize of the codes is
    convert bit for bit, and analyze picks what the same bf16 model's forward picks at every level
    (forward runs on a copy, since it renormalises the codebooks in place).  The error bound of a bf16
    run is test_bf16_synthesize_within_autocast_error's."""
    meta, arr = fixture("vqmodel", "gst")
    m = build_model(meta, arr, compute_dtype="bf16")
    x = torch.from_numpy(arr["x"].copy()).cuda()
    y = torch.from_numpy(arr["y"].copy()).cuda()
    codes = m.analyze(x)
    out = m.convert((x, y))
    assert out.dtype == torch.float32 and tuple(out.shape) == arr["xhat"].shape and bool(torch.isfinite(out).all())
    assert torch.equal(m.synthesize((codes, y), time=x.shape[2]), out)
    twin = copy.deepcopy(m)
    seen, hooks = {}, []
    for i in quantized(twin):
        hooks.append(twin.quantizers[i].register_forward_pre_hook(
            lambda mod, inp, i=i: seen.__setitem__(i, inp[0].detach().clone())))
    with torch.no_grad():
        twin((x, y))
    for h in hooks:
        h.remove()
    for i in quantized(twin):
        assert torch.equal(codes[i], twin.quantizers[i].forward_indices(seen[i])), i


# ------------------------------------------------------------------ driver
@pytest.mark.parametrize("compress", [False, True])
def test_hier_decoder_converts_trials_like_model_convert(tmp_path, compress):
    """decoder.hier.Decoder.decode over a Kaldi decode directory with trials of 64 and 70 frames, as
    tests/test_gpu_inference.py::test_decoder_converts_trials_like_oracle: the written features equal
    model.convert within that test's tolerance for compressed and uncompressed matrices."""
    from vae_npvc_amd.dataset import kaldi_io as K
    from vae_npvc_amd.decoder.hier import Decoder
    meta, arr = fixture("vqmodel", "gst")
    cfg = dict(meta["arch"], model_type="vae_npvc_amd.model.vqvae2", decoder_type="vae_npvc_amd.decoder.hier")
    sd = {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"model": sd, "iteration": 12}, ckpt)
    data = tmp_path / "eval"
    data.mkdir()
    feats = {"src_64": np.ascontiguousarray(arr["x"][0].T),
             "src_70": np.ascontiguousarray(fixture("vqinfer", "gst")[1]["x"][0].T)}
    assert [f.shape for f in feats.values()] == [(64, 24), (70, 24)]
    with K.WriteHelper(f"ark,scp:{data}/feats.ark,{data}/feats.scp") as w:
        for u, f in feats.items():
            w[u] = f
    with open(data / "trials", "w") as f:
        for i, u in enumerate(feats):
            f.write(f"{u} TGT{i}\n")
    with open(data / "spk2spk_id", "w") as f:
        for i in range(len(feats)):
            f.write(f"TGT{i} {(i * 3 + 1) % 4}\n")
    dec = Decoder(cfg)
    assert dec.load_checkpoint(str(ckpt)) == 12
    out = tmp_path / "out"
    out.mkdir()
    dec.decode(data, out, compress=compress)
    got = dict(K.ReadHelper(f"scp:{out}/feats.scp"))
    assert list(got) == list(feats)
    for i, (utt, f) in enumerate(feats.items()):
        xin = torch.from_numpy(f.T.copy()).unsqueeze(0).cuda()
        ref = dec.model.convert((xin, torch.tensor([[(i * 3 + 1) % 4]]).cuda()))[0].T.cpu().numpy()
        assert got[utt].shape == ref.shape == (f.shape[0], 24)
        err = np.linalg.norm(got[utt] - ref) / np.linalg.norm(ref)
        assert err < (5e-3 if compress else 1e-4), (utt, err)
