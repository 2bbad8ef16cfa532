"""Batched conversion of utterances of different lengths on the MI355X:
`Model.analyze` / `synthesize` / `convert` with `lengths` against the
reference's float64 `forward` of each utterance alone
(tests/golden/make_golden_vqvae2_ragged.py: vqragged_<case>, four utterances of
130, 70, 64 and 97 frames and a target speaker each), and the decode driver
with `decode_batch_size`.

Bound as tests/test_gpu_hier_infer.py, per utterance: max|got - f64| / max|f64|
<= max(8 * err32_b, 16 * 2^-23); every fixture's smallest top-2 distance gap is
>= 1e-3, so the indices must be exact."""
import numpy as np
import pytest
import torch

from tests.hier_model_ref import MODEL_CASES, fixture
from tests.test_gpu_hier_encoder import ratios, report
from tests.test_gpu_hier_infer import quantized
from tests.test_gpu_hier_model import build_model

pytestmark = pytest.mark.gpu
LENGTHS = [130, 70, 64, 97]
_runs = {}


def padded_input(arr, T, fill=0.0):
    """(4, 24, T): the fixture's utterances, `fill` from each one's length on."""
    x = torch.full((len(LENGTHS), 24, T), fill)
    for b, n in enumerate(LENGTHS):
        x[b, :, :n] = torch.from_numpy(arr[f"x.{b}"].copy())
    return x.cuda()


def run(case):
    """One model per fixture, its codes and its conversion of the zero-padded batch; computed once, with
    gradients enabled and the parameters requiring them, as a caller that forgot no_grad would."""
    if case not in _runs:
        meta, arr = fixture("vqragged", case)
        assert meta["lengths"] == LENGTHS
        m = build_model(meta, arr)
        x = padded_input(arr, max(LENGTHS))
        y = torch.from_numpy(arr["y_tgt"].copy()).cuda()
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        codes = m.analyze(x, LENGTHS)
        out = m.convert((x, y), lengths=LENGTHS)
        _runs[case] = dict(meta=meta, arr=arr, m=m, x=x, y=y, before=before, codes=codes, out=out)
    return _runs[case]


def per_utterance_ratios(out, arr, meta):
    got = {f"xhat.{b}": out[b, :, :n] for b, n in enumerate(LENGTHS)}
    return ratios(got, {k: arr[k] for k in got}, meta["err32"])


@pytest.mark.parametrize("case", MODEL_CASES)
def test_analyze_gives_every_utterances_reference_indices(case):
    r = run(case)
    m, arr, codes, meta = r["m"], r["arr"], r["codes"], r["meta"]
    lv = m.level_lengths(LENGTHS)
    assert lv == meta["level_lengths"] and meta["gap"] >= 1e-3 and len(codes) == 3
    for k, i in enumerate(quantized(m)):
        assert codes[i].dtype == torch.int64 and tuple(codes[i].shape) == (4, max(lv[i])), i
        got = codes[i].cpu()
        for b, n in enumerate(lv[i]):
            assert torch.equal(got[b, :n], torch.from_numpy(arr[f"idx.{b}.{k}"].copy())), (i, b)
            assert bool((got[b, n:] == 0).all()), (i, b)
    if case == "gst":
        assert codes[2].dtype == torch.float32 and tuple(codes[2].shape) == (4, 32, 1)
        assert bool(torch.isfinite(codes[2]).all())
    assert not any(c.requires_grad for c in codes)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_convert_matches_each_utterances_float64_forward(case):
    r = run(case)
    out = r["out"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 24, 130)
    report(f"vqragged {case} convert fp32", per_utterance_ratios(out, r["arr"], r["meta"]))
    for b, n in enumerate(LENGTHS):
        assert bool((out[b, :, n:] == 0).all()), b  # exactly zero from the utterance's end on


@pytest.mark.parametrize("case", MODEL_CASES)
def test_synthesize_of_analyze_is_convert_and_nothing_is_modified(case):
    r = run(case)
    m = r["m"]
    again = m.synthesize((m.analyze(r["x"], LENGTHS), r["y"]), lengths=LENGTHS)
    assert torch.equal(again, r["out"])
    assert torch.equal(m.synthesize((r["codes"], r["y"]), time=130, lengths=torch.tensor(LENGTHS)), r["out"])
    assert not r["out"].requires_grad and r["out"].grad_fn is None
    after = m.state_dict()
    assert list(after) == list(r["before"])
    for k, v in r["before"].items():
        assert torch.equal(after[k], v), k
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("case", MODEL_CASES)
def test_padding_never_leaks(case):
    """Whatever the input holds from an utterance's end on: the same shapes run the same kernels, so the
    valid frames are bit-identical to the zero-padded call's and finite, codes included."""
    r = run(case)
    m = r["m"]
    for fill in (float("nan"), 1e30):
        x = padded_input(r["arr"], max(LENGTHS), fill)
        codes = m.analyze(x, LENGTHS)
        for a, b in zip(codes, r["codes"]):
            assert torch.equal(a, b), fill
        out = m.convert((x, r["y"]), lengths=LENGTHS)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, r["out"]), fill


@pytest.mark.parametrize("case", MODEL_CASES)
def test_a_longer_padded_input_stays_within_the_bound(case):
    """x padded to 200 frames (NaN beyond each utterance): other frame counts, so other kernels may run; the
    output has max(lengths) frames and is held to the fixture bound, the indices stay exact."""
    r = run(case)
    m = r["m"]
    x = padded_input(r["arr"], 200, float("nan"))
    codes = m.analyze(x, LENGTHS)
    for i in quantized(m):
        assert torch.equal(codes[i], r["codes"][i]), i
    out = m.convert((x, r["y"]), lengths=LENGTHS)
    assert tuple(out.shape) == (4, 24, 130)
    report(f"vqragged {case} convert fp32, T = 200", per_utterance_ratios(out, r["arr"], r["meta"]))
    for b, n in enumerate(LENGTHS):
        assert bool((out[b, :, n:] == 0).all()), b


def test_one_utterance_with_lengths_and_a_sub_batch():
    """B = 1 with lengths, and two of the four utterances in another order: within the bound of each."""
    r = run("gst")
    m, arr, meta = r["m"], r["arr"], r["meta"]
    pick = [3, 1]
    lens = [LENGTHS[b] for b in pick]
    x = torch.zeros(2, 24, max(lens))
    for k, b in enumerate(pick):
        x[k, :, :lens[k]] = torch.from_numpy(arr[f"x.{b}"].copy())
    out = m.convert((x.cuda(), r["y"][pick]), lengths=lens)
    got = {f"xhat.{b}": out[k, :, :lens[k]] for k, b in enumerate(pick)}
    report("vqragged gst sub-batch", ratios(got, {k: arr[k] for k in got}, meta["err32"]))
    one = m.convert((x[:1, :, :97].cuda(), r["y"][3:4]), lengths=[97])
    report("vqragged gst B = 1", ratios({"xhat.3": one[0]}, {"xhat.3": arr["xhat.3"]}, meta["err32"]))
    # without lengths the batch of a ragged length is still refused, and one utterance alone still converts
    with pytest.raises(ValueError, match="B == 1"):
        m.convert((x[:, :, :70].cuda(), r["y"][pick]))
    alone = m.convert((x[1:2, :, :70].cuda(), r["y"][1:2]))
    report("vqragged gst alone, no lengths", ratios({"xhat.1": alone[0]}, {"xhat.1": arr["xhat.1"]}, meta["err32"]))


def test_bf16_synthesize_with_lengths_within_autocast_error():
    """compute_dtype bf16, the rule of tests/test_gpu_hier_infer.py::test_bf16_synthesize_within_autocast_error
    per utterance: synthesize((the fixture's own indices, y'), lengths) on vqragged_plain_top (every level an
    index tensor, so bf16 cannot move an index); relative L2 against float64 at most 1.25 x that of the
    plain-torch restatement of decoders[0] under torch's CPU bf16 autocast on the same input, which in
    float32 must reproduce the fixture."""
    from tests.hier_ref import restated_decoder, stretch
    meta, arr = fixture("vqragged", "plain_top")
    m = build_model(meta, arr, compute_dtype="bf16")
    order = quantized(m)
    assert order == [2, 1, 0]
    lv = m.level_lengths(LENGTHS)
    codes = [None] * 3
    for k, i in enumerate(order):
        c = torch.zeros(4, max(lv[i]), dtype=torch.int64)
        for b, n in enumerate(lv[i]):
            c[b, :n] = torch.from_numpy(arr[f"idx.{b}.{k}"].copy())
        codes[i] = c.cuda()
    y = torch.from_numpy(arr["y_tgt"].copy())
    out = m.synthesize((codes, y.cuda()), lengths=LENGTHS)
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 24, 130) and bool(torch.isfinite(out).all())
    params = {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}
    dec = {k[len("decoders.0."):]: v for k, v in params.items() if k.startswith("decoders.0.")}
    for b, T in enumerate(LENGTHS):
        assert bool((out[b, :, T:] == 0).all()), b
        rows = []
        for i in order:  # top level first, as forward stacks them
            E = params[f"quantizers.{i}.embeddings"]
            En = E / E.norm(dim=1, keepdim=True)
            rows.append(stretch(En[codes[i][b:b + 1, :lv[i][b]].cpu()].transpose(1, 2), T))
        z_vq = torch.cat(rows, dim=1)
        cond = stretch(params["embeds._embedding.weight"][y[b:b + 1, :1]].transpose(1, 2), T)
        want = torch.from_numpy(arr[f"xhat.{b}"].copy())
        l2 = lambda a: float((a.double().cpu() - want).norm() / want.norm())  # noqa: E731
        with torch.no_grad():
            f32 = restated_decoder(meta["arch"]["decoder.0"], dec, z_vq, cond)[0]
            with torch.autocast("cpu", dtype=torch.bfloat16):
                ac = restated_decoder(meta["arch"]["decoder.0"], dec, z_vq, cond)[0]
        hip, e_ac, e32 = l2(out[b, :, :T]), l2(ac), l2(f32)
        print(f"vqragged plain_top utterance {b} ({T} frames) synthesize bf16 rel L2 vs f64: HIP {hip:.3e}, "
              f"torch autocast {e_ac:.3e} (ratio {hip / e_ac:.3f}), restatement in float32 {e32:.3e}")
        assert e32 <= 1e-5  # the restatement's input is the fixture's
        assert hip <= 1.25 * e_ac, b


# ------------------------------------------------------------------ driver
def _decode_dir(tmp_path, arr):
    """Trials of 64, 70, 97 and 130 frames in mixed order, the 97-frame utterance listed twice under different
    targets: (directory, [(utt, features (T, 24), target id)] in trial order)."""
    from vae_npvc_amd.dataset import kaldi_io as K
    data = tmp_path / "eval"
    data.mkdir()
    feats = {f"src_{n}": np.ascontiguousarray(arr[f"x.{b}"].T) for b, n in enumerate(LENGTHS)}
    with K.WriteHelper(f"ark,scp:{data}/feats.ark,{data}/feats.scp") as w:
        for u, f in feats.items():
            w[u] = f
    trials = [("src_97", 0), ("src_64", 1), ("src_130", 2), ("src_97", 3), ("src_70", 0)]
    with open(data / "trials", "w") as f:
        for u, t in trials:
            f.write(f"{u} TGT{t}\n")
    with open(data / "spk2spk_id", "w") as f:
        for t in range(4):
            f.write(f"TGT{t} {(t * 3 + 1) % 4}\n")
    return data, [(u, feats[u], (t * 3 + 1) % 4) for u, t in trials]


def _decoder(tmp_path, meta, arr, **over):
    from vae_npvc_amd.decoder.hier import Decoder
    cfg = dict(meta["arch"], model_type="vae_npvc_amd.model.vqvae2", decoder_type="vae_npvc_amd.decoder.hier", **over)
    sd = {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"model": sd, "iteration": 12}, ckpt)
    dec = Decoder(cfg)
    assert dec.load_checkpoint(str(ckpt)) == 12
    return dec


def _read_all(path):
    """[(key, matrix)] in file order (a key may repeat)."""
    from vae_npvc_amd.dataset import kaldi_io as K
    return [(line.split(None, 1)[0], np.array(K.load_mat(line.strip().split(None, 1)[1])))
            for line in open(path / "feats.scp") if line.strip()]


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("batch", [4, 3])
def test_batched_decode_converts_trials_like_model_convert(tmp_path, batch, compress):
    """decode_batch_size 4 and 3 over five trials: the written features equal model.convert of each utterance
    alone within the tolerances of tests/test_gpu_hier_infer.py::test_hier_decoder_converts_trials_like_
    model_convert, in trial order."""
    meta, arr = fixture("vqragged", "gst")
    data, trials = _decode_dir(tmp_path, arr)
    dec = _decoder(tmp_path, meta, arr, decode_batch_size=batch)
    assert dec.decode_batch_size == batch
    out = tmp_path / "out"
    out.mkdir()
    dec.decode(data, out, compress=compress)
    got = _read_all(out)
    assert [k for k, _ in got] == [u for u, _, _ in trials]
    for (utt, mat), (_, f, tgt) in zip(got, trials):
        xin = torch.from_numpy(f.T.copy()).unsqueeze(0).cuda()
        ref = dec.model.convert((xin, torch.tensor([[tgt]]).cuda()))[0].T.cpu().numpy()
        assert mat.shape == ref.shape == (f.shape[0], 24)
        err = np.linalg.norm(mat - ref) / np.linalg.norm(ref)
        assert err < (5e-3 if compress else 1e-4), (utt, err)


def test_decode_batch_size_one_writes_the_one_at_a_time_bytes(tmp_path):
    """decode_batch_size: 1 (and the key absent) is the loop over single utterances: the same files, byte for
    byte, as that loop written out here with model.convert and the same writer."""
    from vae_npvc_amd.dataset import kaldi_io as K
    meta, arr = fixture("vqragged", "gst")
    data, trials = _decode_dir(tmp_path, arr)
    outs = []
    for name, over in (("one", dict(decode_batch_size=1)), ("absent", {})):
        dec = _decoder(tmp_path, meta, arr, **over)
        assert dec.decode_batch_size == 1
        out = tmp_path / name
        out.mkdir()
        dec.decode(data, out)
        outs.append(out)
    loop = tmp_path / "loop"
    loop.mkdir()
    with K.WriteHelper(f"ark,scp:{loop}/feats.ark,{loop}/feats.scp", compression_method=1) as w:
        for utt, f, tgt in trials:
            xin = torch.from_numpy(f.copy()).float().cuda().t().unsqueeze(0)
            w[utt] = dec.model.convert((xin, torch.tensor([tgt]).long().cuda().view(1, -1)))[0].t().cpu().numpy()
    want = (loop / "feats.ark").read_bytes()
    for out in outs:
        assert (out / "feats.ark").read_bytes() == want
    with pytest.raises(ValueError, match="decode_batch_size"):
        _decoder(tmp_path, meta, arr, decode_batch_size=0)
