"""Batched conversion of utterances of different lengths with vqvae2a and
vqvae2b on the MI355X (-m gpu): `encode` / `convert` (vqvae2b: `decode` /
`infer`) with `lengths` against the reference's float64 conversion of each
utterance alone in eval mode (tests/golden/make_golden_vqvae2ab_ragged.py:
vq2a_ragged_<case>, vq2b_ragged_<case>; four utterances of 130, 70, 64 and 97
frames, a target speaker each, for vqvae2b a speaker per level), and the decode
driver with `decode_batch_size`.

Bound as tests/test_gpu_hier_ragged.py, per utterance: max|got - f64| / max|f64|
<= max(8 * err32_b, 16 * 2^-23), err32_b the reference's own float32-vs-float64
distance; every fixture's smallest top-2 distance gap is >= 1e-3, so the indices
must be exact."""
import numpy as np
import pytest
import torch

from tests.test_gpu_hier_encoder import ratios, report
from tests.test_hier_ab_ragged_host import CASES, IDS, LENGTHS, fixture, fixture_codes

pytestmark = pytest.mark.gpu
CASES_2B = [c for c in CASES if c[0] == "vq2b"]
IDS_2B = [f"{k}_{n}" for k, n in CASES_2B]
CASES_2A = [c for c in CASES if c[0] == "vq2a"]
IDS_2A = [f"{k}_{n}" for k, n in CASES_2A]
_runs = {}


def build_model(kind, case, **over):
    from vae_npvc_amd.model import vqvae2a, vqvae2b
    meta, arr = fixture(kind, case)
    m = (vqvae2a if kind == "vq2a" else vqvae2b).Model(dict(meta["arch"], **over))
    assert list(m.state_dict().keys()) == meta["keys"]
    m.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, strict=True)
    return m.cuda().train()


def padded_input(arr, T, fill=0.0):
    """(4, 24, T): the fixture's utterances, `fill` from each one's length on."""
    x = torch.full((len(LENGTHS), 24, T), fill)
    for b, n in enumerate(LENGTHS):
        x[b, :, :n] = torch.from_numpy(arr[f"x.{b}"].copy())
    return x.cuda()


def run(kind, case):
    """One model per fixture, its codes and conversions of the zero-padded batch; computed once, with gradients
    enabled, the parameters requiring them and the model in training mode, as a caller that forgot all three would."""
    key = (kind, case)
    if key not in _runs:
        meta, arr = fixture(kind, case)
        assert meta["lengths"] == LENGTHS
        m = build_model(kind, case)
        x = padded_input(arr, max(LENGTHS))
        y = torch.from_numpy(arr["y_tgt"].copy()).cuda()
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        r = dict(meta=meta, arr=arr, m=m, x=x, y=y, before=before)
        r["codes"] = m.encode(x, LENGTHS)
        r["out"] = m.convert((x, y), lengths=LENGTHS)
        if kind == "vq2b":
            r["ys"] = torch.from_numpy(arr["ys"].copy()).cuda()
            r["inf"] = m.infer((x, r["ys"]), lengths=LENGTHS)
        _runs[key] = r
    return _runs[key]


def per_utterance(out, arr, meta, tag="xhat", picks=range(4)):
    got = {f"{tag}.{b}": out[k, :, :LENGTHS[b]] for k, b in enumerate(picks)}
    return ratios(got, {k: arr[k] for k in got}, meta["err32"])


def zero_tails(out, picks=range(4)):
    return all(bool((out[k, :, LENGTHS[b]:] == 0).all()) for k, b in enumerate(picks))


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_encode_gives_every_utterances_reference_codes(kind, case):
    r = run(kind, case)
    m, arr, codes, meta = r["m"], r["arr"], r["codes"], r["meta"]
    lv = m.level_lengths(LENGTHS)
    assert lv == meta["level_lengths"] and meta["gap"] >= 1e-3 and len(codes) == m.levels
    for i in range(m.levels):
        if m._is_style(i):
            assert codes[i].dtype == torch.float32 and tuple(codes[i].shape) == (4, 32, 1)
            got = {f"style.{b}": codes[i][b, :, 0] for b in range(4)}
            report(f"{kind}_ragged {case} style level", ratios(got, {k: arr[k] for k in got}, meta["err32"]))
            continue
        assert codes[i].dtype == torch.int64 and tuple(codes[i].shape) == (4, max(lv[i])), i
        got = codes[i].cpu()
        for b, n in enumerate(lv[i]):
            assert torch.equal(got[b, :n], torch.from_numpy(arr[f"idx.{b}.{i}"].copy())), (i, b)
            assert bool((got[b, n:] == 0).all()), (i, b)
    assert not any(c.requires_grad for c in codes)


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_convert_matches_each_utterances_float64_forward(kind, case):
    r = run(kind, case)
    out = r["out"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 24, 130)
    report(f"{kind}_ragged {case} convert fp32", per_utterance(out, r["arr"], r["meta"]))
    assert zero_tails(out)  # exactly zero from each utterance's end on


@pytest.mark.parametrize("kind,case", CASES_2B, ids=IDS_2B)
def test_infer_and_decode_match_each_utterances_float64_infer(kind, case):
    r = run(kind, case)
    m, arr, meta = r["m"], r["arr"], r["meta"]
    assert r["inf"].dtype == torch.float32 and tuple(r["inf"].shape) == (4, 24, 130)
    report(f"{kind}_ragged {case} infer fp32", per_utterance(r["inf"], arr, meta, "xinf"))
    assert zero_tails(r["inf"])
    codes = [c.cuda() for c in fixture_codes(m, meta, arr)]
    for time in (None, 130):
        out = m.decode((codes, r["ys"]), time=time, lengths=torch.tensor(LENGTHS))
        assert tuple(out.shape) == (4, 24, 130) and zero_tails(out)
        report(f"{kind}_ragged {case} decode fp32 from the fixture's codes", per_utterance(out, arr, meta, "xinf"))
    # infer is decode of encode, bit for bit
    assert torch.equal(m.decode((m.encode(r["x"], LENGTHS), r["ys"]), lengths=LENGTHS), r["inf"])
    assert torch.equal(m.decode((r["codes"], r["ys"]), lengths=LENGTHS), r["inf"])


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_nothing_is_modified(kind, case):
    r = run(kind, case)
    m = r["m"]
    assert m.training and torch.is_grad_enabled() and any(p.requires_grad for p in m.parameters())
    for a, b in zip(m.encode(r["x"], LENGTHS), r["codes"]):
        assert torch.equal(a, b)
    assert torch.equal(m.convert((r["x"], r["y"]), lengths=LENGTHS), r["out"])
    outs = [r["out"]]
    if kind == "vq2b":
        assert torch.equal(m.infer((r["x"], r["ys"]), lengths=LENGTHS), r["inf"])
        outs.append(r["inf"])
    assert all(not o.requires_grad and o.grad_fn is None for o in outs)
    after = m.state_dict()
    assert list(after) == list(r["before"])
    for k, v in r["before"].items():
        assert torch.equal(after[k], v), k
    assert all(p.grad is None for p in m.parameters())
    assert m.training
    m.eval()
    try:
        assert torch.equal(m.convert((r["x"], r["y"]), lengths=LENGTHS), r["out"]) and not m.training
    finally:
        m.train()


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_padding_never_leaks(kind, case):
    """Whatever the input holds from an utterance's end on: the same shapes run the same kernels, so the
    valid frames are bit-identical to the zero-padded call's and finite, codes included."""
    r = run(kind, case)
    m = r["m"]
    for fill in (float("nan"), 1e30):
        x = padded_input(r["arr"], max(LENGTHS), fill)
        for a, b in zip(m.encode(x, LENGTHS), r["codes"]):
            assert torch.equal(a, b), fill
        out = m.convert((x, r["y"]), lengths=LENGTHS)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, r["out"]), fill
        if kind == "vq2b":
            inf = m.infer((x, r["ys"]), lengths=LENGTHS)
            assert bool(torch.isfinite(inf).all()) and torch.equal(inf, r["inf"]), fill


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_a_longer_padded_input_stays_within_the_bound(kind, case):
    """x padded to 200 frames (NaN beyond each utterance): the output has max(lengths) frames and is held to the
    fixture bound, the indices stay exact."""
    r = run(kind, case)
    m = r["m"]
    x = padded_input(r["arr"], 200, float("nan"))
    codes = m.encode(x, LENGTHS)
    for i in range(m.levels):
        if not m._is_style(i):
            assert torch.equal(codes[i], r["codes"][i]), i
    out = m.convert((x, r["y"]), lengths=LENGTHS)
    assert tuple(out.shape) == (4, 24, 130) and zero_tails(out)
    report(f"{kind}_ragged {case} convert fp32, T = 200", per_utterance(out, r["arr"], r["meta"]))
    if kind == "vq2b":
        inf = m.infer((x, r["ys"]), lengths=LENGTHS)
        assert tuple(inf.shape) == (4, 24, 130) and zero_tails(inf)
        report(f"{kind}_ragged {case} infer fp32, T = 200", per_utterance(inf, r["arr"], r["meta"], "xinf"))


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_one_utterance_with_lengths_and_a_sub_batch(kind, case):
    """B = 1 with lengths, and two of the four utterances in another order: within the bound of each."""
    r = run(kind, case)
    m, arr, meta = r["m"], r["arr"], r["meta"]
    pick = [3, 1]
    lens = [LENGTHS[b] for b in pick]
    x = r["x"][pick][:, :, :max(lens)].contiguous()
    out = m.convert((x, r["y"][pick]), lengths=lens)
    assert tuple(out.shape) == (2, 24, 97) and zero_tails(out, pick)
    report(f"{kind}_ragged {case} sub-batch", per_utterance(out, arr, meta, picks=pick))
    one = m.convert((x[:1], r["y"][3:4]), lengths=[97])
    assert tuple(one.shape) == (1, 24, 97)
    report(f"{kind}_ragged {case} B = 1", per_utterance(one, arr, meta, picks=[3]))
    if kind == "vq2b":
        inf = m.infer((x, r["ys"][pick]), lengths=lens)
        report(f"{kind}_ragged {case} infer sub-batch", per_utterance(inf, arr, meta, "xinf", pick))
        one = m.infer((r["x"][1:2, :, :70].contiguous(), r["ys"][1:2]), lengths=[70])
        report(f"{kind}_ragged {case} infer B = 1", per_utterance(one, arr, meta, "xinf", [1]))


@pytest.mark.parametrize("kind,case", [("vq2a", "ema_gst"), ("vq2b", "ema_gst")])
def test_without_lengths_convert_is_still_the_eval_mode_forward(kind, case):
    r = run(kind, case)
    m = r["m"]
    x, y = r["x"][2:3, :, :64].contiguous(), r["y"][2:3]  # 64 frames: a length forward accepts
    m.eval()
    try:
        with torch.no_grad():
            want = m((x, y))[0]
    finally:
        m.train()
    got = m.convert((x, y))
    assert torch.equal(got, want) and m.training
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in r["before"].items())
    report(f"{kind}_ragged {case} convert without lengths", per_utterance(got, r["arr"], r["meta"], picks=[2]))
    with pytest.raises(ValueError):  # and a ragged batch without lengths is still refused
        m.convert((r["x"][:, :, :70].contiguous(), r["y"]))


@pytest.mark.parametrize("kind,case", CASES_2B, ids=IDS_2B)
def test_bf16_decode_with_lengths_is_as_close_as_one_at_a_time(kind, case):
    """compute_dtype bf16, decode from the fixture's own codes (so bf16 cannot move an index): per utterance the
    relative L2 against the float64 xinf of the batched call is at most 1.25 x that of the unchanged
    one-at-a-time decode((codes_b, ys_b)) in bf16 (the margin of tests/test_gpu_hier_ragged.py's bf16 test)."""
    meta, arr = fixture(kind, case)
    m = build_model(kind, case, compute_dtype="bf16")
    lv = meta["level_lengths"]
    codes = [c.cuda() for c in fixture_codes(m, meta, arr)]
    ys = torch.from_numpy(arr["ys"].copy()).cuda()
    out = m.decode((codes, ys), lengths=LENGTHS)
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 24, 130) and bool(torch.isfinite(out).all())
    assert zero_tails(out)
    for b, T in enumerate(LENGTHS):
        alone = m.decode(([c[b:b + 1, ..., :lv[i][b]].contiguous() for i, c in enumerate(codes)], ys[b:b + 1]))
        assert tuple(alone.shape) == (1, 24, T)
        want = torch.from_numpy(arr[f"xinf.{b}"].copy())
        l2 = lambda a: float((a.double().cpu() - want).norm() / want.norm())  # noqa: E731
        batched, single = l2(out[b, :, :T]), l2(alone[0])
        print(f"{kind}_ragged {case} utterance {b} ({T} frames) decode bf16 rel L2 vs f64: batched {batched:.3e}, "
              f"one at a time {single:.3e} (ratio {batched / single:.3f})")
        assert batched <= 1.25 * single, b


@pytest.mark.parametrize("kind,case", CASES_2A, ids=IDS_2A)
def test_bf16_vqvae2a_convert_with_lengths(kind, case):
    """vqvae2a has no decode: in bf16 an index may move, so only what holds whatever the codes are."""
    meta, arr = fixture(kind, case)
    m = build_model(kind, case, compute_dtype="bf16")
    y = torch.from_numpy(arr["y_tgt"].copy()).cuda()
    out = m.convert((padded_input(arr, 130), y), lengths=LENGTHS)
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 24, 130)
    assert bool(torch.isfinite(out).all()) and zero_tails(out)
    assert torch.equal(m.convert((padded_input(arr, 130, float("nan")), y), lengths=LENGTHS), out)


# ------------------------------------------------------------------ driver
def _decode_dir(tmp_path, feats, trials):
    """A decode directory of the utterances `feats` {name: (T, 24)} and `trials` [(name, target)]:
    (directory, [(utt, features, target id)] in trial order)."""
    from vae_npvc_amd.dataset import kaldi_io as K
    data = tmp_path / "eval"
    data.mkdir()
    with K.WriteHelper(f"ark,scp:{data}/feats.ark,{data}/feats.scp") as w:
        for u, f in feats.items():
            w[u] = f
    with open(data / "trials", "w") as f:
        for u, t in trials:
            f.write(f"{u} TGT{t}\n")
    with open(data / "spk2spk_id", "w") as f:
        for t in range(4):
            f.write(f"TGT{t} {(t * 3 + 1) % 4}\n")
    return data, [(u, feats[u], (t * 3 + 1) % 4) for u, t in trials]


def _decoder(tmp_path, kind, meta, arr, **over):
    from vae_npvc_amd.decoder.hier import Decoder
    model = "vqvae2a" if kind == "vq2a" else "vqvae2b"
    cfg = dict(meta["arch"], model_type=f"vae_npvc_amd.model.{model}", decoder_type="vae_npvc_amd.decoder.hier", **over)
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"model": {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, "iteration": 12}, ckpt)
    dec = Decoder(cfg)
    assert dec.load_checkpoint(str(ckpt)) == 12
    return dec


def _read_all(path):
    from vae_npvc_amd.dataset import kaldi_io as K
    return [(line.split(None, 1)[0], np.array(K.load_mat(line.strip().split(None, 1)[1])))
            for line in open(path / "feats.scp") if line.strip()]


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("batch", [4, 3])
@pytest.mark.parametrize("kind", ["vq2a", "vq2b"])
def test_batched_decode_converts_trials_in_order(tmp_path, kind, batch, compress):
    """decode_batch_size 4 and 3 over five trials of 97, 64, 130, 97 and 70 frames: the written features equal the
    conversion of each utterance alone (B = 1 with its length, itself held to the fixture above; the path without
    lengths takes no such frame counts) within the tolerances of tests/test_gpu_hier_ragged.py's driver test."""
    meta, arr = fixture(kind, "ema_gst")
    feats = {f"src_{n}": np.ascontiguousarray(arr[f"x.{b}"].T) for b, n in enumerate(LENGTHS)}
    data, trials = _decode_dir(tmp_path, feats, [("src_97", 0), ("src_64", 1), ("src_130", 2), ("src_97", 3),
                                                 ("src_70", 0)])
    dec = _decoder(tmp_path, kind, meta, arr, decode_batch_size=batch)
    assert dec.decode_batch_size == batch
    out = tmp_path / "out"
    out.mkdir()
    dec.decode(data, out, compress=compress)
    got = _read_all(out)
    assert [k for k, _ in got] == [u for u, _, _ in trials]
    for (utt, mat), (_, f, tgt) in zip(got, trials):
        xin = torch.from_numpy(f.T.copy()).unsqueeze(0).cuda()
        ref = dec.model.convert((xin, torch.tensor([[tgt]]).cuda()), lengths=[f.shape[0]])[0].T.cpu().numpy()
        assert mat.shape == ref.shape == (f.shape[0], 24)
        err = np.linalg.norm(mat - ref) / np.linalg.norm(ref)
        assert err < (5e-3 if compress else 1e-4), (utt, err)


@pytest.mark.parametrize("kind", ["vq2a", "vq2b"])
def test_decode_batch_size_one_writes_the_one_at_a_time_bytes(tmp_path, kind):
    """decode_batch_size: 1 (and the key absent) is the loop over single utterances: the same files, byte for
    byte, as that loop written out here with model.convert and the same writer.  The utterances have 64, 128 and
    64 frames: the eval-mode forward takes multiples of the down-sampling only."""
    from vae_npvc_amd.dataset import kaldi_io as K
    meta, arr = fixture(kind, "ema_gst")
    feats = {"a64": np.ascontiguousarray(arr["x.2"].T), "b128": np.ascontiguousarray(arr["x.0"][:, :128].T),
             "c64": np.ascontiguousarray(arr["x.3"][:, :64].T)}
    data, trials = _decode_dir(tmp_path, feats, [("b128", 0), ("a64", 1), ("c64", 2), ("b128", 3)])
    outs = []
    for name, over in (("one", dict(decode_batch_size=1)), ("absent", {})):
        dec = _decoder(tmp_path, kind, meta, arr, **over)
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
