"""`vqvae2a.Model` with `attention.{i}` on the MI355X against the reference's
float64 fixtures (tests/golden/make_golden_vqvae2a_attn.py): the training
steps of vq2a_attn_<case> with the measure and bounds of
tests/test_gpu_vqvae2a.py, the batched conversion of four utterances of
different lengths of vq2a_attn_ragged_<case> with those of
tests/test_gpu_hier_ab_ragged.py (per utterance max|got - f64| / max|f64| <=
max(8 * err32_b, 16 * 2^-23); every top-2 distance gap is >= 1e-3, so the
indices must be exact), this package's Trainer with a checkpoint round trip,
and bf16 (runs, finite, zero tails: its accuracy is tests/test_gpu_attn.py's
claim)."""
import numpy as np
import pytest
import torch

from tests.hier_model_ref import ULP16, fixture
from tests.test_gpu_hier_ab_ragged import _decode_dir, _decoder, _read_all, padded_input, per_utterance, zero_tails
from tests.test_gpu_hier_encoder import ratios, report
from tests.test_gpu_vqvae2a import batch, build_model, codebooks, record_indices, reseed, trainer

pytestmark = pytest.mark.gpu
CASES = ("ema_gst", "single_ema")
LENGTHS = [130, 70, 64, 97]
_runs = {}


@pytest.mark.parametrize("case", CASES)
def test_model_steps_match_the_float64_reference(case):
    meta, arr = fixture("vq2a_attn", case)
    assert meta["gap"] >= 1e-3
    m = build_model(meta, arr)
    assert sorted(m.attentions.keys()) == sorted(k.split(".")[1] for k in meta["arch"] if k.startswith("attention."))
    x, y = batch(arr)
    ids = []
    hooks = record_indices(m, ids)
    reseed(meta["run_seed"])
    for n in range(1, meta["steps"] + 1):
        p = f"s{n}."
        m.zero_grad(set_to_none=True)
        del ids[:]
        xhat, loss, detail = m((x, y))
        assert list(detail) == meta["loss_keys"][n - 1]
        loss.backward()
        assert len(ids) == meta["lookups"][n - 1]
        for j, idx in enumerate(ids):
            assert torch.equal(idx, torch.from_numpy(arr[p + f"idx.{j}"].copy())), (n, j)
        got = {p + "xhat": xhat.detach()}
        got.update({p + "loss." + k: torch.tensor(v, dtype=torch.float64) for k, v in detail.items()})
        got.update({p + "grad." + k: g.grad for k, g in m.named_parameters() if g.grad is not None})
        got.update({p + "buf." + k: b.detach().clone() for k, b in m.named_buffers() if b.is_floating_point()})
        assert sorted(k for k, g in m.named_parameters() if g.grad is not None) == sorted(meta["grads"])
        assert any(k.startswith("attentions.") for k in meta["grads"])
        want = {k: arr[k] for k in got if k not in meta["abs32"]}
        assert set(want) == {k for k in meta["err32"] if k.startswith(p)}
        # one frame at a level (ema_gst's top): the softmax over one key is the constant 1, so the gradients of
        # that attention's q and k linears are identically zero in the reference, in float32 too.  No relative
        # measure exists; they are bounded absolutely against the value path's gradient of the same kind, as
        # tests/test_gpu_attn.py bounds them
        zero = [k for k in want if ".mha.linear_" in k and not want[k].any()]
        for k in zero:
            assert meta["err32"][k] == 0 and ("linear_q." in k or "linear_k." in k), k
            scale = float(np.abs(arr[k.replace("linear_q.", "linear_v.").replace("linear_k.", "linear_v.")]).max())
            assert float(got[k].abs().max()) <= ULP16 * scale, k
            del want[k]
        assert (case == "ema_gst") == bool(zero)
        report(f"vq2a_attn {case} step {n}", ratios(got, want, meta["err32"]))
        for k, a32 in meta["abs32"].items():  # exactly zero in exact arithmetic
            if k.startswith(p):
                scale = float(np.abs(arr[k[:-4] + "weight"]).max())
                assert float(got[k].abs().max()) <= max(8 * a32, ULP16 * scale), k
    for h in hooks:
        h.remove()
    # encode in eval mode after the last step
    m.eval()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    codes = m.encode(x)
    got, want = {}, {}
    for i, c in enumerate(codes):
        if c.is_floating_point():
            got[f"enc.{i}"], want[f"enc.{i}"] = c, arr[f"enc.{i}"]
        else:
            assert c.dtype == torch.int64 and torch.equal(c.cpu(), torch.from_numpy(arr[f"enc.{i}"].copy())), i
    if got:
        report(f"vq2a_attn {case} encode", ratios(got, want, meta["err32"]))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


def run(case):
    """One model per ragged fixture with its codes and conversion of the zero-padded batch, computed once."""
    if case not in _runs:
        meta, arr = fixture("vq2a_attn_ragged", case)
        assert meta["lengths"] == LENGTHS and meta["gap"] >= 1e-3
        m = build_model(meta, arr)
        x = padded_input(arr, max(LENGTHS))
        y = torch.from_numpy(arr["y_tgt"].copy()).cuda()
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        r = dict(meta=meta, arr=arr, m=m, x=x, y=y, before=before)
        r["codes"] = m.encode(x, LENGTHS)
        r["out"] = m.convert((x, y), lengths=LENGTHS)
        _runs[case] = r
    return _runs[case]


@pytest.mark.parametrize("case", CASES)
def test_encode_with_lengths_gives_every_utterances_reference_codes(case):
    r = run(case)
    m, arr, codes, meta = r["m"], r["arr"], r["codes"], r["meta"]
    lv = m.level_lengths(LENGTHS)
    assert lv == meta["level_lengths"] and len(codes) == m.levels
    for i in range(m.levels):
        if m._is_style(i):
            got = {f"style.{b}": codes[i][b, :, 0] for b in range(4)}
            report(f"vq2a_attn_ragged {case} style level", ratios(got, {k: arr[k] for k in got}, meta["err32"]))
            continue
        got = codes[i].cpu()
        assert got.dtype == torch.int64 and tuple(got.shape) == (4, max(lv[i])), i
        for b, n in enumerate(lv[i]):
            assert torch.equal(got[b, :n], torch.from_numpy(arr[f"idx.{b}.{i}"].copy())), (i, b)
            assert bool((got[b, n:] == 0).all()), (i, b)


@pytest.mark.parametrize("case", CASES)
def test_convert_with_lengths_matches_each_utterances_float64_forward(case):
    r = run(case)
    out, m = r["out"], r["m"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 24, 130) and out.grad_fn is None
    report(f"vq2a_attn_ragged {case} convert fp32", per_utterance(out, r["arr"], r["meta"]))
    assert zero_tails(out)
    # NaN in the input's padding changes no bit, codes included
    xn = padded_input(r["arr"], max(LENGTHS), float("nan"))
    for a, b in zip(m.encode(xn, LENGTHS), r["codes"]):
        assert torch.equal(a, b)
    assert torch.equal(m.convert((xn, r["y"]), lengths=LENGTHS), out)
    # nothing in the state_dict changes over encode / convert
    after = m.state_dict()
    assert list(after) == list(r["before"]) and all(torch.equal(after[k], v) for k, v in r["before"].items())
    assert all(p.grad is None for p in m.parameters()) and m.training


def test_convert_without_lengths_is_the_eval_forward():
    r = run("ema_gst")
    m, arr = r["m"], r["arr"]
    x = torch.from_numpy(arr["x.2"].copy()).cuda()[None]  # 64 frames: a multiple of the down-sampling
    out = m.convert((x, r["y"][2:3]))
    got = {"xhat.2": out[0]}
    report("vq2a_attn_ragged ema_gst convert without lengths", ratios(got, {"xhat.2": arr["xhat.2"]}, r["meta"]["err32"]))
    with_len = m.convert((x, r["y"][2:3]), lengths=[64])
    report("vq2a_attn_ragged ema_gst one utterance with lengths",
           ratios({"xhat.2": with_len[0]}, {"xhat.2": arr["xhat.2"]}, r["meta"]["err32"]))


def test_trainer_steps_and_checkpoints(tmp_path):
    meta, arr = fixture("vq2a_attn", "ema_gst")
    tr = trainer(meta, arr)
    x, y = batch(arr)
    reseed(meta["run_seed"])
    start = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    totals = []
    for s in range(2):
        it, detail = tr.train_step((x, y))
        assert it == s + 1 and list(detail) == meta["loss_keys"][s] and all(np.isfinite(v) for v in detail.values())
        totals.append(detail["Total"])
    assert totals[0] != totals[1]
    now = tr.model.state_dict()
    # the optimizer walks the attention parameters too (zero gradients: every linear_k.bias, and level 2's q and k
    # linears, whose softmax runs over one frame)
    moved = [k for k in now if k.startswith(("attentions.0.", "attentions.1.")) and not k.endswith("linear_k.bias")]
    moved += [f"attentions.2.mha.linear_{n}.weight" for n in ("v", "out")]
    assert len(moved) == 16
    for k in moved:
        assert not torch.equal(now[k], start[k]), k
    before = {k: v.detach().clone() for k, v in now.items()}
    path = tmp_path / "ck.pt"
    tr.save_checkpoint(str(path))
    tr2 = trainer(meta, arr)
    assert tr2.load_checkpoint(str(path)) == 2
    for k, v in tr2.model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(q.initialized for q in codebooks(tr2.model))
    assert torch.equal(tr2.engine.exp_avg, tr.engine.exp_avg) and torch.equal(tr2.engine.exp_avg_sq, tr.engine.exp_avg_sq)
    reseed(11)
    _, d1 = tr.train_step((x, y))
    reseed(11)
    _, d2 = tr2.train_step((x, y))
    assert d1 == d2
    for (k, a), b in zip(tr.model.state_dict().items(), tr2.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_the_decode_driver_converts_batches_of_different_lengths(tmp_path):
    """decoder.hier with decode_batch_size 3 over four trials: the checkpoint with the `attentions` keys loads, and
    the written features are each utterance's conversion alone (B = 1 with its length, held to the fixture above),
    within the tolerance of tests/test_gpu_hier_ab_ragged.py's driver test."""
    meta, arr = fixture("vq2a_attn_ragged", "ema_gst")
    feats = {f"src_{n}": np.ascontiguousarray(arr[f"x.{b}"].T) for b, n in enumerate(LENGTHS)}
    data, trials = _decode_dir(tmp_path, feats, [("src_97", 0), ("src_64", 1), ("src_130", 2), ("src_70", 3)])
    dec = _decoder(tmp_path, "vq2a", meta, arr, decode_batch_size=3)
    assert sorted(dec.model.attentions.keys()) == ["0", "1", "2"]
    out = tmp_path / "out"
    out.mkdir()
    dec.decode(data, out, compress=False)
    got = _read_all(out)
    assert [k for k, _ in got] == [u for u, _, _ in trials]
    for (utt, mat), (_, f, tgt) in zip(got, trials):
        xin = torch.from_numpy(f.T.copy()).unsqueeze(0).cuda()
        ref = dec.model.convert((xin, torch.tensor([[tgt]]).cuda()), lengths=[f.shape[0]])[0].T.cpu().numpy()
        assert mat.shape == ref.shape == (f.shape[0], 24)
        assert np.linalg.norm(mat - ref) / np.linalg.norm(ref) < 1e-4, utt


def test_bf16_runs_finite_with_zero_tails():
    meta, arr = fixture("vq2a_attn", "ema_gst")
    m = build_model(meta, arr, compute_dtype="bf16")
    x, y = batch(arr)
    reseed(meta["run_seed"])
    xhat, loss, detail = m((x, y))
    loss.backward()
    assert list(detail) == meta["loss_keys"][0] and all(np.isfinite(v) for v in detail.values())
    assert bool(torch.isfinite(xhat).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    rmeta, rarr = fixture("vq2a_attn_ragged", "ema_gst")
    mr = build_model(rmeta, rarr, compute_dtype="bf16")
    xr = padded_input(rarr, max(LENGTHS), float("nan"))
    out = mr.convert((xr, torch.from_numpy(rarr["y_tgt"].copy()).cuda()), lengths=LENGTHS)
    assert tuple(out.shape) == (4, 24, 130) and bool(torch.isfinite(out).all()) and zero_tails(out)
    assert all(float(out[b, :, :n].abs().max()) > 0 for b, n in enumerate(LENGTHS))
