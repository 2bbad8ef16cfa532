"""Model.encode / decode / infer of the flat model with `lengths` on the MI355X,
and the two drivers on top of them, against the committed CPU oracle
(oracle.vqvae_cpu.OracleVQVAE, eval mode) run on every utterance ALONE
(tests/flat_ragged_ref.py: seeded weights, codebook and six utterances per
case, computed once).  Never against this package's own one-at-a-time output:
a batched GEMM may run another kernel instance than a single utterance's.

Bounds, per utterance, relative L2 against the fp32 oracle:
  fp32   1e-4, the bound of test_gpu_inference.py::test_decoder_converts_trials_like_oracle
         (5e-3 after the Kaldi writer's compression, as there);
  bf16   BF16_BOUND[case] = twice the largest error of the one-at-a-time bf16
         `decode` of the commit before this feature on the same utterances
         and the oracle's ids, measured once on an MI355X: 3.5902e-3 (vcc20),
         3.4423e-3 (aishell3), 2.9020e-3 (vcc20_multi), 3.3766e-3 (vcc20_plain).
         `decode` without lengths still issues that commit's launches, and
         the bf16 test prints its figures for the record.  The factor 2 allows
         for other GEMM instances at other frame counts.
"""
import numpy as np
import pytest
import torch

from tests import flat_ragged_ref as R
from tests.helpers import NEAR_TIE

pytestmark = pytest.mark.gpu

CASES = ["vcc20", "aishell3", "vcc20_multi", "vcc20_plain"]
FP32_BOUND = 1e-4
# largest per-utterance relative L2 of the one-at-a-time bf16 decode against the fp32 oracle (see above)
BF16_MEASURED = {"vcc20": 3.5902e-3, "aishell3": 3.4423e-3, "vcc20_multi": 2.9020e-3, "vcc20_plain": 3.3766e-3}
BF16_BOUND = {k: 2.0 * v for k, v in BF16_MEASURED.items()}

_models = {}


def model(name, dtype="fp32"):
    if (name, dtype) not in _models:
        _models[name, dtype] = R.model(R.case(name), dtype)
    return _models[name, dtype]


def oracle_ids(c, order=None, width=None, fill=0):
    """The oracle's ids of the utterances `order` as a (B, width) batch, `fill` from each end up."""
    order = list(range(len(c.ids))) if order is None else list(order)
    width = width or max(len(c.ids[b]) for b in order)
    idx = torch.full((len(order), width), fill, dtype=torch.int64)
    for k, b in enumerate(order):
        idx[k, :len(c.ids[b])] = c.ids[b]
    return idx


def check_xhat(c, out, order, bound, what):
    """out (B, mel, max len) against the oracle per utterance; exact zeros from each end up."""
    lens = [c.lens[b] for b in order]
    assert tuple(out.shape) == (len(order), c.xhat[0].shape[0], max(lens)) and out.dtype == torch.float32
    for k, b in enumerate(order):
        err = R.rel_l2(out[k, :, :lens[k]], c.xhat[b])
        print(f"{what} {c.name} utterance {b} ({lens[k]} frames): rel L2 {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (what, b, err)
        assert not bool(out[k, :, lens[k]:].any()), (what, b)


@pytest.mark.parametrize("name", CASES)
def test_encode_gives_each_utterance_the_oracles_ids(name):
    c, m = R.case(name), model(name)
    assert min(float(g.min()) for g in c.gaps) >= NEAR_TIE  # no oracle near-tie: the ids must be exact
    x, lens = R.padded(c)
    idx = m.encode(x.cuda(), lengths=lens).cpu()
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (len(lens), max(lens) // c.S)
    assert torch.equal(idx, oracle_ids(c))  # zeros from T_z,b up
    assert torch.equal(m.encode(x.cuda(), lengths=torch.tensor(lens)).cpu(), idx)


@pytest.mark.parametrize("name", CASES)
def test_decode_renders_each_utterance_like_the_oracle(name):
    c, m = R.case(name), model(name)
    order = list(range(len(c.lens)))
    out = m.decode((oracle_ids(c).cuda(), c.y.cuda()), lengths=c.lens).cpu()
    check_xhat(c, out, order, FP32_BOUND, "decode")
    # entries from each utterance's end up are ignored, whatever they hold, and so is a wider index tensor
    wide = m.decode((oracle_ids(c, width=max(c.lens) // c.S + 7, fill=10 ** 6).cuda(), c.y.cuda()), lengths=c.lens)
    assert torch.equal(wide.cpu(), out)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_infer_is_decode_of_encode_and_padding_never_leaks(name, dtype):
    c, m = R.case(name), model(name, dtype)
    x, lens = R.padded(c)
    y = c.y.cuda()
    idx = m.encode(x.cuda(), lengths=lens)
    out = m.infer((x.cuda(), y), lengths=lens)
    assert torch.equal(out, m.decode((idx, y), lengths=lens))
    if dtype == "fp32":
        check_xhat(c, out.cpu(), range(len(lens)), FP32_BOUND, "infer")
    for fill in (float("nan"), 1e30):
        xf, _ = R.padded(c, fill=fill)
        assert torch.equal(m.encode(xf.cuda(), lengths=lens), idx), fill
        assert torch.equal(m.infer((xf.cuda(), y), lengths=lens), out), fill
    assert not bool(torch.isnan(out).any())


@pytest.mark.parametrize("name", CASES)
def test_longer_padding_one_utterance_and_another_order(name):
    c, m = R.case(name), model(name)
    x, lens = R.padded(c, T=200, fill=float("nan"))
    out = m.infer((x.cuda(), c.y.cuda()), lengths=lens).cpu()
    check_xhat(c, out, range(len(lens)), FP32_BOUND, "T=200")
    assert tuple(m.encode(x.cuda(), lengths=lens).shape) == (len(lens), max(lens) // c.S)
    for order in ([3], [4], [3, 0, 5], [5, 4]):
        x, lens = R.padded(c, order=order)
        y = c.y[order].cuda()
        assert torch.equal(m.encode(x.cuda(), lengths=lens).cpu(), oracle_ids(c, order))
        check_xhat(c, m.infer((x.cuda(), y), lengths=lens).cpu(), order, FP32_BOUND, f"order {order}")


@pytest.mark.parametrize("name,pad", [("vcc20", 32), ("vcc20_multi", 48)])
def test_a_rounded_frame_count_changes_no_shape_or_bound(name, pad, monkeypatch):
    """VQVAEEngine.LEN_PAD > 1 (the A/B setting of tools/flat_convert_bench.py): the batch runs at more frames
    than max(lengths) (160 for 130, 192 for 128 at S = 2), x is padded to them, and the outputs are cut back."""
    from vae_npvc_amd.engine.step import VQVAEEngine
    monkeypatch.setattr(VQVAEEngine, "LEN_PAD", pad)
    c, m = R.case(name), model(name)
    assert m.engine().len_frames(c.lens) == {"vcc20": 160, "vcc20_multi": 192}[name]
    x, lens = R.padded(c, fill=float("nan"))
    idx = m.encode(x.cuda(), lengths=lens)
    assert torch.equal(idx.cpu(), oracle_ids(c))
    out = m.infer((x.cuda(), c.y.cuda()), lengths=lens)
    assert torch.equal(out, m.decode((idx, c.y.cuda()), lengths=lens))
    check_xhat(c, out.cpu(), range(len(lens)), FP32_BOUND, f"LEN_PAD {pad}")


@pytest.mark.parametrize("name", ["vcc20", "vcc20_multi", "vcc20_plain"])
def test_no_side_effects(name):
    c = R.case(name)
    m = R.model(c)  # a model of its own: its buffers are compared
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, lens = R.padded(c)
    out = m.infer((x.cuda(), c.y.cuda()), lengths=lens)  # no torch.no_grad() around it
    idx = m.encode(x.cuda(), lengths=lens)
    assert not out.requires_grad and not idx.requires_grad
    assert all(p.grad is None for p in m.parameters())
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(before[k], after[k].cpu()) for k in before)


@pytest.mark.parametrize("name", CASES)
def test_bf16_decode_stays_within_twice_the_one_at_a_time_error(name):
    """See the module docstring for the bound's origin; prints the one-at-a-time figures it came from."""
    c, m = R.case(name), model(name, "bf16")
    alone = []
    for b, ids in enumerate(c.ids):  # the one-at-a-time decode, printed for the record (not the yardstick)
        o = m.decode((ids.view(1, -1).cuda(), c.y[b:b + 1].cuda())).cpu()
        alone.append(R.rel_l2(o[0], c.xhat[b]))
    print(f"bf16 one-at-a-time {name}: max {max(alone):.4e} per utterance {[f'{e:.3e}' for e in alone]}")
    out = m.decode((oracle_ids(c).cuda(), c.y.cuda()), lengths=c.lens).cpu()
    check_xhat(c, out, range(len(c.lens)), BF16_BOUND[name], "bf16 decode")


# ------------------------------------------------------------------ drivers
TRIALS = [(0, 5), (1, 40), (2, 77), (0, 91), (3, 12)]  # (utterance, target speaker): utterance 0 twice


def _decode_dir(tmp_path, c):
    from vae_npvc_amd.dataset import kaldi_io as K
    data = tmp_path / "eval"
    data.mkdir()
    with K.WriteHelper(f"ark,scp:{data}/feats.ark,{data}/feats.scp") as w:
        for b in sorted({b for b, _ in TRIALS}):
            w[f"src_{b}"] = c.xs[b].T.contiguous().numpy()
    (data / "trials").write_text("".join(f"src_{b} TGT{s}\n" for b, s in TRIALS))
    (data / "spk2spk_id").write_text("".join(f"TGT{s} {s}\n" for _, s in TRIALS))
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"model": c.sd, "iteration": 12}, ckpt)
    return data, ckpt


def _decoder(c, ckpt, **over):
    from vae_npvc_amd.decoder.basic import Decoder
    dec = Decoder(dict(c.cfg, **over))
    assert dec.load_checkpoint(str(ckpt)) == 12
    return dec


_trial_ref = {}


def trial_ref(c):
    """The oracle's conversion of every trial, (T, mel), computed once."""
    if not _trial_ref:
        from oracle.vqvae_cpu import OracleVQVAE
        orc = OracleVQVAE(c.cfg, c.sd)
        orc.training = False
        with torch.no_grad():
            for b, s in TRIALS:
                _trial_ref[b, s] = orc.decode(c.ids[b].view(1, -1), torch.tensor([[s]]))[0].T.numpy().copy()
    return _trial_ref


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("batch", [4, 3])
def test_batched_decode_converts_trials_like_the_oracle(tmp_path, batch, compress):
    from vae_npvc_amd.dataset import kaldi_io as K
    c = R.case("vcc20")
    data, ckpt = _decode_dir(tmp_path, c)
    dec = _decoder(c, ckpt, decode_batch_size=batch)
    assert dec.decode_batch_size == batch
    out = tmp_path / "out"
    out.mkdir()
    dec.decode(data, out, compress=compress)
    keys = [line.split()[0] for line in open(out / "feats.scp")]
    assert keys == [f"src_{b}" for b, _ in TRIALS]  # trial order, the repeated source twice
    got = [np.array(K.load_mat(line.split(None, 1)[1].strip())) for line in open(out / "feats.scp")]
    ref = trial_ref(c)
    for (b, s), g in zip(TRIALS, got):
        assert g.shape == ref[b, s].shape == (c.lens[b], 80)
        err = np.linalg.norm(g - ref[b, s]) / np.linalg.norm(ref[b, s])
        assert err < (5e-3 if compress else FP32_BOUND), (b, s, err)


def test_decode_batch_size_one_writes_the_one_at_a_time_bytes(tmp_path):
    """decode_batch_size: 1 (and the key absent) is the loop over single utterances: the same files, byte for
    byte, as that loop written out here with model.infer and the same writer."""
    from vae_npvc_amd.dataset import kaldi_io as K
    c = R.case("vcc20")
    data, ckpt = _decode_dir(tmp_path, c)
    outs = []
    for name, over in (("one", dict(decode_batch_size=1)), ("absent", {})):
        dec = _decoder(c, ckpt, **over)
        assert dec.decode_batch_size == 1
        out = tmp_path / name
        out.mkdir()
        dec.decode(data, out)
        outs.append(out)
    want = tmp_path / "want"
    want.mkdir()
    with K.WriteHelper(f"ark,scp:{want}/feats.ark,{want}/feats.scp", compression_method=1) as wf:
        for b, s in TRIALS:
            x = c.xs[b].unsqueeze(0).cuda()
            with torch.no_grad():
                wf[f"src_{b}"] = dec.model.infer((x, torch.tensor([[s]]).cuda()))[0].t().cpu().numpy()
    for out in outs:
        assert (out / "feats.ark").read_bytes() == (want / "feats.ark").read_bytes()


def test_extract_bnf_batched_matches_the_oracle_in_input_order(tmp_path):
    import yaml
    from vae_npvc_amd.bin.extract_bnf import main
    from vae_npvc_amd.dataset import kaldi_io as K
    c = R.case("vcc20")
    names = [f"utt_{b}" for b in range(len(c.xs))]  # lengths 130, 70, 64, 97, 1, 33: not sorted
    with K.WriteHelper(f"ark,scp:{tmp_path}/feats.ark,{tmp_path}/feats.scp") as w:
        for n, x in zip(names, c.xs):
            w[n] = x.T.contiguous().numpy()
    ckpt, conf = tmp_path / "ckpt.pt", tmp_path / "conf.yaml"
    torch.save({"model": c.sd, "iteration": 12}, ckpt)
    conf.write_text(yaml.safe_dump(c.cfg))
    base = ["-c", str(conf), "--model_path", str(ckpt), "--batch_size", "4"]
    assert main(base + ["--bnf_kind", "id", f"scp:{tmp_path}/feats.scp", str(tmp_path / "id.txt")]) == len(names)
    lines = [line.split() for line in open(tmp_path / "id.txt")]
    assert [u for u, _ in lines] == names
    own = {u: np.array([int(t) for t in toks.strip("<>").split("><")]) for u, toks in lines}
    for b, n in enumerate(names):
        assert np.array_equal(own[n], c.ids[b].numpy()), n
    main(base + ["--bnf_kind", "csid", f"scp:{tmp_path}/feats.scp", str(tmp_path / "cs.txt")])
    lines = [line.split() for line in open(tmp_path / "cs.txt")]
    assert [u for u, _ in lines] == names
    for u, toks in lines:
        i = own[u]
        assert [int(t) for t in toks.strip("<>").split("><")] == i[np.concatenate([[True], i[1:] != i[:-1]])].tolist()
    for kind in ("csid", "token"):
        main(base + ["--bnf_kind", kind, "--output_txt", "false", f"ark:{tmp_path}/feats.ark",
                     f"ark,scp:{tmp_path}/{kind}.ark,{tmp_path}/{kind}.scp"])
        assert [line.split()[0] for line in open(tmp_path / f"{kind}.scp")] == names
        got = dict(K.ReadHelper(f"scp:{tmp_path}/{kind}.scp"))
        for u in names:
            i = own[u]
            want = i[np.concatenate([[True], i[1:] != i[:-1]])] if kind == "csid" else i.reshape(-1, 1)
            assert np.array_equal(np.array(got[u]).reshape(want.shape), want), (kind, u)
    # the default is the loop over single utterances: the same text
    main(base[:4] + ["--bnf_kind", "id", f"scp:{tmp_path}/feats.scp", str(tmp_path / "id1.txt")])
    assert (tmp_path / "id1.txt").read_text() == (tmp_path / "id.txt").read_text()
