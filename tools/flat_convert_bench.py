"""Utterances per second of the flat model's two inference drivers over a
synthetic directory, at batch size 1 (the loop over single utterances) and a
few larger values:

  decode  `decoder.basic.Decoder.decode` with conf/vcc20.yaml's model, by
          `decode_batch_size`;
  token   `bin.extract_bnf` (`--bnf_kind id`, text output) with
          conf/aishell3.yaml's model, by `--batch_size`.

The directory: TRIALS trials over TRIALS // 3 source utterances (every source
is converted to three target speakers; the token part reads the sources of the
trials in trial order, so it encodes TRIALS utterances too), lengths drawn
uniformly from LEN_LO..LEN_HI frames with a fixed seed, listed in shuffled
order.  The weights are the seeded initial ones: the time of a conversion does
not depend on their values.

One timed window is one whole run over the directory: reading the features,
the model calls, the read-back and the writer (compressed Kaldi matrices for
decode, text for token).  Device events around the call (it ends with a
read-back, so the host clock would serve as well); the sizes alternate inside
every round, WINDOWS rounds after one warm-up run each; median and range of
utterances per second.  Every size's output is compared with size 1's before it
is timed: the largest relative L2 over the trials (decode), the share of equal
ids (token).

On a tree whose drivers take no batch size only size 1 is measured (the
baseline: size 1 must reproduce it).  `--len-pad N` sets the engine's LEN_PAD
(frames the padded T of a batch is rounded up to) for an A/B run.  A lab
script, no pass/fail bar.
Usage (GPU box): python tools/flat_convert_bench.py [--json OUT] [--dtype bf16] [--sizes 1,4,8,16,32]
                 [--part decode|token|both] [--len-pad 1]"""
import argparse
import inspect
import json
import os
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from vae_npvc_amd.bin import extract_bnf  # noqa: E402
from vae_npvc_amd.dataset import kaldi_io as K  # noqa: E402
from vae_npvc_amd.decoder.basic import Decoder  # noqa: E402

TRIALS, LEN_LO, LEN_HI, SEED = 96, 150, 650, 20
WINDOWS = 5


def config(name, dtype):
    cfg = yaml.safe_load(open(Path(ROOT) / "vae_npvc_amd" / "conf" / f"{name}.yaml"))
    cfg["compute_dtype"] = dtype
    return cfg


def make_dir(root, mel, speakers):
    """The synthetic decode directory; returns (path, the trials' lengths in trial order)."""
    rng = np.random.default_rng(SEED)
    data = Path(root) / "eval"
    data.mkdir()
    n_src = TRIALS // 3
    lens = rng.integers(LEN_LO, LEN_HI + 1, n_src)
    with K.WriteHelper(f"ark,scp:{data}/feats.ark,{data}/feats.scp") as w:
        for u in range(n_src):
            w[f"utt{u:03d}"] = rng.standard_normal((int(lens[u]), mel)).astype(np.float32)
    trials = [(u, int(rng.integers(0, speakers))) for u in range(n_src) for _ in range(3)]
    order = rng.permutation(len(trials))
    src = dict(line.strip().split(None, 1) for line in open(data / "feats.scp"))
    with open(data / "trials", "w") as f, open(data / "trial_feats.scp", "w") as h:
        for i, k in enumerate(order):
            f.write(f"utt{trials[k][0]:03d} {trials[k][1]}\n")
            h.write(f"trial{i:03d} {src[f'utt{trials[k][0]:03d}']}\n")  # the token part's input: one entry per trial
    return data, [int(lens[trials[k][0]]) for k in order]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, 1e-3 * e0.elapsed_time(e1)


def sweep(run, compare, sizes, windows, label):
    """run(size, name) -> output; compare(output, size 1's output) -> a figure.  Returns {size: record}."""
    base, diff = None, {}
    for s in sizes:  # warm-up run of every size (every shape the timed windows use), checked against size 1's
        got = run(s, f"warm{s}")
        base = got if base is None else base
        diff[s] = compare(got, base)
    times = {s: [] for s in sizes}
    for _ in range(windows):
        for s in sizes:  # alternate: every size sees the same machine state
            times[s].append(timed(lambda: run(s, "timed"))[1])
    rec = {}
    for s in sizes:
        ups = sorted(TRIALS / t for t in times[s])
        rec[str(s)] = {"utt_per_s_median": statistics.median(ups), "utt_per_s_min": ups[0], "utt_per_s_max": ups[-1],
                       "run_s": times[s], "vs_size_1": diff[s]}
        print(f"{label} size {s}: median {statistics.median(ups):.1f} utt/s (min {ups[0]:.1f}, max {ups[-1]:.1f}); "
              f"vs size 1: {diff[s]:.3e}", flush=True)
    return rec


def decode_part(work, dtype, sizes, windows):
    cfg = config("vcc20", dtype)
    data, lens = make_dir(work, cfg["encoder"]["in_channels"][0], cfg["y_num"])
    torch.manual_seed(SEED)
    dec = Decoder(cfg)
    batched = hasattr(dec, "decode_batch_size")

    def run(size, name):
        if batched:
            dec.decode_batch_size = size
        out = Path(work) / name
        shutil.rmtree(out, ignore_errors=True)
        out.mkdir()
        dec.decode(data, out)
        return [np.array(K.load_mat(line.strip().split(None, 1)[1])) for line in open(out / "feats.scp")]

    def compare(got, base):  # largest relative L2 over the trials
        assert [g.shape[0] for g in got] == lens
        return max(float(np.linalg.norm(g - b) / np.linalg.norm(b)) for g, b in zip(got, base))

    rec = sweep(run, compare, sizes if batched else [1], windows, f"{dtype} decode")
    return {"batched_driver": batched, "frames": sum(lens), "min": min(lens), "max": max(lens), "sizes": rec,
            "vs_size_1": "largest relative L2 of the written (compressed) features over the trials"}


def token_part(work, dtype, sizes, windows):
    cfg = config("aishell3", dtype)
    data, lens = make_dir(work, cfg["encoder"]["in_channels"][0], cfg["y_num"])
    conf, ckpt = Path(work) / "conf.yaml", Path(work) / "ckpt.pt"
    conf.write_text(yaml.safe_dump(cfg))
    torch.manual_seed(SEED)
    from vae_npvc_amd.model.vqvae import Model
    m = Model(cfg)
    sd = m.state_dict()
    sd["quantizer.emb_init"] = torch.tensor(True)  # a trained codebook: N(0, 1) * 0.3
    sd["quantizer.embeddings"] = torch.randn(sd["quantizer.embeddings"].shape) * 0.3
    torch.save({"model": sd, "iteration": 0}, ckpt)
    batched = "--batch_size" in inspect.getsource(extract_bnf)

    def run(size, name):
        out = Path(work) / f"{name}.txt"
        argv = ["-c", str(conf), "--model_path", str(ckpt), "--bnf_kind", "id"]
        extract_bnf.main(argv + (["--batch_size", str(size)] if batched else [])
                         + [f"scp:{data}/trial_feats.scp", str(out)])
        return [line.split() for line in open(out)]

    def compare(got, base):  # share of equal ids, in input order
        assert [u for u, _ in got] == [u for u, _ in base] and len(got) == len(lens)
        a = np.concatenate([np.array(t.strip("<>").split("><"), dtype=np.int64) for _, t in got])
        b = np.concatenate([np.array(t.strip("<>").split("><"), dtype=np.int64) for _, t in base])
        assert a.shape == b.shape == (sum(lens),)
        return float((a == b).mean())

    rec = sweep(run, compare, sizes if batched else [1], windows, f"{dtype} token")
    return {"batched_driver": batched, "frames": sum(lens), "sizes": rec,
            "vs_size_1": "share of ids equal to size 1's (the model is built and loaded inside every run)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--sizes", default="1,4,8,16,32")
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--part", default="both", choices=["decode", "token", "both"])
    ap.add_argument("--len-pad", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "flat_convert_bench needs the MI355X"
    if a.len_pad is not None:
        from vae_npvc_amd.engine.step import VQVAEEngine
        VQVAEEngine.LEN_PAD = a.len_pad
    sizes = [int(s) for s in a.sizes.split(",")]
    res = {"dtype": a.dtype, "trials": TRIALS, "windows": a.windows, "len_pad": a.len_pad,
           "lengths": f"uniform integers {LEN_LO}..{LEN_HI}, seed {SEED}"}
    for part, fn in (("decode", decode_part), ("token", token_part)):
        if a.part in (part, "both"):
            work = tempfile.mkdtemp(prefix="flat_convert_bench_")
            try:
                res[part] = fn(work, a.dtype, sizes, a.windows)
            finally:
                shutil.rmtree(work, ignore_errors=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
