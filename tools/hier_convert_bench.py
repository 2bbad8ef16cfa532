"""Utterances per second of `decoder.hier.Decoder.decode` with the hierarchical
model at the vae2 recipe's size (80 mels, 3 levels, use_gst, 512-channel
convs) over a synthetic decode directory, at `decode_batch_size` 1 (the loop
over single utterances) and a few larger values.

The directory: TRIALS trials over TRIALS // 3 source utterances (every source
is converted to three target speakers), lengths drawn uniformly from
LEN_LO..LEN_HI frames with a fixed seed, listed in shuffled order.  The
weights are the seeded initial ones: the time of a conversion does not depend
on their values.

One timed window is one whole `decode` of the directory: reading the
features, the conversions, the read-back and the Kaldi writer (compressed
matrices, the default).  Device events around the call (it ends with a
read-back, so the host clock would serve as well); the batch sizes alternate
inside every round, WINDOWS rounds after one warm-up decode each; median and
range of utterances per second.  Every size's output is compared with size
1's (largest relative L2 over the trials) before it is timed.

On a tree whose driver has no `decode_batch_size` only size 1 is measured (the
baseline: `decode_batch_size: 1` must reproduce it).  A lab script, no
pass/fail bar.

--model vqvae2a | vqvae2b measures those two models at the same dimensions
(model_arch).  Their one-at-a-time conversion is the eval-mode forward, which
takes only lengths that are multiples of the encoders' total down-sampling
(64), so for them the lengths are drawn uniformly from the multiples of 64
inside LEN_LO..LEN_HI (192..640); every size converts the same directory.  On
a tree whose `convert` takes no `lengths` for these models give --sizes 1.
Usage (GPU box): python tools/hier_convert_bench.py [--json OUT] [--dtype bf16] [--sizes 1,4,8,16,32]
                                                    [--model vqvae2|vqvae2a|vqvae2b]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_npvc_amd.dataset import kaldi_io as K  # noqa: E402
from vae_npvc_amd.decoder.hier import Decoder  # noqa: E402

MEL, SPEAKERS = 80, 117
TRIALS, LEN_LO, LEN_HI, SEED = 96, 150, 650, 20
WINDOWS = 5


def recipe(dtype):
    """The vae2 recipe's model keys (egs/vcc20/vae2/conf/train_pytorch_vqvae2.yaml), as tools/hier_train_bench.py."""
    enc = dict(kernel_size=3, z_channels=128, dilation=False, stack_kernel_size=3, stack_layers=1,
               use_weight_norm=True, use_causal_conv=False)
    dec = dict(out_channels=[512], skip_channels=128, kernel_size=3, upsample_scales=[1], dilation=False,
               stack_kernel_size=3, use_weight_norm=True, use_causal_conv=False)
    vq = dict(z_dim=128, z_num=512, normalize=True)
    return {
        "model_type": "vae_npvc_amd.model.vqvae2", "decoder_type": "vae_npvc_amd.decoder.hier",
        "levels": 3, "y_dim": 128, "y_num": SPEAKERS, "beta": 0.01, "use_gst": True, "use_ema": False, "jitter_p": 0.0,
        "compute_dtype": dtype,
        "encoder.0": dict(enc, in_channels=[MEL], out_channels=[512], downsample_scales=[1], stacks=[6]),
        "encoder.1": dict(enc, in_channels=[512, 512], out_channels=[512, 512], downsample_scales=[2, 2], stacks=[3, 3]),
        "encoder.2": dict(enc, in_channels=[512, 512], out_channels=[512, 512], downsample_scales=[4, 4], stacks=[3, 3]),
        "quantizer.0": dict(vq), "quantizer.1": dict(vq),
        "quantizer.2": dict(ref_embed_dim=128, gst_tokens=10, gst_token_dim=128, gst_heads=4),
        "decoder.0": dict(dec, in_channels=[384], cond_channels=128, final_channels=MEL, stacks=[10]),
        "decoder.1": dict(dec, in_channels=[128], cond_channels=256, final_channels=128, stacks=[6]),
        "decoder.2": dict(dec, in_channels=[128], cond_channels=128, final_channels=128, stacks=[6]),
    }


GRANULE = 64  # the total down-sampling of the three encoders


def model_arch(model, dtype):
    """The config of --model: vqvae2 is the recipe; vqvae2a the same dimensions with EMA codebooks and the
    decoders wired for its chain (decoder i reads level i and decoder i + 1's output, every one conditioned on
    the speaker); vqvae2b the same with level decoders of final_channels 128 that read their own level alone and
    an unconditioned final_decoder of the recipe's decoder.0 shape."""
    cfg = recipe(dtype)
    if model == "vqvae2":
        return cfg
    cfg.update(model_type=f"vae_npvc_amd.model.{model}", use_ema=True)
    for i in (0, 1):
        cfg[f"quantizer.{i}"] = dict(z_dim=128, z_num=512, mu=0.99)
    if model == "vqvae2a":
        for i, cin in enumerate((256, 256, 128)):
            cfg[f"decoder.{i}"] = dict(cfg[f"decoder.{i}"], in_channels=[cin], cond_channels=128)
    else:
        cfg["final_decoder"] = dict(cfg["decoder.0"], cond_channels=0)
        for i in range(3):
            cfg[f"decoder.{i}"] = dict(cfg[f"decoder.{i}"], in_channels=[128], cond_channels=128, final_channels=128)
    return cfg


def make_dir(root, granule=1):
    """The synthetic decode directory; returns (path, the trials' lengths in trial order).  granule > 1: the
    lengths are multiples of it."""
    rng = np.random.default_rng(SEED)
    data = Path(root) / "eval"
    data.mkdir()
    n_src = TRIALS // 3
    if granule == 1:
        lens = rng.integers(LEN_LO, LEN_HI + 1, n_src)
    else:
        lens = granule * rng.integers(-(-LEN_LO // granule), LEN_HI // granule + 1, n_src)
    with K.WriteHelper(f"ark,scp:{data}/feats.ark,{data}/feats.scp") as w:
        for u in range(n_src):
            w[f"utt{u:03d}"] = rng.standard_normal((int(lens[u]), MEL)).astype(np.float32)
    trials = [(u, int(rng.integers(0, SPEAKERS))) for u in range(n_src) for _ in range(3)]
    order = rng.permutation(len(trials))
    with open(data / "trials", "w") as f:
        for k in order:
            f.write(f"utt{trials[k][0]:03d} {trials[k][1]}\n")
    return data, [int(lens[trials[k][0]]) for k in order]


def read_all(path):
    return [np.array(K.load_mat(line.strip().split(None, 1)[1])) for line in open(Path(path) / "feats.scp")
            if line.strip()]


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--sizes", default="1,4,8,16,32")
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--model", default="vqvae2", choices=["vqvae2", "vqvae2a", "vqvae2b"])
    return ap


def main():
    a = parser().parse_args()
    assert torch.cuda.is_available(), "hier_convert_bench needs the MI355X"
    work = tempfile.mkdtemp(prefix="hier_convert_bench_")
    try:
        data, lens = make_dir(work, 1 if a.model == "vqvae2" else GRANULE)
        torch.manual_seed(SEED)
        dec = Decoder(model_arch(a.model, a.dtype))
        if a.model != "vqvae2":  # an EMA codebook is all zeros before its first training forward
            for q in dec.model.quantizers[:2]:
                q.embeddings.normal_()
        batched = hasattr(dec, "decode_batch_size")
        sizes = [int(s) for s in a.sizes.split(",")] if batched else [1]

        def decode(size, name):
            if batched:
                dec.decode_batch_size = size
            out = Path(work) / name
            shutil.rmtree(out, ignore_errors=True)
            out.mkdir()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dec.decode(data, out)
            e1.record()
            e1.synchronize()
            return out, 1e-3 * e0.elapsed_time(e1)

        # warm-up decode of every size (every shape the timed windows use), checked against size 1's output
        base, diff = None, {}
        for s in sizes:
            got = read_all(decode(s, f"warm{s}")[0])
            assert [g.shape[0] for g in got] == lens
            if base is None:
                base = got
            diff[s] = max(float(np.linalg.norm(g - b) / np.linalg.norm(b)) for g, b in zip(got, base))
        times = {s: [] for s in sizes}
        for _ in range(a.windows):
            for s in sizes:  # alternate: every size sees the same machine state
                times[s].append(decode(s, "timed")[1])
        dist = f"uniform integers {LEN_LO}..{LEN_HI}, seed {SEED}" if a.model == "vqvae2" else \
            f"uniform multiples of {GRANULE} in {LEN_LO}..{LEN_HI}, seed {SEED}"
        res = {"dtype": a.dtype, "batched_driver": batched, "trials": TRIALS, "frames": sum(lens),
               "lengths": {"distribution": dist, "min": min(lens),
                           "max": max(lens), "mean": sum(lens) / len(lens)},
               "windows": a.windows, "sizes": {}}
        if a.model != "vqvae2":  # the default's records keep their keys
            res["model"] = a.model
        for s in sizes:
            ups = sorted(TRIALS / t for t in times[s])
            res["sizes"][str(s)] = {"utt_per_s_median": statistics.median(ups), "utt_per_s_min": ups[0],
                                    "utt_per_s_max": ups[-1], "decode_s": times[s],
                                    "max_rel_l2_vs_size_1": diff[s]}
            tag = "" if a.model == "vqvae2" else a.model + " "
            print(f"{tag}{a.dtype} decode_batch_size {s}: median {statistics.median(ups):.1f} utt/s "
                  f"(min {ups[0]:.1f}, max {ups[-1]:.1f}); written features vs size 1: rel L2 <= {diff[s]:.2e}",
                  flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
