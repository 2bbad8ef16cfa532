"""What feeds the training step, measured at the bench's shape (vcc20 recipe,
64 x 256 frames x 80 mel, bf16 engine) on a synthetic corpus generated here:

  a  batches/s of DataLoader over dataset/utt2mel_spk.py with num_jobs 0 and 8
     (bin/train.py's arguments: shuffle, drop_last, pin_memory): the path of
     the default dataset_type;
  b  the same DataLoaders over dataset/resident.py's Dataset (items sliced
     from host memory);
  c  batches/s of resident.loader (batches cut on the device), and the device
     time of vqx_crop_batch alone with its bytes per second (the cropped rows
     read once, x written once) against the 8 TB/s HBM figure;
  d  wall-clock ms per iteration of Trainer.train_step fed by a (num_jobs 8)
     and by c, beside the same trainer stepping on one fixed device batch.
     Every path reads the loss dict at every step, as bin/train.py does.

Corpus (default): 4096 utterances of 200 to 700 frames drawn uniformly, 80
mel, Kaldi speech-feature compressed arks -- about 1.8 M frames, 5 h at 10 ms,
0.6 GB resident in fp32; 64 batches an epoch.  The vcc20 recipe's own size is
not recorded in this repository, so this is a stand-in of its order; --utts
changes it.

a and b are host clocks over windows of consecutive batches of one running
iterator (a new epoch re-creates the workers, as in bin/train.py); c and d are
host clocks over windows that end in one device synchronisation, the paths
of d alternating; the kernel time is device events around windows of
launches.  Median with min and max over the windows.  A lab script, no
pass/fail bar.
Usage (GPU box): python tools/input_bench.py [--out DIR] [--utts N] [--skip-workers] [--kernel-only]"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time
import types
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from vae_npvc_amd import ops  # noqa: E402
from vae_npvc_amd.dataset import kaldi_io as K  # noqa: E402
from vae_npvc_amd.dataset import resident, utt2mel_spk  # noqa: E402
from vae_npvc_amd.trainer.basic import Trainer  # noqa: E402

B, T, MEL = 64, 256, 80
WINDOWS = 7
HBM_BYTES_PER_S = 8e12
CONF = Path(__file__).resolve().parent.parent / "vae_npvc_amd" / "conf" / "vcc20.yaml"


def write_corpus(root, n_utts, y_num, seed=0):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(200, 701, n_utts)
    with K.WriteHelper(f"ark,scp:{root}/feats.ark,{root}/feats.scp", compression_method=K.K_SPEECH_FEATURE) as w:
        for i, n in enumerate(lengths):
            w[f"utt{i:06d}"] = rng.standard_normal((int(n), MEL)).astype(np.float32)
    with open(root / "utt2num_frames", "w") as f:
        f.writelines(f"utt{i:06d} {int(n)}\n" for i, n in enumerate(lengths))
    with open(root / "utt2spk_id", "w") as f:
        f.writelines(f"utt{i:06d} {i % y_num}\n" for i in range(n_utts))
    return int(lengths.sum())


def endless(loader):
    while True:
        yield from loader


def summary(v, unit):
    return {f"median_{unit}": statistics.median(v), f"min_{unit}": min(v), f"max_{unit}": max(v), "windows": len(v)}


def host_rate(batches, warmup, reps, windows=WINDOWS, device=False):
    """batches/s over `windows` windows of `reps` consecutive batches."""
    for _ in range(warmup):
        next(batches)
    rates = []
    for _ in range(windows):
        if device:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            next(batches)
        if device:
            torch.cuda.synchronize()
        rates.append(reps / (time.perf_counter() - t0))
    return dict(summary(rates, "batches_per_s"), reps=reps)


def kernel_time(ds, reps=200, windows=WINDOWS):
    """Device time of vqx_crop_batch alone on one batch's plan (every crop a full T rows)."""
    corpus, table = ds.on_device("cuda:0")
    rng = random.Random(1)
    idx = rng.sample([i for i in range(len(ds.lengths)) if ds.lengths[i] >= T], B)
    row0 = torch.tensor([int(ds.offsets[i]) + rng.randint(0, ds.lengths[i] - T) for i in idx])
    length = torch.full((B,), T, dtype=torch.int32)
    utt = torch.tensor(idx, dtype=torch.int32)
    x = torch.empty(B, MEL, T, device="cuda")
    y = torch.empty(B, 1, dtype=torch.int64, device="cuda")
    for _ in range(20):
        ops.crop_batch(corpus, table, row0, length, utt, x, y)
    us = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.crop_batch(corpus, table, row0, length, utt, x, y)
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / reps)
    nbytes = 2 * B * MEL * T * 4 + 2 * B * 8
    r = dict(summary(us, "us"), reps=reps, algorithmic_bytes=nbytes)
    r["bytes_per_s"] = nbytes / (r["median_us"] * 1e-6)
    r["fraction_of_hbm"] = r["bytes_per_s"] / HBM_BYTES_PER_S
    r["note"] = "back-to-back launches in one stream: launch-to-launch time, an upper bound of the kernel's own"
    return r


def fed_steps(tr, feeds, reps, windows=WINDOWS, warmup=12):
    """ms per iteration of train_step + reading the loss dict, the feeds alternating."""
    def step(batch):
        _, detail = tr.train_step(batch)
        for _k, _v in detail.items():  # bin/train.py reads every value at every step
            pass

    for nxt in feeds.values():
        for _ in range(warmup):
            step(nxt())
    ms = {k: [] for k in feeds}
    each = {k: [] for k in feeds}  # single iterations (host clock; the loss read paces the loop): where a mean comes from
    for _ in range(windows):
        for name, nxt in feeds.items():
            if name.startswith("a"):  # worker prefetch filled up while the other paths ran: drain it
                for _ in range(16):
                    nxt()
            torch.cuda.synchronize()
            t0 = t = time.perf_counter()
            for _ in range(reps):
                step(nxt())
                t, tp = time.perf_counter(), t
                each[name].append(1e3 * (t - tp))
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / reps)
    out = {}
    for k, v in ms.items():
        e = sorted(each[k])
        out[k] = dict(summary(v, "ms"), reps=reps, iter_median_ms=statistics.median(e), iter_p99_ms=e[int(0.99 * len(e))],
                      iter_max_ms=e[-1], iters_over_twice_median=sum(x > 2 * statistics.median(e) for x in e),
                      iters=len(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/input")
    ap.add_argument("--utts", type=int, default=4096)
    ap.add_argument("--skip-workers", action="store_true", help="leave out the num_jobs 8 DataLoaders")
    ap.add_argument("--step-reps", type=int, default=64)
    ap.add_argument("--kernel-only", action="store_true",
                    help="vqx_crop_batch launches on a random corpus and nothing else: the program of a "
                         "`rocprofv3 --kernel-trace --stats` run, for the kernel's own time")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "input_bench needs the MI355X"
    if a.kernel_only:
        ds = types.SimpleNamespace(lengths=[700] * 2048, offsets=torch.arange(2049) * 700,
                                   on_device=lambda d: (torch.randn(2048 * 700, MEL, device=d),
                                                        torch.arange(2048, device=d)))
        print(kernel_time(ds, reps=100, windows=3), flush=True)
        return
    cfg = yaml.safe_load(open(CONF))
    cfg.update(compute_dtype="bf16", batch_size=B, crop_length=T)
    res = {"shape": dict(B=B, T=T, mel=MEL), "dtype": "bf16", "utts": a.utts, "cpus": len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        t0 = time.perf_counter()
        res["frames"] = write_corpus(root, a.utts, cfg["y_num"])
        res["write_s"] = time.perf_counter() - t0
        par = utt2mel_spk.Dataset(root, cfg)
        t0 = time.perf_counter()
        ds = resident.Dataset(root, cfg)
        res["resident_load_s"], res["resident_bytes"] = time.perf_counter() - t0, ds.frames.numel() * 4
        print(ds.load_info, flush=True)
        torch.manual_seed(0)
        random.seed(0)

        def dl(dataset, jobs):
            return DataLoader(dataset, num_workers=jobs, shuffle=True, batch_size=B, pin_memory=True, drop_last=True)

        jobs = [0] if a.skip_workers else [0, 8]
        res["input"] = {}
        for name, dataset in (("a_utt2mel_spk", par), ("b_resident_dataset", ds)):
            for j in jobs:
                it = endless(dl(dataset, j))
                res["input"][f"{name}_jobs{j}"] = host_rate(it, warmup=8, reps=32 if j == 0 else 128)
                del it
                print(name, j, res["input"][f"{name}_jobs{j}"], flush=True)
        res["input"]["c_resident_loader"] = host_rate(endless(resident.loader(ds, B, shuffle=True, drop_last=True)),
                                                      warmup=64, reps=512, device=True)
        print("c", res["input"]["c_resident_loader"], flush=True)
        res["crop_batch_kernel"] = kernel_time(ds)
        print("kernel", res["crop_batch_kernel"], flush=True)

        tr = Trainer(cfg)
        x0 = torch.randn(B, MEL, T, device="cuda")
        y0 = torch.randint(0, cfg["y_num"], (B, 1), device="cuda")
        feeds = {"fixed_batch": lambda: (x0, y0)}
        c_it = endless(resident.loader(ds, B, shuffle=True, drop_last=True))
        feeds["c_resident_loader"] = lambda: next(c_it)
        if not a.skip_workers:
            a_it = endless(dl(par, 8))
            feeds["a_utt2mel_spk_jobs8"] = lambda: next(a_it)
        res["train_step"] = fed_steps(tr, feeds, a.step_reps)
        for k, v in res["train_step"].items():
            print(f"train_step fed by {k}: median {v['median_ms']:.3f} ms (min {v['min_ms']:.3f}, "
                  f"max {v['max_ms']:.3f})", flush=True)
        fx = res["train_step"]["fixed_batch"]
        res["train_step"]["fixed_batch_spread_ms"] = fx["max_ms"] - fx["min_ms"]
        del feeds, c_it
        if not a.skip_workers:
            del a_it
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "input_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
