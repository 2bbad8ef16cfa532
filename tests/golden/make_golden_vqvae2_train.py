"""Fixtures of training steps of the hierarchical model:
tests/golden/vqtrain_<case> (.npz + .json), case gst | plain_top.

Run where the reference checkout is available (not on the GPU box, not from
any test):

    python tests/golden/make_golden_vqvae2_train.py --reference DIR [--only NAME]

Starts from the parameters, x and y stored in vqmodel_<case>
(make_golden_vqvae2_model.py) and restates the reference's Trainer.train_step
(trainer/basic.py:55-79, which itself needs .cuda()) on the CPU around the
reference's `vqvae2.Model`: zero_grad, forward, backward,
clip_grad_norm_(0.5), torch.optim.Adam(lr 1e-3, betas (0.5, 0.999)),
StepLR(step_size 1, gamma 0.5).  Once in float32 and once in float64; the
float64 run is the expected result, the float32 run's distance from it per
quantity (`err32`) is the reference's own rounding.

Per forward: the loss dict, the gradient norm before the clip, the indices of
every quantized level, the smallest top-2 distance gap per level.  Asserted
here, so a fixture that exists satisfies it: every recorded forward has all
gaps >= 2e-4 (twice the project's near-tie threshold) in both runs, the two
runs' indices are identical, and every norm is above 0.5 (the clip is active
in every step).  FORWARDS is what holds: gst 3 (the 4th forward's smallest gap
is 8.9e-5), plain_top 2 (the 3rd's is 2.2e-5).
"""
import argparse
import json
import os
from pathlib import Path

import numpy as np
import torch

from make_golden_vqvae2_model import load_reference, rel, top2_gap

HERE = Path(__file__).resolve().parent
FORWARDS = {"gst": 3, "plain_top": 2}
MIN_GAP = 2e-4
TRAIN = dict(learning_rate=1e-3, max_grad_norm=0.5, optim_type="Adam", lr_scheduler="StepLR",
             lr_param=dict(step_size=1, gamma=0.5))
BETAS = (0.5, 0.999)


def load_model_fixture(case):
    meta = json.load(open(HERE / f"vqmodel_{case}.json"))
    arr = {}
    for name in meta["files"]:
        arr.update(np.load(HERE / name, allow_pickle=False))
    return meta, arr


def run(ref, meta, arr, dtype, forwards):
    m = ref.Model(meta["arch"])
    sd = {k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}
    torch.nn.Module.load_state_dict(m, sd)  # the class's own override reads an attribute it never sets
    m.to(dtype)
    m.train()
    x = torch.from_numpy(arr["x"].copy()).to(dtype)
    y = torch.from_numpy(arr["y"].copy())
    opt = torch.optim.Adam(m.parameters(), lr=TRAIN["learning_rate"], betas=BETAS, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.StepLR(optimizer=opt, **TRAIN["lr_param"])
    out = []
    for _ in range(forwards):
        gaps, ids, hooks = [], [], []
        for q in m.quantizers:
            if hasattr(q, "embeddings"):
                hooks.append(q.register_forward_hook(
                    lambda mod, inp, o: gaps.append(top2_gap(inp[0], mod.embeddings, mod.normalize))))
                hooks.append(q.register_forward_hook(lambda mod, inp, o: ids.append(mod.encode(inp[0].detach()))))
        m.zero_grad()
        _, loss, detail = m((x, y))
        for h in hooks:
            h.remove()
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(m.parameters(), TRAIN["max_grad_norm"])
        opt.step()
        sched.step()
        out.append(dict(detail={k: float(v) for k, v in detail.items()}, norm=float(norm), gaps=gaps, ids=ids))
    return out


def make(ref, case):
    meta, arr = load_model_fixture(case)
    n = FORWARDS[case]
    r32 = run(ref, meta, arr, torch.float32, n)
    r64 = run(ref, meta, arr, torch.float64, n)
    arrays, err32, gaps32, gaps64 = {}, {}, [], []
    for s, (a, b) in enumerate(zip(r32, r64)):
        assert min(a["gaps"] + b["gaps"]) >= MIN_GAP, (case, s, a["gaps"], b["gaps"])
        assert len(a["ids"]) == len(b["ids"]) and all(torch.equal(i, j) for i, j in zip(a["ids"], b["ids"])), (case, s)
        assert min(a["norm"], b["norm"]) > TRAIN["max_grad_norm"], (case, s, a["norm"], b["norm"])
        for k, v in b["detail"].items():
            arrays[f"loss.{s}.{k}"] = np.float64(v)
            err32[f"{s}.{k}"] = rel(a["detail"][k], v)
        arrays[f"norm.{s}"] = np.float64(b["norm"])
        err32[f"{s}.norm"] = rel(a["norm"], b["norm"])
        for k, idx in enumerate(b["ids"]):
            arrays[f"idx.{s}.{k}"] = idx.numpy()
        gaps32.append(a["gaps"])
        gaps64.append(b["gaps"])
    np.savez_compressed(HERE / f"vqtrain_{case}.npz", **arrays)
    out = {"case": case, "model_fixture": f"vqmodel_{case}", "forwards": n, "train": TRAIN, "betas": list(BETAS),
           "loss_keys": list(r64[0]["detail"].keys()), "levels": len(r64[0]["ids"]), "min_gap": MIN_GAP,
           "gaps32": gaps32, "gaps64": gaps64, "norms64": [b["norm"] for b in r64], "err32": err32,
           "files": [f"vqtrain_{case}.npz"]}
    with open(HERE / f"vqtrain_{case}.json", "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"vqtrain_{case}: {n} forwards, norms {[round(b['norm'], 4) for b in r64]}, "
          f"smallest gap {min(min(g) for g in gaps32 + gaps64):.3g}, err32 {min(err32.values()):.2e}.."
          f"{max(err32.values()):.2e}, {(HERE / f'vqtrain_{case}.npz').stat().st_size} bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQX_REFERENCE"),
                    help="checkout of the reference repository (default: env VQX_REFERENCE)")
    ap.add_argument("--only", default=None, choices=sorted(FORWARDS))
    a = ap.parse_args()
    if not a.reference:
        ap.error("give --reference DIR or set VQX_REFERENCE")
    torch.set_num_threads(1)
    ref, _ = load_reference(a.reference)
    for name in FORWARDS:
        if a.only in (None, name):
            make(ref, name)
