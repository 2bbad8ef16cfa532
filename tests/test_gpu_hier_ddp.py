"""Data parallel for the hierarchical models (vqvae2, vqvae2a, vqvae2b) on the
GPU, against the reference's float64 fixtures: N ranks on equal shards of the
global batch must take the step one process takes on the whole batch
(SURVEY §8e), so the targets are the single-process fixtures themselves and
the measure and bound are the single-process tests' own
(tests/test_gpu_hier_encoder.py `ratios` / `report`: error <= max(8 err32,
16 ulp) per quantity).  Splitting a sum over two ranks reorders it; it does
not change its error class.

Two ranks (gloo process group, both on cuda:0: the box has one GPU and RCCL
refuses two ranks on one device), rank r on utterance r of the fixture's B = 2
batch, every rank reseeded with the fixture's seed.  One pair of children per
family runs all its cases in sequence inside one process group; a fourth
child runs the RCCL branch in a world-size-1 nccl group.  Children are killed
in a `finally`, so a failure leaves nothing on the GPU.

  * vqvae2a (ema_gst, single_ema, plain_shared) and vqvae2b (pooled_ema, whose
    pooled one-frame EMA top level takes the N_global < K gather path): model
    + engine driven directly -- forward, backward, reduce_grads(), no optimizer
    step, as the fixtures take none.  Per step: the averaged gradients, the
    float buffers (global EMA state) and emb_init on each rank, the ranks'
    lookups bit-exact against their rows, xhat, the rank mean of the
    frame-mean losses, the EMA diagnostics on each rank; parameters and
    buffers bit-identical between the ranks.
  * vqvae2 through Trainer (gst, plain_top): train_step over the fixture's
    steps; rank-mean losses, the pre-clip norm of the averaged gradient, the
    ranks' indices; flat_p and the moments equal on both ranks; both
    `grad_sync` values give the same bits.
  * RCCL, world size 1: the trainer with a Comm equals the one without bit for
    bit (an AVG over one rank is the identity), 4 * n_params bytes per step;
    the EMA path of vqvae2a runs there against the fixture.
  * valid_step under a comm issues no collective and writes nothing.
"""
import hashlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.hier_model_ref import ULP16, fixture
from tests.test_gpu_hier_encoder import ratios, report

pytestmark = pytest.mark.gpu

MEAN_KEYS = ("Total", "VQ loss", "X like", "quanti_err")      # frame means over equal shards: global = rank mean
EMA_KEYS = ("entropy", "used_curr", "usage", "diff_emb")      # from the all-reduced statistics: global on every rank
A_CASES = ("ema_gst", "single_ema", "plain_shared")
TRAIN_CASES = ("gst", "plain_top")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sha(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ children
def _model_steps(kind, case, rank, world):
    """The fixture's steps on this rank's shard with the engine's data-parallel
    path; everything the parent compares, as numpy arrays."""
    import importlib
    from vae_npvc_amd.parallel.ddp import Comm
    T = importlib.import_module({"vq2a": "tests.test_gpu_vqvae2a", "vq2b": "tests.test_gpu_vqvae2b"}[kind])
    meta, arr = fixture(kind, case)
    m = T.build_model(meta, arr)
    eng = m.engine()
    comm = Comm()
    eng.attach_comm(comm)
    assert (eng.world, eng.rank) == (world, rank) and eng.flat_g.numel() == eng.n_params
    x, y = T.batch(arr)
    per = x.shape[0] // world
    x, y = x[rank * per:(rank + 1) * per].contiguous(), y[rank * per:(rank + 1) * per].contiguous()
    ids = []
    hooks = T.record_indices(m, ids)
    T.reseed(meta["run_seed"])
    steps = []
    for n in range(1, meta["steps"] + 1):
        for p in eng.params:
            p.grad = None
        del ids[:]
        calls = comm.calls
        xhat, loss, detail = m((x, y))
        loss.backward()
        eng.reduce_grads()
        torch.cuda.synchronize()
        steps.append(dict(
            detail=dict(detail), keys=list(detail), total_is_loss=float(loss.detach()) == detail["Total"],
            idx=[i.numpy() for i in ids], xhat=xhat.detach().cpu().numpy(), calls=comm.calls - calls,
            grads={k: p.grad.cpu().numpy() for k, p in m.named_parameters() if p.grad is not None},
            grads_are_views=all(p.grad is None or p.grad.data_ptr() == eng.flat_g.data_ptr() + 4 * o
                                for p, o in zip(eng.params, eng._p_off)),
            bufs={k: b.detach().cpu().numpy() for k, b in m.named_buffers()}))
    for h in hooks:
        h.remove()
    out = dict(steps=steps, state=_sha(*m.state_dict().values()))
    # valid_step under a comm: no collective, nothing written, the generator untouched
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    calls, nbytes, rng = comm.calls, comm.bytes, torch.get_rng_state()
    vdetail = eng.valid_step(x, y)
    out["valid"] = dict(calls=comm.calls - calls, bytes=comm.bytes - nbytes, training=m.training,
                        rng=bool(torch.equal(torch.get_rng_state(), rng)),
                        same=all(torch.equal(v, before[k]) for k, v in m.state_dict().items()),
                        finite=all(np.isfinite(v) for v in vdetail.values()))
    return out


def _trainer_steps(case, rank, world, comm=None, **over):
    """train_step over the vqtrain fixture's steps on this rank's shard.  The
    Trainer attaches its own Comm when the world is larger than 1; `comm`
    attaches one by hand (the world-size-1 RCCL group)."""
    from tests import test_gpu_hier_trainer as T
    tmeta, _ = T.train_fixture(case)
    meta, _ = fixture("vqmodel", case)
    tr = T.make_trainer(case, **over)
    eng = tr.engine
    if comm is not None:
        eng.attach_comm(comm)
    assert (eng.world, eng.rank) == (world, rank) and (eng.comm is not None) == (world > 1 or comm is not None)
    x, y = T.batch(case)
    per = x.shape[0] // world
    x, y = x[rank * per:(rank + 1) * per].contiguous(), y[rank * per:(rank + 1) * per].contiguous()
    torch.manual_seed(meta["seed"])
    np.random.seed(meta["seed"])
    ids = {}
    hooks = T.record_indices(tr.model, ids)
    details, norms, nbytes = [], [], []
    for s in range(tmeta["forwards"]):
        b0 = eng.comm.bytes if eng.comm is not None else 0
        it, detail = tr.train_step((x, y))
        assert it == s + 1
        details.append(dict(detail))
        norms.append(float(eng.sumsq.sqrt()))
        nbytes.append((eng.comm.bytes if eng.comm is not None else 0) - b0)
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    return dict(details=details, keys=list(details[0]), norms=norms, bytes=nbytes, n_params=eng.n_params,
                idx={i: [t.numpy() for t in v] for i, v in ids.items()}, levels=T.quantized_levels(tr.model),
                p=_sha(eng.flat_p), m=_sha(eng.exp_avg), v=_sha(eng.exp_avg_sq), opt_step=int(eng.opt_step),
                grad_sync=tr.grad_sync, overlap=None if eng.comm is None else eng.comm.overlap)


def _family(name, rank, world):
    if name == "vq2a":
        return {c: _model_steps("vq2a", c, rank, world) for c in A_CASES}
    if name == "vq2b":
        return {"pooled_ema": _model_steps("vq2b", "pooled_ema", rank, world)}
    if name == "vqvae2":
        out = {c: _trainer_steps(c, rank, world) for c in TRAIN_CASES}
        out["gst_end"] = _trainer_steps("gst", rank, world, grad_sync="end")
        return out
    if name == "rccl":
        from vae_npvc_amd.parallel.ddp import Comm
        comm = Comm()
        return dict(backend=comm.backend, plain=_trainer_steps("gst", rank, world),
                    ddp=_trainer_steps("gst", rank, world, comm=comm),
                    ema=_model_steps("vq2a", "ema_gst", rank, world))
    raise ValueError(name)


def _child(rank, world, port, backend, name, q):
    try:
        import torch.distributed as dist
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        kw = {"device_id": dev} if backend == "nccl" else {}
        dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world, **kw)
        out = _family(name, rank, world)
        torch.cuda.synchronize()
        q.put((rank, out, None))
        dist.destroy_process_group()
    except Exception as e:  # surface the failure to the parent
        import traceback
        q.put((rank, None, traceback.format_exc() + repr(e)))


def _spawn(name, world=2, backend="gloo"):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    keep = os.environ.get("MASTER_ADDR")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    ps = [ctx.Process(target=_child, args=(r, world, port, backend, name, q)) for r in range(world)]
    try:
        for p in ps:
            p.start()
        res = []
        for _ in ps:
            res.append(q.get(timeout=300))
            assert res[-1][2] is None, res[-1][2]  # a rank failed: do not wait for the other
        for p in ps:
            p.join(60)
    finally:
        for p in ps:
            if p.is_alive():
                p.kill()
            p.join(10)
        if keep is None:
            os.environ.pop("MASTER_ADDR", None)
        else:
            os.environ["MASTER_ADDR"] = keep
    return [r[1] for r in sorted(res, key=lambda r: r[0])]


@pytest.fixture(scope="module")
def vq2a_ranks():
    return _spawn("vq2a")


@pytest.fixture(scope="module")
def vq2b_ranks():
    return _spawn("vq2b")


@pytest.fixture(scope="module")
def vqvae2_ranks():
    return _spawn("vqvae2")


@pytest.fixture(scope="module")
def rccl_rank():
    return _spawn("rccl", world=1, backend="nccl")[0]


# ------------------------------------------------------------------ checks
def _key_kind(k):
    return k.split(".")[0]


def check_model_steps(kind, case, ranks):
    """`ranks`: _model_steps' result of every rank (rank order) for one case."""
    meta, arr = fixture(kind, case)
    assert meta["gap"] >= 1e-3
    ema = bool(meta["buffers"])
    world = len(ranks)
    for n in range(1, meta["steps"] + 1):
        p = f"s{n}."
        st = [r["steps"][n - 1] for r in ranks]
        for s in st:
            assert s["keys"] == meta["loss_keys"][n - 1] and s["total_is_loss"] and s["grads_are_views"]
            assert all(isinstance(v, float) for v in s["detail"].values())
            assert len(s["idx"]) == meta["lookups"][n - 1]
            assert sorted(s["grads"]) == sorted(meta["grads"])
        # each rank's lookups against its rows, bit-exact
        for j in range(meta["lookups"][n - 1]):
            got = np.concatenate([s["idx"][j] for s in st], axis=0)
            assert np.array_equal(got, arr[p + f"idx.{j}"]), (n, j)
        # collectives of a steady-state step: one bundle per EMA call and the gradient bucket
        if n > 1 or not ema:
            assert all(s["calls"] == (meta["lookups"][n - 1] if ema else 0) + 1 for s in st), [s["calls"] for s in st]
        # the reduced gradients and the EMA state are the same bits on every rank
        for s in st[1:]:
            assert all(np.array_equal(s["grads"][k], st[0]["grads"][k]) for k in st[0]["grads"]), n
            assert all(np.array_equal(s["bufs"][k], st[0]["bufs"][k]) for k in st[0]["bufs"]), n
        xhat = torch.from_numpy(np.concatenate([s["xhat"] for s in st], axis=0))
        for r, s in enumerate(st):
            got = {p + "xhat": xhat}
            for k in s["keys"]:
                if _key_kind(k) in MEAN_KEYS:
                    got[p + "loss." + k] = torch.tensor(np.mean([t["detail"][k] for t in st]), dtype=torch.float64)
                elif ema:
                    assert _key_kind(k) in EMA_KEYS
                    got[p + "loss." + k] = torch.tensor(s["detail"][k], dtype=torch.float64)
                # (a plain level's entropy.k is the rank's own shard's: no fixture value)
            got.update({p + "grad." + k: torch.from_numpy(g) for k, g in s["grads"].items()})
            got.update({p + "buf." + k: torch.from_numpy(b) for k, b in s["bufs"].items() if b.dtype.kind == "f"})
            want = {k: arr[k] for k in got if k not in meta["abs32"]}
            skipped = set() if ema else {p + "loss." + k for k in s["keys"] if _key_kind(k) not in MEAN_KEYS}
            assert set(want) | skipped == {k for k in meta["err32"] if k.startswith(p)}
            report(f"{kind} {case} step {n}, {world} ranks, rank {r}", ratios(got, want, meta["err32"]))
            for k, a32 in meta["abs32"].items():  # exactly zero in exact arithmetic
                if k.startswith(p):
                    scale = float(np.abs(arr[k[:-4] + "weight"]).max())
                    assert float(got[k].abs().max()) <= max(8 * a32, ULP16 * scale), k
            for k, b in s["bufs"].items():
                if b.dtype.kind != "f":
                    assert bool(b) == bool(arr[p + "buf." + k]), k
    assert all(r["state"] == ranks[0]["state"] for r in ranks)  # parameters and buffers, bit for bit


def check_valid(ranks):
    for r in ranks:
        v = r["valid"]
        assert v["calls"] == 0 and v["bytes"] == 0, v
        assert v["same"] and v["training"] and v["rng"] and v["finite"], v


@pytest.mark.parametrize("case", A_CASES)
def test_vqvae2a_two_ranks_match_the_float64_reference(vq2a_ranks, case):
    check_model_steps("vq2a", case, [r[case] for r in vq2a_ranks])


def test_vqvae2b_pooled_ema_two_ranks_match_the_float64_reference(vq2b_ranks):
    """Its pooled top level has one frame per utterance: N_global = 2 < K, the
    noisy tiling of the gathered global batch at init and at every update."""
    check_model_steps("vq2b", "pooled_ema", [r["pooled_ema"] for r in vq2b_ranks])


def test_valid_step_under_a_comm_issues_no_collective(vq2a_ranks, vq2b_ranks):
    for case in A_CASES:
        check_valid([r[case] for r in vq2a_ranks])
    check_valid([r["pooled_ema"] for r in vq2b_ranks])


def check_trainer_steps(case, ranks):
    from tests.test_gpu_hier_trainer import train_fixture
    tmeta, tarr = train_fixture(case)
    got, want = {}, {}
    for s in range(tmeta["forwards"]):
        for k in tmeta["loss_keys"]:
            if _key_kind(k) in MEAN_KEYS:
                got[f"{s}.{k}"] = torch.tensor(np.mean([r["details"][s][k] for r in ranks]), dtype=torch.float64)
                want[f"{s}.{k}"] = tarr[f"loss.{s}.{k}"]
        want[f"{s}.norm"] = tarr[f"norm.{s}"]
    for r in ranks:
        assert r["keys"] == tmeta["loss_keys"] and r["opt_step"] == tmeta["forwards"]
        assert len(r["levels"]) == tmeta["levels"]
        assert r["norms"] == ranks[0]["norms"]  # the norm of the one averaged gradient
        assert all(b >= 4 * r["n_params"] for b in r["bytes"])
    for s in range(tmeta["forwards"]):
        for k, i in enumerate(ranks[0]["levels"]):
            idx = np.concatenate([r["idx"][i][s] for r in ranks], axis=0)
            assert np.array_equal(idx, tarr[f"idx.{s}.{k}"]), (s, k, i)
        got[f"{s}.norm"] = torch.tensor(ranks[0]["norms"][s], dtype=torch.float64).reshape(())
    report(f"vqtrain {case} fp32, {len(ranks)} ranks", ratios(got, want, tmeta["err32"]))
    for r in ranks[1:]:
        assert (r["p"], r["m"], r["v"]) == (ranks[0]["p"], ranks[0]["m"], ranks[0]["v"])


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_vqvae2_trainer_two_ranks_match_the_float64_reference(vqvae2_ranks, case):
    check_trainer_steps(case, [r[case] for r in vqvae2_ranks])


def test_grad_sync_end_and_overlap_give_the_same_bits(vqvae2_ranks):
    for r in vqvae2_ranks:
        a, b = r["gst"], r["gst_end"]
        assert (a["grad_sync"], a["overlap"], b["grad_sync"], b["overlap"]) == ("overlap", True, "end", False)
        assert (a["p"], a["m"], a["v"]) == (b["p"], b["m"], b["v"])
        assert a["details"] == b["details"] and a["norms"] == b["norms"]
    check_trainer_steps("gst", [r["gst_end"] for r in vqvae2_ranks])


def test_rccl_world1_comm_equals_the_plain_trainer(rccl_rank):
    r = rccl_rank
    assert r["backend"] == "nccl"
    plain, ddp = r["plain"], r["ddp"]
    assert plain["overlap"] is None and ddp["overlap"] is True
    assert (ddp["p"], ddp["m"], ddp["v"]) == (plain["p"], plain["m"], plain["v"])  # an AVG over one rank: the identity
    assert ddp["details"] == plain["details"] and ddp["norms"] == plain["norms"]
    assert ddp["bytes"] == [4 * ddp["n_params"]] * len(ddp["bytes"])  # the flat gradient, once per step
    assert plain["bytes"] == [0] * len(plain["bytes"])
    check_trainer_steps("gst", [ddp])
    # the EMA levels' bundle on device tensors (a stream wait, not a host wait)
    check_model_steps("vq2a", "ema_gst", [r["ema"]])
    check_valid([r["ema"]])
