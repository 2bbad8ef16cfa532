"""Data parallel for the hierarchical models without a GPU: vqx_multi_pack
refuses bad arguments on the host before any launch, the EMA levels' global
code-row draw (model/layers_vq.py draw_code_rows with a comm) assembles the
single-process draw of the concatenated batch bit for bit and leaves the CPU
generator where one process leaves it, and Trainer._setup_engine attaches a
Comm to an engine that declares `data_parallel` and keeps refusing one that
declares nothing."""
import ctypes
from types import SimpleNamespace

import pytest
import torch


def test_multi_pack_signature_and_host_rejections():
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd import ops
    lib = L.load()
    assert "vqx_multi_pack" in L._SIGS and lib.vqx_multi_pack.argtypes == L._SIGS["vqx_multi_pack"]
    assert callable(ops.multi_pack)
    a = ctypes.addressof
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    numel, off, g = i64(5, 4097), i64(0, 5), ptrs(None, None)
    odd, overlap, neg = ptrs(fake + 2, None), i64(0, 4), i64(3, -1)  # (kept alive: addressof holds no reference)
    with pytest.raises(L.VqxError, match="bad arguments"):  # a null flat
        L.call("vqx_multi_pack", None, 4102, a(off), a(numel), a(g), 2, None)
    with pytest.raises(L.VqxError, match="range"):  # past the end
        L.call("vqx_multi_pack", fake, 4101, a(off), a(numel), a(g), 2, None)
    with pytest.raises(L.VqxError, match="range"):  # overlapping
        L.call("vqx_multi_pack", fake, 8000, a(overlap), a(numel), a(g), 2, None)
    with pytest.raises(L.VqxError, match="negative"):
        L.call("vqx_multi_pack", fake, 8000, a(off), a(neg), a(g), 2, None)
    with pytest.raises(L.VqxError, match="4-B"):  # an odd gradient pointer
        L.call("vqx_multi_pack", fake, 4102, a(off), a(numel), a(odd), 2, None)
    with pytest.raises(L.VqxError, match="4-B"):  # an odd flat
        L.call("vqx_multi_pack", fake + 2, 4102, a(off), a(numel), a(g), 2, None)


class FakeComm:
    """world 2; all_gather_cat returns the given global frames (rank order)."""

    def __init__(self, rank, z_global):
        self.world, self.rank, self.z_global = 2, rank, z_global
        self.gathers = 0

    def all_gather_cat(self, t):
        n = t.shape[0]
        assert torch.equal(t, self.z_global[self.rank * n:(self.rank + 1) * n])
        self.gathers += 1
        return self.z_global.clone()


def _rows(zf, perm, rows):
    """What the device path puts into the SUM all-reduce: ops.gather_rows_host's
    zf[perm] with zero rows for -1, or the tiled rows as drawn."""
    if rows is not None:
        return rows
    out = torch.zeros(perm.numel(), zf.shape[1])
    own = perm >= 0
    out[own] = zf[perm[own].long()]
    return out


@pytest.mark.parametrize("n_local,K", [(24, 16), (8, 16), (16, 16), (1, 16), (3, 16)])
def test_global_code_row_draw_assembles_the_single_process_draw(n_local, K):
    """N_global = 2 * n_local: 48, 16 and 32 frames take the permutation path
    (16 = K is its edge), 2 and 6 frames the noisy tiling of the gathered batch
    (2 = the pooled one-frame top level)."""
    from vae_npvc_amd.model.layers_vq import draw_code_rows
    D = 64
    z = torch.randn(2 * n_local, D, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(77)
    perm, rows = draw_code_rows(z, K)
    want = _rows(z, perm, rows)
    state = torch.get_rng_state()
    tiled = 2 * n_local < K
    assert (rows is not None) == tiled
    total = torch.zeros(K, D)
    for rank in range(2):
        zl = z[rank * n_local:(rank + 1) * n_local]
        comm = FakeComm(rank, z)
        torch.manual_seed(77)
        p, r = draw_code_rows(zl, K, comm, summed=True)
        assert torch.equal(torch.get_rng_state(), state)  # consumed as one process consumes it
        assert (r is not None) == tiled and comm.gathers == int(tiled)
        if p is not None:
            assert p.dtype == torch.int32 and int(p.min()) >= -1 and int(p.max()) < n_local
        total += _rows(zl, p, r)
        # init_emb's form: with the tiling every rank holds all K rows
        torch.manual_seed(77)
        p0, r0 = draw_code_rows(zl, K, FakeComm(rank, z))
        if tiled:
            assert torch.equal(r0, want)
        else:
            assert torch.equal(p0, p)
    assert torch.equal(total, want)  # x + 0 = x: the sum over ranks is bit-exact


def _trainer(monkeypatch, engine, log):
    import vae_npvc_amd.parallel.ddp as ddp
    import vae_npvc_amd.trainer.basic as tb
    monkeypatch.setattr(tb.dist, "is_available", lambda: True)
    monkeypatch.setattr(tb.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(tb.dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(tb.dist, "broadcast", lambda t, src: log.append(("broadcast", t)))
    monkeypatch.setattr(ddp.dist, "get_rank", lambda *a: 1)
    monkeypatch.setattr(ddp.dist, "get_backend", lambda *a: "gloo")
    tr = object.__new__(tb.Trainer)
    tr.device, tr.grad_sync, tr.scheduler_cfg = "cuda", "end", None
    tr.learning_rate, tr.max_grad_norm, tr.optim_kind = 1e-3, 5, "adam"
    tr.model = SimpleNamespace(engine=lambda dev: engine, buffers=lambda: ["buf0", "buf1"])
    return tr


def test_setup_engine_attaches_a_comm_to_a_data_parallel_engine(monkeypatch):
    from vae_npvc_amd.parallel.ddp import Comm
    log = []
    engine = SimpleNamespace(fused_forward=False, data_parallel=True, flat_p="flat_p",
                             attach_comm=lambda c: log.append(("attach", c)),
                             invalidate_packed=lambda: log.append(("invalidate",)),
                             init_optimizer=lambda *a, **k: log.append(("init_optimizer",)))
    tr = _trainer(monkeypatch, engine, log)
    tr._setup_engine()
    assert [e[0] for e in log] == ["attach", "broadcast", "broadcast", "broadcast", "invalidate", "init_optimizer"]
    comm = log[0][1]
    assert isinstance(comm, Comm) and comm.world == 2 and comm.rank == 1 and comm.overlap is False
    assert [e[1] for e in log[1:4]] == ["flat_p", "buf0", "buf1"]


def test_setup_engine_refuses_an_engine_that_declares_nothing(monkeypatch):
    log = []
    engine = SimpleNamespace(fused_forward=False, attach_comm=lambda c: log.append(("attach", c)))
    tr = _trainer(monkeypatch, engine, log)
    with pytest.raises(NotImplementedError, match="data parallel"):
        tr._setup_engine()
    assert log == []  # refused before attach_comm and before any broadcast
