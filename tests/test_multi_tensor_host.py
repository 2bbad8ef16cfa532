"""The multi-tensor optimizer pair without a GPU: the Python-side layout
(ops.multi_layout: dense offsets, the position of every partial, the launch
groups) covers every element exactly once, the library counts the same
chunks, both entry points have ctypes signatures at ABI 130, and bad
arguments are refused on the host before any launch."""
import ctypes
import re

import pytest

from tests.helpers import ROOT

LIST_A = [1, 3, 4, 5, 4095, 4096, 4097, 8193]


def list_b(ops):
    n = [1 + i % 7 for i in range(ops.MULTI_MAX_TENSORS + 2)]
    n[ops.MULTI_MAX_TENSORS - 1] = 4097
    return n


def _ops():
    from vae_npvc_amd import ops
    return ops


@pytest.mark.parametrize("which", ["A", "B", "empty_tensors"])
def test_layout_covers_every_element_once(which):
    ops = _ops()
    numels = {"A": LIST_A, "B": list_b(ops), "empty_tensors": [0, 5, 0, 4096, 0]}[which]
    offsets, first, n_part = ops.multi_layout(numels)
    total = sum(numels)
    seen = [0] * total
    owner = [None] * n_part
    for i, (n, off, f) in enumerate(zip(numels, offsets, first)):
        chunks = -(-n // ops.MULTI_CHUNK)
        for c in range(chunks):
            assert owner[f + c] is None
            owner[f + c] = i
            lo, hi = c * ops.MULTI_CHUNK, min((c + 1) * ops.MULTI_CHUNK, n)
            assert lo < hi  # no empty chunk
            for e in range(off + lo, off + hi):
                seen[e] += 1
    assert all(s == 1 for s in seen)
    assert all(o is not None for o in owner) and owner == sorted(owner)  # tensor order, no gap
    # dense, in order, no padding: the offsets FusedOptimState walks
    assert offsets == [sum(numels[:i]) for i in range(len(numels))]
    # the launch groups: consecutive runs of at most MULTI_MAX_TENSORS tensors
    groups = [list(range(i, min(i + ops.MULTI_MAX_TENSORS, len(numels))))
              for i in range(0, len(numels), ops.MULTI_MAX_TENSORS)]
    assert sum(groups, []) == list(range(len(numels)))
    if which == "B":
        assert len(groups) == 2 and len(groups[1]) == 2
    # the library's own count (host only)
    plan = ops.MultiTensorPlan(numels)
    assert plan.n_partials == n_part and plan.offsets == offsets
    assert list(plan.numel_arr)[:len(numels)] == numels


def test_signatures_and_version():
    from vae_npvc_amd import _lib as L
    lib = L.load()
    for name in ("vqx_multi_sq_norm", "vqx_multi_adam_step", "vqx_multi_chunks"):
        assert name in L._SIGS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == L._SIGS[name]
    assert L.ABI_VERSION == 130 and lib.vqx_version() == 130
    text = (ROOT / "include" / "vqx.h").read_text()
    assert re.search(r"#define VQX_ABI_VERSION 130\b", text)
    m = re.search(r"#define VQX_MULTI_MAX_TENSORS (\d+)", text)
    assert m and int(m.group(1)) == _ops().MULTI_MAX_TENSORS
    m = re.search(r"#define VQX_MULTI_CHUNK (\d+)", text)
    assert m and int(m.group(1)) == _ops().MULTI_CHUNK


def test_host_rejections():
    """Refused before any launch (no GPU is touched): a partial count that does
    not match, ranges out of order or past the flat buffer, a gradient pointer
    that is not 4-B aligned, an unknown kind."""
    from vae_npvc_amd import _lib as L
    a = ctypes.addressof
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    numel, off, g = i64(5, 4097), i64(0, 5), ptrs(None, None)
    odd, overlap, neg = ptrs(fake + 2, None), i64(0, 4), i64(3, -1)  # (kept alive: addressof holds no reference)
    with pytest.raises(L.VqxError, match="partials"):
        L.call("vqx_multi_sq_norm", a(g), a(numel), 2, fake, 2, None)
    with pytest.raises(L.VqxError, match="4-B"):
        L.call("vqx_multi_sq_norm", a(odd), a(numel), 2, fake, 3, None)
    with pytest.raises(L.VqxError, match="kind"):
        L.call("vqx_multi_adam_step", fake, fake, fake, 4102, a(off), a(numel), a(g), 2, fake, None, 1.0, 2, None)
    with pytest.raises(L.VqxError, match="range"):  # past the end
        L.call("vqx_multi_adam_step", fake, fake, fake, 4101, a(off), a(numel), a(g), 2, fake, None, 1.0, 0, None)
    with pytest.raises(L.VqxError, match="range"):  # overlapping
        L.call("vqx_multi_adam_step", fake, fake, fake, 8000, a(overlap), a(numel), a(g), 2, fake, None, 1.0, 0, None)
    with pytest.raises(L.VqxError, match="negative"):
        L.call("vqx_multi_chunks", a(neg), 2, ctypes.byref(ctypes.c_int64()))


def test_trainer_refuses_data_parallel_for_an_autograd_engine(monkeypatch):
    """With more than one rank, Trainer._setup_engine raises for an engine
    without a fused forward (the hierarchical model's) before any broadcast,
    not train unsynchronised."""
    from types import SimpleNamespace

    import vae_npvc_amd.trainer.basic as tb
    monkeypatch.setattr(tb.dist, "is_available", lambda: True)
    monkeypatch.setattr(tb.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(tb.dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(tb.dist, "broadcast", lambda *a, **k: pytest.fail("broadcast reached"))
    tr = object.__new__(tb.Trainer)
    tr.device, tr.grad_sync, tr.scheduler_cfg = "cuda", "overlap", None
    tr.model = SimpleNamespace(engine=lambda dev: SimpleNamespace(fused_forward=False))
    with pytest.raises(NotImplementedError, match="data parallel"):
        tr._setup_engine()
