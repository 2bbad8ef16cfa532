"""Thin tensor-level wrappers over the libvqx C ABI (device tensors in, no
allocation inside the kernels).  Every function here launches HIP kernels on
torch's current stream; there is no CPU path.

Layout convention: activations are frame-major 2-D tensors [N = B*T, C]
(the reference's (B, C, T) transposed), weights of a conv are "packed
effective" [cout, ntaps*cin] (see include/vqx.h).
"""
import ctypes

import torch

from . import _lib as L
from ._lib import call, ptr, stream_ptr

_DT = {torch.float32: L.VQX_F32, torch.bfloat16: L.VQX_BF16}


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise L.VqxError(f"unsupported dtype {dtype}") from None


def _check_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.VqxError("libvqx ops need device tensors (the HIP kernels are the only implementation)")


# ---- host extent checks (debug mode; vae_npvc_amd/debug.py)
_debug = False
_logical_end = {}  # guarded allocations: storage data_ptr -> bytes of the storage that belong to the buffer


def set_debug_checks(on):
    """Check every pointer argument's span against its tensor's storage before
    the calls below (off by default: a few microseconds of host time per call).
    Returns the previous setting."""
    global _debug
    prev, _debug = _debug, bool(on)
    return prev


def _span(t, elems, what):
    """`t` must hold `elems` elements from its data pointer on."""
    if not _debug or t is None or elems <= 0:
        return
    st = t.untyped_storage()
    end = _logical_end.get(st.data_ptr(), st.nbytes())
    avail = (end - t.storage_offset() * t.element_size()) // t.element_size()
    if elems > avail:
        raise L.VqxError(f"extent check: {what} needs {elems} elements from its pointer, its buffer holds {avail}")


def _rows(t, rows, ld, cols, what):
    if rows > 0 and t is not None:
        _span(t, (rows - 1) * ld + cols, what)


def _conv_extents(x, w, y, a, bias, rowbias, res, mask, out2, y2, colsum, stats, tiles, gn_h, gn_mr):
    n, cout, cin = a.n_rows, a.cout, a.cin
    split = a.split_col if out2 is not None else 0
    tm = (n + 127) // 128
    _rows(x, n, a.ldx, cin, "conv x")
    _span(w, cout * a.ntaps * cin, "conv w")
    _rows(y, n, a.ldy, split or cout, "conv y")
    _span(bias, cout, "conv bias")
    _span(rowbias, (n // max(1, a.T)) * max(1, a.rowbias_T) * cout, "conv rowbias")
    _rows(res, n, a.ldres, split or cout, "conv res")
    _rows(mask, n, a.ldmask, cout, "conv mask")
    _rows(out2, n, a.ldo2, cout - split, "conv out2")
    _rows(y2, n, a.ldy2, cout, "conv y2")
    _span(colsum, tm * cout, "conv colsum_part")
    _span(stats, (n // 128) * ((cout + 127) // 128) * 4, "conv stat_part")
    _span(tiles, (n // 128) * ((cout + 127) // 128) * 4, "conv gn_stat_tiles")
    _rows(gn_h, n, a.ldgn, cout * (2 if a.gn_glu else 1), "conv gn_h")
    _span(gn_mr, (n // max(1, a.T)) * 2 * max(1, a.gn_groups), "conv gn_mean_rstd")


POLICY_AUTO, POLICY_IM2COL, POLICY_TALL256, POLICY_TALL512, POLICY_TR128, POLICY_K1_2PCU = 0, 1, 2, 3, 4, 5  # vqx.h
_policy = POLICY_AUTO


def set_kernel_policy(policy):
    """Policy for the conv GEMM calls that pass no `policy` (include/vqx.h
    VQX_POLICY_*; for tests and A/B tools -- the library itself keeps no such
    state: the policy travels in every call's arguments).  Returns the old one."""
    global _policy
    if policy not in (POLICY_AUTO, POLICY_IM2COL, POLICY_TALL256, POLICY_TALL512, POLICY_TR128, POLICY_K1_2PCU):
        raise ValueError(f"kernel policy {policy} not in 0..5")
    prev, _policy = _policy, int(policy)
    return prev


class kernel_policy:
    """with ops.kernel_policy(p): set_kernel_policy(p) for the block."""

    def __init__(self, policy):
        self.policy = policy

    def __enter__(self):
        self.prev = set_kernel_policy(self.policy)
        return self

    def __exit__(self, *exc):
        set_kernel_policy(self.prev)
        return False


def conv_args(x, w, y, *, T, cin, cout, ntaps, pad, prologue=L.PRO_NONE, pro_scale=1.0, bias=None,
              rowbias=None, res=None, mask=None, mask_slope=0.0, mask_scale=1.0, gn_h=None, gn_mr=None,
              gn_gamma=None, gn_beta=None, out2=None, split_col=0, out2_accumulate=False, out_f32=False,
              act=None, y2=None, colsum=None, gn_stats=None, gn_bwd=None, gn_groups=1, gn_glu=False,
              gn_tiles=None, gn_eps=1e-5, dil=1, policy=None, rowbias_T=0):
    epi = 0
    if bias is not None:
        epi |= L.EPI_BIAS
    if rowbias is not None:
        epi |= L.EPI_ROWBIAS
    if mask is not None:
        epi |= L.EPI_MASK
    if res is not None:
        epi |= L.EPI_RES
    if gn_h is not None and gn_bwd is None:  # GNBWD reads gn_* as the forward GN's operands
        epi |= L.EPI_GNADD
    if out2 is not None:
        epi |= L.EPI_SPLIT
    if out_f32:
        epi |= L.EPI_OUTF32
    if act is not None and y2 is None:
        epi |= L.EPI_ACT
    if y2 is not None:
        epi |= L.EPI_ACT2
    if colsum is not None:
        epi |= L.EPI_COLSUM
    if gn_stats is not None:
        epi |= L.EPI_GNSTATS
    if gn_bwd is not None:
        epi |= L.EPI_GNBWD
    a = L.ConvArgs()
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
    a.bias, a.rowbias, a.res, a.mask = ptr(bias), ptr(rowbias), ptr(res), ptr(mask)
    a.gn_h, a.gn_mean_rstd, a.gn_gamma, a.gn_beta, a.out2 = ptr(gn_h), ptr(gn_mr), ptr(gn_gamma), ptr(gn_beta), ptr(out2)
    a.n_rows, a.T, a.cin, a.cout, a.ntaps, a.pad, a.dil = x.shape[0], T, cin, cout, ntaps, pad, dil
    a.kernel_policy = _policy if policy is None else policy
    a.rowbias_T = rowbias_T  # > 1: rowbias [B*rowbias_T, cout], one row per stretch segment (forward only)
    a.ldx, a.ldy = x.stride(0), y.stride(0)
    a.ldres = res.stride(0) if res is not None else 0
    a.ldmask = mask.stride(0) if mask is not None else 0
    a.ldgn = gn_h.stride(0) if gn_h is not None else 0
    a.ldo2 = out2.stride(0) if out2 is not None else 0
    a.dtype = dt_code(x.dtype)
    a.prologue, a.epilogue = prologue, epi
    a.split_col, a.out2_accumulate = split_col, int(bool(out2_accumulate))
    a.pro_scale, a.mask_slope, a.mask_scale = pro_scale, mask_slope, mask_scale
    a.y2, a.ldy2 = ptr(y2), (y2.stride(0) if y2 is not None else 0)
    a.epi_act = act if act is not None else 0
    a.colsum_part = ptr(colsum)
    a.gn_stat_tiles, a.gn_eps = ptr(gn_tiles), gn_eps
    a.stat_part = ptr(gn_stats if gn_stats is not None else gn_bwd)
    a.gn_groups, a.gn_glu = gn_groups, int(gn_glu)
    if _debug:
        _conv_extents(x, w, y, a, bias, rowbias, res, mask, out2, y2, colsum,
                      gn_stats if gn_stats is not None else gn_bwd, gn_tiles, gn_h, gn_mr)
    return a


class LaunchProbe:
    """Per-launch timing of the conv GEMM kernels (bench.py's roofline leg).
    libvqx launches each GEMM with hipExtLaunchKernelGGL and a start/stop
    event pair stamped on the kernel's own dispatch (vqx_probe_*), on the
    stream the kernel runs on; this class only labels and aggregates."""

    _DT = {L.VQX_F32: "float", L.VQX_BF16: "unsigned short"}

    def __init__(self):
        self.shapes = []

    def clear(self):
        self.shapes = []
        call("vqx_probe_clear")

    def start(self):
        """Resume recording (the log is kept; clear() empties it)."""
        call("vqx_probe_enable", 1)

    def stop(self):
        call("vqx_probe_enable", 0)

    def select(self, info=None):
        """Record only launches of the kernel with this 5-int info (records()[i][4]);
        None = all.  Other launches skip the event pair and its queue cost."""
        if info is None:
            call("vqx_probe_select", None)
        else:
            self._sel = (ctypes.c_int32 * 5)(*info)
            call("vqx_probe_select", self._sel)

    def records(self):
        """[(rocprof symbol, flops, seconds, shape label, info5)] after a device sync."""
        torch.cuda.synchronize()
        n = ctypes.c_int64()
        call("vqx_probe_count", ctypes.byref(n))
        info = (ctypes.c_int32 * 5)()
        fl, ms = ctypes.c_double(), ctypes.c_float()
        out = []
        for i in range(n.value):
            call("vqx_probe_read", i, info, ctypes.byref(fl), ctypes.byref(ms))
            dt, mode, pro, gen, ek = list(info)  # ek: epilogue kind (vqx_gemm_kernel.h EK_*)
            bk = 64 if dt == L.VQX_BF16 else 32
            if gen == 5:  # data + weight gradient in one launch (vqx_gemm_dual.hip)
                sym = {2: f"vqx::dual_tr_kernel<{ek}>", 3: f"vqx::dual_k1_kernel<{ek}>"}.get(pro, "vqx::dual_kernel")
            elif gen == 4:  # three workgroups per CU (vqx_gemm_kernel.h conv_gemm3_kernel)
                sym = f"vqx::conv_gemm3_kernel<{self._DT[dt]}, {mode}, {pro}, false, {ek}>"
            elif gen == 6:  # ping-pong tap-reuse kernel (vqx_gemm_pp.h conv_pp_kernel)
                sym = f"vqx::conv_pp_kernel<{mode}, {ek}, {pro}, 2>"  # pro slot = frame segments
            elif gen == 2 and mode == 2:  # tap-reuse weight gradient (vqx_gemm_kernel.h wgrad_tr_kernel)
                sym = f"vqx::wgrad_tr_kernel<{ek}, {pro}>"  # pro slot = K groups
            elif gen == 3:  # tall tap-reuse kernel (vqx_gemm_kernel.h conv_tr8_kernel)
                sym = f"vqx::conv_tr8_kernel<{mode}, {ek}, {pro}>"  # pro slot = frame segments
            elif gen == 2:  # tap-reuse kernel (3-tap FWD/DGRAD, vqx_gemm_kernel.h conv_tr_kernel)
                sym = f"vqx::conv_tr_kernel<{mode}, {ek}, {pro}>"  # pro slot = channels per stage
            else:
                sym = f"vqx::conv_gemm_kernel<{self._DT[dt]}, {mode}, {pro}, {'true' if gen else 'false'}, {bk}, 2, {ek}>"
            out.append((sym, fl.value, ms.value * 1e-3, self.shapes[i] if i < len(self.shapes) else "",
                        (dt, mode, pro, gen, ek)))
        return out

    def summary(self, by_shape=False):
        """Aggregate per kernel symbol (by_shape: per symbol and layer shape)."""
        agg = {}
        for key, fl, sec, shape, _ in self.records():
            if by_shape:
                key = f"{key} {shape}"
            a = agg.setdefault(key, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += fl
            a[2] += sec
        return {k: {"launches": n, "flops": f, "seconds": t, "avg_us": 1e6 * t / n, "tflops": f / t / 1e12}
                for k, (n, f, t) in agg.items()}


_probe = None


def set_probe(p):
    """Install (p.start()) or remove (None) the GEMM launch probe."""
    global _probe
    if _probe is not None and p is None:
        _probe.stop()
    _probe = p
    if p is not None:
        p.start()


def conv_fwd(x, w, y, **kw):
    """y = epi(conv(pro(x), w)); x [N, cin], w packed [cout, ntaps*cin], y [N, cout]."""
    _check_cuda(x, w, y)
    a = conv_args(x, w, y, **kw)
    if _probe is not None:
        _probe.shapes.append(f"{a.cin}->{a.cout} k{a.ntaps} epi{a.epilogue}")
    call("vqx_conv1d_fwd", ctypes.byref(a), stream_ptr())
    return y


def conv_dgrad(dy, w, dx, **kw):
    """dx = epi(conv_transpose(dy, w)); dy [N, cout_f], w packed [cout_f, ntaps*cin_f], dx [N, cin_f].
    Pass cin=cout_f, cout=cin_f."""
    _check_cuda(dy, w, dx)
    a = conv_args(dy, w, dx, **kw)
    if _probe is not None:
        _probe.shapes.append(f"{a.cin}->{a.cout} k{a.ntaps} epi{a.epilogue}")
    call("vqx_conv1d_dgrad", ctypes.byref(a), stream_ptr())
    return dx


def wgrad_args(p, q, slabs, *, T, r_dim, c_dim, ntaps, pad, shift_sign=1, q_prologue=L.PRO_NONE, pro_scale=1.0,
               splits=1, dil=1, policy=None, fixup_dw=None, fixup_counters=None):
    a = L.WgradArgs()
    a.kernel_policy = _policy if policy is None else policy
    a.p, a.q, a.slabs = ptr(p), ptr(q), ptr(slabs)
    a.n_rows, a.T, a.r_dim, a.c_dim, a.ntaps, a.pad, a.shift_sign = p.shape[0], T, r_dim, c_dim, ntaps, pad, shift_sign
    a.ldp, a.ldq = p.stride(0), q.stride(0)
    a.dtype, a.q_prologue, a.splits, a.pro_scale, a.dil = dt_code(p.dtype), q_prologue, splits, pro_scale, dil
    a.slab_dtype = dt_code(slabs.dtype)
    a.fixup_dw, a.fixup_counters = ptr(fixup_dw), ptr(fixup_counters)
    if _debug:
        _span(fixup_dw, r_dim * ntaps * c_dim, "wgrad fixup_dw")
        _rows(p, a.n_rows, a.ldp, r_dim, "wgrad p")
        _rows(q, a.n_rows, a.ldq, c_dim, "wgrad q")
        _span(slabs, splits * r_dim * ntaps * c_dim, "wgrad slabs")
    return a


def conv_wgrad(p, q, slabs, **kw):
    """slabs[s, r, j*c_dim + c] = sum_{n in split s} p[n, r] * pro(q[n + sign*(j*dil-pad), c]);
    slabs fp32, or bf16 for bf16 operands (each split's partial rounded once).
    Keywords: T, r_dim, c_dim, ntaps, pad, shift_sign, q_prologue, pro_scale, splits, dil."""
    _check_cuda(p, q, slabs)
    a = wgrad_args(p, q, slabs, **kw)
    if _probe is not None:
        _probe.shapes.append(f"{a.r_dim}x{a.ntaps}x{a.c_dim} s{a.splits}")
    call("vqx_conv1d_wgrad", ctypes.byref(a), stream_ptr())
    return slabs


def conv_dgrad_wgrad(dy, w, dx, dgrad_kw, p, q, slabs, wgrad_kw):
    """conv_wgrad(p, q, slabs, **wgrad_kw) and conv_dgrad(dy, w, dx, **dgrad_kw)
    of one layer (same output gradient) through vqx_conv1d_dgrad_wgrad: one
    launch interleaving both GEMMs where a fused kernel covers the pair, else
    the two launches in that order.  Returns True when fused."""
    _check_cuda(dy, w, dx, p, q, slabs)
    ad = conv_args(dy, w, dx, **dgrad_kw)
    aw = wgrad_args(p, q, slabs, **wgrad_kw)
    fused = ctypes.c_int32(0)
    call("vqx_conv1d_dgrad_wgrad", ctypes.byref(ad), ctypes.byref(aw), ctypes.byref(fused), stream_ptr())
    if _probe is not None:
        sd = f"{ad.cin}->{ad.cout} k{ad.ntaps} epi{ad.epilogue}"
        sw = f"{aw.r_dim}x{aw.ntaps}x{aw.c_dim} s{aw.splits}"
        _probe.shapes.extend([f"dual {sd} + {sw}"] if fused.value else [sw, sd])
    return bool(fused.value)


def wgrad_tiles(n_rows, T, r_dim, c_dim, ntaps, pad, dtype, q_prologue=L.PRO_NONE, dil=1, policy=POLICY_AUTO):
    """Output tiles per split of the weight-gradient kernel conv_wgrad would
    launch under kernel policy `policy`."""
    t = ctypes.c_int32()
    call("vqx_wgrad_tiles", n_rows, T, r_dim, c_dim, ntaps, pad, dil, dtype, q_prologue, policy, ctypes.byref(t))
    return t.value


def _wn_extents(d):
    """Spans of one weight-norm table entry (include/vqx.h vqx_wn_layer)."""
    kind, cout, cin, k, s = d["kind"], d["cout"], d["cin"], d["k"], d.get("stride", 1) or 1
    if kind == L.WN_COLREDUCE:
        _span(d.get("v"), cin * cout, "colreduce src")
        _span(d.get("dv"), cout, "colreduce dst")
        return
    rows = cin if kind in (1, L.WN_RESAMPLE_T) else cout
    cols = (3 * s * cin if kind == L.WN_RESAMPLE else 3 * s * cout if kind == L.WN_RESAMPLE_T
            else (cout if kind == 1 else cin) * k)
    for key in ("v", "dv"):
        _span(d.get(key), cout * cin * k, f"weight-norm {key}")
    for key in ("g", "dg", "norm"):
        _span(d.get(key), rows, f"weight-norm {key}")
    _span(d.get("w_packed"), rows * cols, "weight-norm w_packed")
    _span(d.get("slabs"), d.get("splits", 1) * rows * cols, "weight-norm slabs")


def wgrad_fixup_ok(n_rows, T, r_dim, c_dim, ntaps, pad, dtype, slab_dtype, q_prologue=L.PRO_NONE, dil=1,
                   policy=POLICY_AUTO):
    """Whether conv_wgrad of this shape takes the in-launch split-K reduction (fixup_dw, ABI 127)."""
    ok = ctypes.c_int32()
    call("vqx_wgrad_fixup_ok", n_rows, T, r_dim, c_dim, ntaps, pad, dil, dtype, slab_dtype, q_prologue, policy,
         ctypes.byref(ok))
    return bool(ok.value)


def wn_table(layers):
    """Pack a list of dicts into a ctypes WNLayer array (host copy) and a device byte tensor copy."""
    arr = (L.WNLayer * len(layers))()
    for i, d in enumerate(layers):
        e = arr[i]
        for k in ("v", "g", "w_packed", "norm", "dv", "dg", "slabs"):
            setattr(e, k, ptr(d.get(k)))
        e.kind, e.cout, e.cin, e.k = d["kind"], d["cout"], d["cin"], d["k"]
        e.splits, e.dtype = d.get("splits", 1), d["dtype"]
        e.stride, e.pad = d.get("stride", 0), d.get("pad", 0)
        sl = d.get("slabs")
        e.slab_dtype = dt_code(sl.dtype) if sl is not None else L.VQX_F32
        if _debug:
            _wn_extents(d)
    raw = bytes(arr)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
    return arr, dev


def colreduce_entry(src, dst):
    """VQX_WN_COLREDUCE table entry: dst[c] = sum_r src[r][c] (src contiguous f32 [R][C])."""
    R, C = src.shape
    return dict(kind=L.WN_COLREDUCE, v=src, dv=dst, cin=R, cout=C, k=1, dtype=L.VQX_F32, splits=1)


def linear_table(layers):
    """Device table of vqx_linear_layer (host ctypes copy kept alive alongside)."""
    arr = (L.LinearLayer * len(layers))()
    for i, d in enumerate(layers):
        for k in ("W", "bias", "out", "dout", "dW", "dbias"):
            setattr(arr[i], k, ptr(d.get(k)))
    arr.ents = layers  # the tensors behind the pointers (debug extent checks)
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to("cuda")
    return arr, dev


def _linear_extents(arr, B, I, O, dc=None, partials=None):
    if not _debug:
        return
    for d in arr.ents:
        _span(d.get("W"), O * I, "linear W")
        _span(d.get("dW"), O * I, "linear dW")
        for key in ("bias", "dbias"):
            _span(d.get(key), O, f"linear {key}")
        for key in ("out", "dout"):
            _span(d.get(key), B * O, f"linear {key}")
    _span(dc, B * I, "linear dc")
    _span(partials, len(arr) * ((O + 63) // 64) * B * I, "linear partials")


def linear_batched_fwd(table, c, B, I, O):
    arr, dev = table
    _linear_extents(arr, B, I, O)
    _span(c, B * I, "linear c")
    call("vqx_linear_batched_fwd", dev.data_ptr(), len(arr), ptr(c), B, I, O, stream_ptr())


def linear_ids_ok(B, I, O, emb):
    """Whether linear_batched_*_ids take this shape (vqx.h: I = 128, B <= 64, O % 64 == 0, aligned table)."""
    return I == 128 and 1 <= B <= 64 and O % 64 == 0 and emb.data_ptr() % 16 == 0


def linear_batched_fwd_ids(table, emb, ids, B, I, O):
    """linear_batched_fwd with c[b] = emb[ids[b]] (the embedding lookup in the operand loads)."""
    arr, dev = table
    _check_cuda(emb, ids)
    if ids.dtype != torch.int64 or ids.numel() != B:
        raise ValueError("linear_batched_fwd_ids: B int64 ids")
    _linear_extents(arr, B, I, O)
    call("vqx_linear_batched_fwd_ids", dev.data_ptr(), len(arr), ptr(emb), ptr(ids), B, I, O, stream_ptr())


def linear_batched_bwd_ids(table, emb, ids, B, I, O, dc, partials):
    arr, dev = table
    _check_cuda(emb, ids)
    if ids.dtype != torch.int64 or ids.numel() != B:
        raise ValueError("linear_batched_bwd_ids: B int64 ids")
    _linear_extents(arr, B, I, O, dc, partials)
    call("vqx_linear_batched_bwd_ids", dev.data_ptr(), len(arr), ptr(emb), ptr(ids), B, I, O, ptr(dc), ptr(partials),
         stream_ptr())


def linear_batched_bwd(table, c, B, I, O, dc, partials=None):
    """partials: f32 workspace of >= len(table) * ceil(O/64) * B * I (allocated if None)."""
    arr, dev = table
    if dc is not None and partials is None:
        partials = torch.empty(len(arr) * ((O + 63) // 64) * B * I, device=c.device, dtype=torch.float32)
    _linear_extents(arr, B, I, O, dc, partials)
    _span(c, B * I, "linear c")
    call("vqx_linear_batched_bwd", dev.data_ptr(), len(arr), ptr(c), B, I, O, ptr(dc), ptr(partials), stream_ptr())


WNF_NORMS_READY = 1  # include/vqx.h VQX_WNF_NORMS_READY


def weight_norm_fwd(table, flags=0):
    arr, dev = table
    if flags:
        call("vqx_weight_norm_fwd_flags", ctypes.addressof(arr), dev.data_ptr(), len(arr), flags, stream_ptr())
    else:
        call("vqx_weight_norm_fwd", ctypes.addressof(arr), dev.data_ptr(), len(arr), stream_ptr())


def weight_norm_bwd(table, sq_partials=None):
    """sq_partials: also leave the sum of squares of every written gradient
    value as per-wave partials there (weight_norm_bwd_partials(table) floats)."""
    arr, dev = table
    if sq_partials is None:
        call("vqx_weight_norm_bwd", ctypes.addressof(arr), dev.data_ptr(), len(arr), stream_ptr())
        return
    _check_cuda(sq_partials)
    if _debug:
        _span(sq_partials, weight_norm_bwd_partials(table), "weight-norm sq partials")
    call("vqx_weight_norm_bwd_sq", ctypes.addressof(arr), dev.data_ptr(), len(arr), ptr(sq_partials),
         sq_partials.numel(), stream_ptr())


def weight_norm_bwd_partials(table):
    """Number of sum-of-squares partials weight_norm_bwd(table, sq) writes."""
    arr, _ = table
    n = ctypes.c_int64(0)
    call("vqx_weight_norm_bwd_partials", ctypes.addressof(arr), len(arr), ctypes.byref(n))
    return n.value


def sq_norm_finish(partials, g, ranges, out, scratch):
    """out[0] = sum(partials) + sum over ranges (int64 [n, 2] device tensor of
    (offset, length) into g) of g^2, in a fixed order; scratch >= 256 floats."""
    _check_cuda(partials, g, out, scratch)
    if scratch.numel() < 256:
        raise ValueError("sq_norm_finish: scratch needs 256 floats")
    nr = 0 if ranges is None else ranges.shape[0]
    if nr:
        _check_cuda(ranges)
        if ranges.dtype != torch.int64 or ranges.dim() != 2 or ranges.shape[1] != 2:
            raise ValueError("sq_norm_finish: ranges must be an int64 [n, 2] tensor")
    call("vqx_sq_norm_finish", ptr(partials), partials.numel(), ptr(g), ptr(ranges) if nr else None, nr, ptr(scratch),
         ptr(out), stream_ptr())
    return out


def sq_norm_finish_adam(partials, g, ranges, out, scratch, step, lr0, gamma, step_size, beta1, beta2, eps, hyper):
    """sq_norm_finish then adam_hyper, the second in the finish's last launch."""
    _check_cuda(partials, g, out, scratch, step, hyper)
    if scratch.numel() < 256:
        raise ValueError("sq_norm_finish_adam: scratch needs 256 floats")
    nr = 0 if ranges is None else ranges.shape[0]
    if nr:
        _check_cuda(ranges)
        if ranges.dtype != torch.int64 or ranges.dim() != 2 or ranges.shape[1] != 2:
            raise ValueError("sq_norm_finish_adam: ranges must be an int64 [n, 2] tensor")
    call("vqx_sq_norm_finish_adam", ptr(partials), partials.numel(), ptr(g), ptr(ranges) if nr else None, nr,
         ptr(scratch), ptr(out), ptr(step), lr0, gamma, step_size, beta1, beta2, eps, ptr(hyper), stream_ptr())
    return out


def groupnorm_stats(x, T, G, partials, mean_rstd, eps=1e-5):
    call("vqx_groupnorm_stats", ptr(x), x.stride(0), dt_code(x.dtype), x.shape[0], T, x.shape[1], G, eps,
         ptr(partials), ptr(mean_rstd), stream_ptr())
    return mean_rstd


def gn_lrelu_fwd(h, g, T, mean_rstd, gamma, beta):
    """g = LeakyReLU_0.2(GroupNorm_1(h)) with precomputed statistics mean_rstd [B, 2]."""
    call("vqx_gn_lrelu_fwd", ptr(h), h.stride(0), ptr(g), g.stride(0), dt_code(h.dtype), h.shape[0], T, h.shape[1],
         ptr(mean_rstd), ptr(gamma), ptr(beta), stream_ptr())


def gn_glu_fwd(u, g, T, mean_rstd, gamma, beta):
    call("vqx_gn_glu_fwd", ptr(u), u.stride(0), ptr(g), g.stride(0), dt_code(u.dtype), u.shape[0], T, u.shape[1],
         ptr(mean_rstd), ptr(gamma), ptr(beta), stream_ptr())
    return g


def gn_glu_fwd_tiles(u, g, T, parts, mean_rstd, gamma, beta, eps=1e-5):
    """gn_finalize_tiles(G=2) + gn_glu_fwd in one launch; writes mean_rstd."""
    call("vqx_gn_glu_fwd_tiles", ptr(u), u.stride(0), ptr(g), g.stride(0), dt_code(u.dtype), u.shape[0], T,
         u.shape[1], ptr(parts), eps, ptr(mean_rstd), ptr(gamma), ptr(beta), stream_ptr())
    return g


def gn_bwd(dy, u, du, T, G, glu, mean_rstd, gamma, beta, partials, colsum_b=None, dgamma_b=None, dbeta_b=None,
           nparts=0):
    """nparts > 0: `partials` already holds the producing GEMM's GNBWD tiles (nparts per utterance)."""
    call("vqx_gn_bwd", ptr(dy), dy.stride(0), ptr(u), u.stride(0), ptr(du), du.stride(0), dt_code(u.dtype),
         u.shape[0], T, u.shape[1], G, int(glu), ptr(mean_rstd), ptr(gamma), ptr(beta), ptr(partials), nparts,
         ptr(colsum_b), ptr(dgamma_b), ptr(dbeta_b), stream_ptr())
    return du


def gn_finalize_tiles(parts, n_rows, T, C, G, mean_rstd, eps=1e-5):
    call("vqx_gn_finalize_tiles", ptr(parts), n_rows, T, C, G, eps, ptr(mean_rstd), stream_ptr())
    return mean_rstd


def colsum(x, partials, out, accumulate=False, C=None):
    C = x.shape[1] if C is None else C
    call("vqx_colsum", ptr(x), x.stride(0), dt_code(x.dtype), x.shape[0], C, ptr(partials), ptr(out),
         int(accumulate), stream_ptr())
    return out


def colsum_parts(n_rows, C, dtype):
    """Row parts colsum_partials writes for an [n_rows, C] input of `dtype`."""
    n = ctypes.c_int32()
    call("vqx_colsum_parts", int(n_rows), int(C), dt_code(dtype), ctypes.byref(n))
    return n.value


def colsum_partials(x, partials):
    """partials[p][c] = sum over row part p of x[:, c] (the first level of colsum);
    `partials` is f32 [colsum_parts(...), C], to be reduced later (colreduce_entry)."""
    _check_cuda(x, partials)
    n, C = x.shape
    if tuple(partials.shape) != (colsum_parts(n, C, x.dtype), C) or not partials.is_contiguous():
        raise ValueError(f"colsum_partials: partials {tuple(partials.shape)} != ({colsum_parts(n, C, x.dtype)}, {C})")
    call("vqx_colsum_partials", ptr(x), x.stride(0), dt_code(x.dtype), n, C, ptr(partials), stream_ptr())
    return partials


def nct_to_ntc(x_nct, y):
    B, C, T = x_nct.shape
    call("vqx_nct_to_ntc", ptr(x_nct), B, C, T, ptr(y), y.stride(0), dt_code(y.dtype), stream_ptr())
    return y


def step_prologue(wn_table=None, cond=None, x_nct=None, y=None):
    """One launch for weight_norm_fwd(wn_table, flags=WNF_NORMS_READY),
    linear_batched_fwd_ids(*cond) and nct_to_ntc(x_nct, y), with their bits
    (vqx_step_prologue).  cond = (table, emb, ids, B, I, O); any job may be None."""
    wh, wd, nw = None, 0, 0
    if wn_table is not None:
        arr, dev = wn_table
        wh, wd, nw = ctypes.addressof(arr), dev.data_ptr(), len(arr)
    cd, nc, emb_p, ids_p, B, I, O = 0, 0, 0, 0, 0, 0, 0
    if cond is not None:
        (arr, dev), emb, ids, B, I, O = cond
        _check_cuda(emb, ids)
        if ids.dtype != torch.int64 or ids.numel() != B:
            raise ValueError("step_prologue: B int64 ids")
        _linear_extents(arr, B, I, O)
        cd, nc, emb_p, ids_p = dev.data_ptr(), len(arr), ptr(emb), ptr(ids)
    xp, xB, C, T, yp, ldy, ydt = 0, 0, 0, 0, 0, 0, 0
    if x_nct is not None:
        _check_cuda(x_nct, y)
        xB, C, T = x_nct.shape
        if not x_nct.is_contiguous() or y.dim() != 2 or y.shape[0] != xB * T or y.shape[1] < C or y.stride(1) != 1:
            raise ValueError(f"step_prologue: x {tuple(x_nct.shape)} into y {tuple(y.shape)}")
        xp, yp, ldy, ydt = ptr(x_nct), ptr(y), y.stride(0), dt_code(y.dtype)
    call("vqx_step_prologue", wh, wd, nw, cd, nc, emb_p, ids_p, B, I, O, xp, xB, C, T, yp, ldy, ydt, stream_ptr())


def ntc_to_nct(y, x_nct):
    B, C, T = x_nct.shape
    call("vqx_ntc_to_nct", ptr(y), y.stride(0), dt_code(y.dtype), B, C, T, ptr(x_nct), stream_ptr())
    return x_nct


def logloss_fwd_bwd(x_nct, xhat, grad_scale, dxhat, loss_out, partials):
    B, C, T = x_nct.shape
    call("vqx_logloss_fwd_bwd", ptr(x_nct), ptr(xhat), xhat.stride(0), B, C, T, grad_scale, ptr(dxhat),
         dxhat.stride(0) if dxhat is not None else 0, dt_code(dxhat.dtype) if dxhat is not None else 0,
         ptr(loss_out), ptr(partials), stream_ptr())
    return loss_out


def logloss_parts(x_nct, xhat, grad_scale, dxhat, partials):
    """logloss_fwd_bwd without its final sum launch: the per-workgroup partials
    only; returns their count (vq_ema_update(close=...) sums them)."""
    B, C, T = x_nct.shape
    n = ctypes.c_int32(0)
    call("vqx_logloss_parts", ptr(x_nct), ptr(xhat), xhat.stride(0), B, C, T, grad_scale, ptr(dxhat),
         dxhat.stride(0) if dxhat is not None else 0, dt_code(dxhat.dtype) if dxhat is not None else 0,
         ptr(partials), ctypes.byref(n), stream_ptr())
    if n.value > partials.numel():
        raise L.VqxError(f"logloss_parts: {n.value} partials written into a buffer of {partials.numel()}")
    return n.value


def logloss_fwd_bwd_x(x_nct, xhat, grad_scale, dxhat, loss_out, partials, extra_partials, extra_out):
    """logloss_fwd_bwd, and extra_out[0] = the sum of extra_partials in the same
    final launch (the VQ kernel's commitment partials: VQ_FRAMES frames each)."""
    B, C, T = x_nct.shape
    _check_cuda(extra_partials, extra_out)
    call("vqx_logloss_fwd_bwd_x", ptr(x_nct), ptr(xhat), xhat.stride(0), B, C, T, grad_scale, ptr(dxhat),
         dxhat.stride(0) if dxhat is not None else 0, dt_code(dxhat.dtype) if dxhat is not None else 0,
         ptr(loss_out), ptr(partials), ptr(extra_partials), extra_partials.numel(), ptr(extra_out), stream_ptr())
    return loss_out


VQ_FRAMES = 32  # frames per commitment partial of vqx_vq_forward (vqx_vq.hip VQ_FRAMES)


def vq_workspace(n_rows, K, stats, D=128):
    """Floats of workspace vqx_vq_forward needs for K codes of width D (with or
    without EMA statistics)."""
    out = ctypes.c_int64()
    call("vqx_vq_workspace", int(n_rows), int(K), int(D), int(bool(stats)), ctypes.byref(out))
    return out.value


def vq_forward(z, E, idx, zq, zq_c, sqerr, partials=None, bsum=None, bcnt=None):
    """partials: f32 workspace of >= vq_workspace(N, K, bsum is not None, D) floats (allocated if None)."""
    N, D = z.shape
    need = vq_workspace(N, E.shape[0], bsum is not None, D)
    if partials is None:
        partials = torch.empty(need, device=z.device, dtype=torch.float32)
    if partials.numel() < need:
        raise ValueError(f"vq_forward: workspace {partials.numel()} < {need} floats")
    if _debug:
        K = E.shape[0]
        for t, n, what in ((idx, N, "idx"), (zq, N * D, "zq"), (zq_c, N * D, "zq_c"), (bsum, K * D, "bsum"),
                           (bcnt, K, "bcnt"), (E, K * D, "codebook")):
            _span(t, n, f"vq_forward {what}")
    call("vqx_vq_forward", ptr(z), N, D, ptr(E), E.shape[0], ptr(idx), ptr(zq), ptr(zq_c),
         dt_code(zq_c.dtype) if zq_c is not None else 0, ptr(sqerr), ptr(partials), ptr(bsum), ptr(bcnt),
         stream_ptr())


def vq_stats(z, idx, K, partials, bsum, bcnt):
    """EMA statistics alone (vqx_vq_stats): bsum [K, D] = sum of the frames per
    code, bcnt [K] = counts; partials as vq_forward's workspace with stats."""
    N, D = z.shape
    need = vq_workspace(N, K, True, D)
    if partials.numel() < need:
        raise ValueError(f"vq_stats: workspace {partials.numel()} < {need} floats")
    call("vqx_vq_stats", ptr(z), N, D, ptr(idx), K, ptr(partials), ptr(bsum), ptr(bcnt), stream_ptr())


def ema_workspace(K, D):
    """Floats of vq_ema_update's workspace: the per-workgroup partials and the arrival counter."""
    return (K * D + 1023) // 1024 + 1


def vq_ema_update(emb_sum, emb_elem, E, bsum, bcnt, rand_rows, mu, threshold, diag, partials=None, clear=False,
                  sums=(), publish=None, rows=None):
    """partials: workspace of ceil(K*D/1024) + 1 floats, zero-initialised once
    (the last word is an arrival counter each call leaves zero; allocated here
    if None); clear: bsum / bcnt are zero afterwards (vqx_vq_ema_update_clear).
    sums: up to two (parts, scale, out) -- out[0] = scale * sum(parts) in the
    last workgroup; publish: (mailbox, src, dev_copy) -- src published into the
    Mailbox after them; rows: (src, host int32 indices) -- rand_rows read as
    src[indices] inside the launch (rand_rows unused) (vqx_vq_ema_update_close,
    which implies clear).  Returns publish's (seq, slot), else None."""
    K, D = E.shape
    need = ema_workspace(K, D)
    if partials is None:
        partials = torch.zeros(need, device=E.device, dtype=torch.float32)
    if partials.numel() < need:
        raise ValueError(f"vq_ema_update: workspace {partials.numel()} < {need} floats")
    if _debug:
        for t, n, what in ((emb_sum, K * D, "emb_sum"), (emb_elem, K, "emb_elem"), (bsum, K * D, "bsum"),
                           (bcnt, K, "bcnt"), (rand_rows, K * D, "rand_rows"), (diag, 4, "diag")):
            _span(t, n, f"vq_ema_update {what}")
    if not sums and publish is None and rows is None:
        call("vqx_vq_ema_update_clear" if clear else "vqx_vq_ema_update", ptr(emb_sum), ptr(emb_elem), ptr(E), ptr(bsum),
             ptr(bcnt), ptr(rand_rows), K, D, mu, threshold, ptr(diag), ptr(partials), stream_ptr())
        return None
    if not clear or len(sums) > 2:
        raise ValueError("vq_ema_update: sums / publish need clear=True and at most two sums")
    c = L.StepClose()
    for i, (parts, scale, out) in enumerate(sums):
        _check_cuda(parts, out)
        c.parts[i], c.n[i], c.scale[i], c.out[i] = ptr(parts), parts.numel(), float(scale), ptr(out)
    res = None
    if publish is not None:
        mb, src, copy = publish
        _check_cuda(src, copy)
        if src.numel() > mb.floats or not src.is_contiguous() or src.dtype != torch.float32:
            raise ValueError(f"vq_ema_update: publish a contiguous f32 tensor of <= {mb.floats} values")
        seq, slot = res = mb.reserve()
        c.pub_src, c.pub_n, c.pub_copy, c.pub_box = ptr(src), src.numel(), ptr(copy), mb._dev
        c.pub_slot, c.pub_slots, c.pub_floats, c.pub_seq = slot, mb.slots, mb.floats, seq
    if rows is not None:
        src, idx = rows
        _check_cuda(src)
        if idx.dtype != torch.int32 or idx.is_cuda or idx.numel() != K or not idx.is_contiguous() or src.shape[1] != D:
            raise ValueError("vq_ema_update: rows = (src [n, D] device, K host int32 indices)")
        c.rows_src, c.rows_ld, c.n_rows, c.rows_host = ptr(src), src.stride(0), K, idx.data_ptr()
    call("vqx_vq_ema_update_close", ptr(emb_sum), ptr(emb_elem), ptr(E), ptr(bsum), ptr(bcnt), ptr(rand_rows), K, D,
         mu, threshold, ptr(diag), ptr(partials), ctypes.addressof(c), stream_ptr())
    return res


def gather_rows(src, rows, out):
    call("vqx_gather_rows", ptr(src), src.stride(0), ptr(rows), out.shape[0], out.shape[1], ptr(out), stream_ptr())
    return out


def gather_rows_host(src, rows, out):
    """out[i] = src[rows[i]] (zero rows for negative ids) with `rows` a host
    int32 tensor passed to the kernels by value (no copy on the stream)."""
    _check_cuda(src, out)
    if rows.device.type != "cpu" or rows.numel() != out.shape[0]:
        raise ValueError("gather_rows_host: rows must be a host tensor of out.shape[0] ids")
    if not out.is_contiguous() or out.dim() != 2 or out.shape[1] > src.shape[1] or src.stride(1) != 1:
        raise ValueError("gather_rows_host: out must be contiguous [n, D] with D <= src's row width")
    if rows.numel() and (int(rows.max()) >= src.shape[0] or int(rows.min()) < -1):
        raise ValueError(f"gather_rows_host: row ids must lie in [-1, {src.shape[0]})")
    rows = rows.to(torch.int32).contiguous()
    call("vqx_gather_rows_host", ptr(src), src.stride(0), rows.data_ptr(), out.shape[0], out.shape[1], ptr(out),
         stream_ptr())
    return out


def crop_batch(corpus, spk_table, row0, length, utt, x, y):
    """x[b, :, :length[b]] = corpus[row0[b]:row0[b] + length[b]].T, zeros up to
    T; y[b] = spk_table[utt[b]] (vqx_crop_batch).  corpus [n_rows, mel] f32 and
    spk_table [n_utts] int64 are device tensors; row0 (int64), length and utt
    (int32) are host tensors of B entries, passed to the kernel by value (no
    copy on the stream); x (B, mel, T) f32 and y (B,) or (B, 1) int64 are
    written whole.  The library validates every item before it launches."""
    _check_cuda(corpus, spk_table, x, y)
    B = x.shape[0] if x.dim() == 3 else -1
    if (corpus.dim() != 2 or corpus.dtype != torch.float32 or not corpus.is_contiguous() or B < 0
            or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[1] != corpus.shape[1]):
        raise ValueError("crop_batch: corpus [n_rows, mel] and x (B, mel, T) must be contiguous f32 with one mel")
    if spk_table.dtype != torch.int64 or spk_table.dim() != 1 or not spk_table.is_contiguous():
        raise ValueError("crop_batch: spk_table must be a contiguous int64 vector")
    if y.dtype != torch.int64 or y.numel() != B or not y.is_contiguous():
        raise ValueError("crop_batch: y must be contiguous int64 with B elements")
    for t, dt, what in ((row0, torch.int64, "row0"), (length, torch.int32, "length"), (utt, torch.int32, "utt")):
        if t.device.type != "cpu" or t.dtype != dt or t.numel() != B or not t.is_contiguous():
            raise ValueError(f"crop_batch: {what} must be a contiguous host {dt} tensor of B = {B} entries")
    _span(corpus, corpus.numel(), "crop_batch corpus")
    _span(x, x.numel(), "crop_batch x")
    call("vqx_crop_batch", ptr(corpus), corpus.shape[0], corpus.shape[1], ptr(spk_table), spk_table.numel(),
         row0.data_ptr(), length.data_ptr(), utt.data_ptr(), B, x.shape[2], ptr(x), ptr(y), stream_ptr())
    return x, y


def vq_commit_bwd(z, zq, scale, dz):
    call("vqx_vq_commit_bwd", ptr(z), ptr(zq), z.numel(), scale, ptr(dz), dt_code(dz.dtype), stream_ptr())
    return dz


COMMIT_PARTS = 256  # vqx.h VQX_COMMIT_PARTS


def vq_commit_bwd_cs(z, zq, scale, dz, partials):
    """vq_commit_bwd plus partials[p][d] = column sums of the stored dz over row part p
    (COMMIT_PARTS parts; the first level of the bias gradient of the conv producing z)."""
    _check_cuda(z, zq, dz, partials)
    N, D = z.shape
    if tuple(partials.shape) != (COMMIT_PARTS, D) or not partials.is_contiguous() or tuple(dz.shape) != (N, D) \
            or not (z.is_contiguous() and zq.is_contiguous() and dz.is_contiguous()):
        raise ValueError("vq_commit_bwd_cs: contiguous z/zq/dz [N, D] and partials [COMMIT_PARTS, D] expected")
    call("vqx_vq_commit_bwd_cs", ptr(z), ptr(zq), N, D, scale, ptr(dz), dt_code(dz.dtype), ptr(partials),
         stream_ptr())
    return dz


def time_gather(x, y, B, T, src_t):
    call("vqx_time_gather", ptr(x), ptr(y), B, T, x.shape[1], ptr(src_t), dt_code(x.dtype), stream_ptr())
    return y


def embedding_fwd(weight, ids, out):
    call("vqx_embedding_fwd", ptr(weight), ptr(ids), ids.numel(), weight.shape[1], ptr(out), stream_ptr())
    return out


def embedding_bwd(dout, ids, dweight):
    call("vqx_embedding_bwd", ptr(dout), ptr(ids), ids.numel(), dweight.shape[1], ptr(dweight), stream_ptr())
    return dweight


def embedding_bwd_rows(dout, ids, dweight, accumulate=False):
    """Every row of dweight: (+)= the sum of dout's rows whose id is that row, in
    batch order (0 where absent); no zero fill needed before it."""
    _check_cuda(dout, ids, dweight)
    if ids.dtype != torch.int64 or not (dout.is_contiguous() and dweight.is_contiguous()):
        raise ValueError("embedding_bwd_rows: int64 ids, contiguous dout / dweight")
    _span(dout, ids.numel() * dweight.shape[1], "embedding dout")
    _span(ids, ids.numel(), "embedding ids")
    call("vqx_embedding_bwd_rows", ptr(dout), ptr(ids), ids.numel(), dweight.shape[1], dweight.shape[0], ptr(dweight),
         int(accumulate), stream_ptr())
    return dweight


def linear_f32(c, W, bias, out):
    B, I = c.shape
    O = W.shape[0]
    call("vqx_linear_f32", ptr(c), ptr(W), ptr(bias), B, I, O, ptr(out), stream_ptr())
    return out


def linear_bwd_f32(dout, c, W, dW=None, dc=None):
    B, I = c.shape
    O = W.shape[0]
    call("vqx_linear_bwd_f32", ptr(dout), ptr(c), ptr(W), B, I, O, ptr(dW), ptr(dc), stream_ptr())


def grad_sq_norm(g, partials, out):
    call("vqx_grad_sq_norm", ptr(g), g.numel(), ptr(partials), ptr(out), stream_ptr())
    return out


def adam_hyper(step, lr0, gamma, step_size, beta1, beta2, eps, hyper):
    call("vqx_adam_hyper", ptr(step), lr0, gamma, step_size, beta1, beta2, eps, ptr(hyper), stream_ptr())


def adam_step(p, g, m, v, hyper, sumsq, max_norm):
    call("vqx_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), ptr(sumsq), max_norm,
         stream_ptr())


def radam_hyper(step, lr0, gamma, step_size, beta1, beta2, eps, hyper):
    call("vqx_radam_hyper", ptr(step), lr0, gamma, step_size, beta1, beta2, eps, ptr(hyper), stream_ptr())


def adam_step_wn(p, g, m, v, hyper, sumsq, max_norm, rows_table, segs):
    """adam_step plus the next forward's weight-norm preparation of the rows
    in `rows_table` (wn_table of weight-normed convs); `segs` = (host int64
    [n, 2] tensor, its device copy) of the other flat ranges."""
    arr, dev = rows_table
    sh, sd = segs
    call("vqx_adam_step_wn", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), ptr(sumsq), max_norm,
         ctypes.addressof(arr), dev.data_ptr(), len(arr), sh.data_ptr() if sh.numel() else None,
         ptr(sd) if sh.numel() else None, sh.shape[0], stream_ptr())


def radam_step(p, g, m, v, hyper, sumsq, max_norm):
    call("vqx_radam_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), ptr(sumsq), max_norm,
         stream_ptr())


MULTI_MAX_TENSORS = 128  # include/vqx.h VQX_MULTI_MAX_TENSORS: tensors per launch of the multi-tensor kernels
MULTI_CHUNK = 4096       # VQX_MULTI_CHUNK: elements per block and per partial


def multi_layout(numels):
    """(offsets, first partial, number of partials) of tensors packed densely in
    list order: tensor i owns flat elements [offsets[i], offsets[i] + numels[i])
    and the partials [first[i], first[i] + ceil(numels[i] / MULTI_CHUNK))."""
    offsets, first, off, ch = [], [], 0, 0
    for n in numels:
        if n < 0:
            raise ValueError("multi_layout: negative length")
        offsets.append(off)
        first.append(ch)
        off += n
        ch += -(-n // MULTI_CHUNK)
    return offsets, first, ch


class MultiTensorPlan:
    """Host arrays of vqx_multi_sq_norm / vqx_multi_adam_step for a fixed list
    of tensor lengths: numel and offset (dense in list order unless given) are
    filled once, the gradient pointers by set_grads() before each use."""

    def __init__(self, numels, offsets=None):
        numels = [int(n) for n in numels]
        dense, _, self.n_partials = multi_layout(numels)
        offsets = dense if offsets is None else [int(o) for o in offsets]
        if len(offsets) != len(numels):
            raise ValueError("MultiTensorPlan: one offset per tensor")
        self.n = len(numels)
        self.numels, self.offsets = numels, offsets
        self.numel_arr = (ctypes.c_int64 * max(self.n, 1))(*numels)
        self.offset_arr = (ctypes.c_int64 * max(self.n, 1))(*offsets)
        self.grad_arr = (ctypes.c_void_p * max(self.n, 1))()
        chunks = ctypes.c_int64(0)
        call("vqx_multi_chunks", ctypes.addressof(self.numel_arr), self.n, ctypes.byref(chunks))
        if chunks.value != self.n_partials:
            raise RuntimeError(f"multi_layout counts {self.n_partials} partials, the library {chunks.value}")

    def set_grads(self, grads):
        """grads: one contiguous float32 device tensor (or None) per tensor of
        the plan; the caller keeps them alive until the launches have run."""
        if len(grads) != self.n:
            raise ValueError(f"MultiTensorPlan: {len(grads)} gradients for {self.n} tensors")
        arr = self.grad_arr
        for i, g in enumerate(grads):
            if g is None:
                arr[i] = None
                continue
            if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous() or g.numel() != self.numels[i]:
                raise ValueError(f"MultiTensorPlan: gradient {i} must be a contiguous float32 device tensor of "
                                 f"{self.numels[i]} elements")
            arr[i] = g.data_ptr()


def multi_sq_norm(plan, partials):
    """partials[c] = sum g^2 over chunk c of the plan's gradients (zeros for a
    missing gradient); partials has plan.n_partials floats."""
    _check_cuda(partials)
    if partials.numel() != plan.n_partials or partials.dtype != torch.float32 or not partials.is_contiguous():
        raise ValueError(f"multi_sq_norm: partials must be {plan.n_partials} contiguous floats")
    call("vqx_multi_sq_norm", ctypes.addressof(plan.grad_arr), ctypes.addressof(plan.numel_arr), plan.n,
         ptr(partials), plan.n_partials, stream_ptr())
    return partials


def multi_adam_step(p, m, v, plan, hyper, sumsq, max_norm, kind=0):
    """adam_step (kind 0) or radam_step (kind 1) of the flat p, m, v from the
    plan's scattered gradients; a tensor without a gradient is left alone."""
    _check_cuda(p, m, v, hyper)
    if not (p.numel() == m.numel() == v.numel()) or any(t.dtype != torch.float32 or not t.is_contiguous()
                                                        for t in (p, m, v)):
        raise ValueError("multi_adam_step: p, m and v must be contiguous float32 tensors of one length")
    call("vqx_multi_adam_step", ptr(p), ptr(m), ptr(v), p.numel(), ctypes.addressof(plan.offset_arr),
         ctypes.addressof(plan.numel_arr), ctypes.addressof(plan.grad_arr), plan.n, ptr(hyper), ptr(sumsq),
         max_norm, kind, stream_ptr())


def multi_pack(plan, flat):
    """flat[offset_i : offset_i + numel_i] = gradient i of the plan (after
    set_grads()), zeros where the gradient is missing: the one flat buffer a
    collective reduces.  ceil(n / MULTI_MAX_TENSORS) launches."""
    _check_cuda(flat)
    if flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("multi_pack: flat must be a contiguous float32 tensor")
    call("vqx_multi_pack", ptr(flat), flat.numel(), ctypes.addressof(plan.offset_arr),
         ctypes.addressof(plan.numel_arr), ctypes.addressof(plan.grad_arr), plan.n, stream_ptr())
    return flat


def convert_2d(src, dst, rows=None, cols=None):
    """dst[:rows, :cols] = src (dtype-converting, strided); src=None zero-fills."""
    rows = dst.shape[0] if rows is None else rows
    cols = dst.shape[1] if cols is None else cols
    call("vqx_convert_2d", ptr(src), src.stride(0) if src is not None else 0,
         dt_code(src.dtype) if src is not None else 0, ptr(dst), dst.stride(0), dt_code(dst.dtype), rows, cols,
         stream_ptr())
    return dst


def convert_2d_zero2(src, dst, zero_dst):
    """dst = src (dtype-converting, strided) and zero_dst = 0 (dst's dtype), one launch."""
    _check_cuda(src, dst, zero_dst)
    if tuple(src.shape) != tuple(dst.shape) or zero_dst.dtype != dst.dtype or zero_dst.dim() != 2:
        raise ValueError("convert_2d_zero2: src and dst must share a shape, zero_dst dst's dtype")
    call("vqx_convert_2d_zero2", ptr(src), src.stride(0), dt_code(src.dtype), ptr(dst), dst.stride(0),
         dt_code(dst.dtype), dst.shape[0], dst.shape[1], ptr(zero_dst), zero_dst.stride(0), zero_dst.shape[0],
         zero_dst.shape[1], stream_ptr())
    return dst


def zero_(t):
    """Zero a contiguous f32/bf16 device tensor with the native fill."""
    flat = t.view(1, -1)
    return convert_2d(None, flat)


def scale_act_2d(src, dst, scale, act, rows=None, cols=None):
    """dst = act(scale * src) (strided, dtype-converting)."""
    rows = dst.shape[0] if rows is None else rows
    cols = dst.shape[1] if cols is None else cols
    call("vqx_scale_act_2d", ptr(src), src.stride(0), dt_code(src.dtype), ptr(dst), dst.stride(0), dt_code(dst.dtype),
         rows, cols, scale, act, stream_ptr())
    return dst


def vq_normalize(z, E, z_norm, z_len, emb_norm, e_len, partials, normloss_out=None):
    """embed_norm() in place on E, emb_norm = E/||E||, z_norm = z/||z|| (+ sum (z_norm - z)^2)."""
    call("vqx_vq_normalize", ptr(z), z.shape[0], z.shape[1], ptr(E), E.shape[0], ptr(z_norm), ptr(z_len),
         ptr(emb_norm), ptr(e_len), ptr(partials), ptr(normloss_out), stream_ptr())


def vq_perplexity(counts, n_rows, out):
    call("vqx_vq_perplexity", ptr(counts), counts.shape[0], n_rows, ptr(out), stream_ptr())


def vq_plain_bwd(z, z_norm, z_len, zq, dzq, src_t, T, normalize, beta, scale, dz, bsum, bcnt, emb, e_len, dE):
    call("vqx_vq_plain_bwd", ptr(z), ptr(z_norm), ptr(z_len), ptr(zq), ptr(dzq), ptr(src_t), T, zq.shape[0],
         zq.shape[1], int(normalize), beta, scale, ptr(dz), dt_code(dz.dtype), ptr(bsum), ptr(bcnt), ptr(emb),
         ptr(e_len), emb.shape[0], ptr(dE), stream_ptr())


def vq_plain_bwd_g(z, z_norm, z_len, zq, dzq, T, normalize, s_qut, s_enc, g_qut, g_enc, dz, bsum, bcnt, emb, e_len,
                   dE):
    """vq_plain_bwd with the weights of z_qut / z_enc given apart (s_qut = scale,
    s_enc = beta * scale) and their upstream gradients as device scalars (f32,
    one element each; None = 1): no readback (vqx_vq_plain_bwd_g)."""
    _check_cuda(z_norm, zq, dz, bsum, bcnt, emb, dE)
    for g in (g_qut, g_enc):
        if g is not None and (not g.is_cuda or g.dtype != torch.float32 or g.numel() != 1):
            raise ValueError("vq_plain_bwd_g: an upstream gradient must be a one-element f32 device tensor")
    call("vqx_vq_plain_bwd_g", ptr(z), ptr(z_norm), ptr(z_len), ptr(zq), ptr(dzq), T, zq.shape[0], zq.shape[1],
         int(normalize), s_qut, s_enc, ptr(g_qut), ptr(g_enc), ptr(dz), dt_code(dz.dtype), ptr(bsum), ptr(bcnt),
         ptr(emb), ptr(e_len), emb.shape[0], ptr(dE), stream_ptr())


GST_PARAMS = ("gst_embs", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo")  # vqx_gst_args order


def gst_workspace(B, N, F, H, R, E):
    """Floats of the workspace one gst_fwd + gst_bwd pair shares (vqx_gst_workspace)."""
    out = ctypes.c_int64()
    call("vqx_gst_workspace", int(B), int(N), int(F), int(H), int(R), int(E), ctypes.byref(out))
    return out.value


def _gst_args(z, T, params, heads, ws, what):
    """The parts of vqx_gst_args both directions share.  z: f32 [B*T, >= R] rows
    (stride(0) = ldz); params: the nine f32 tensors in GST_PARAMS order."""
    _check_cuda(z, ws, *params)
    emb, wq, bq, wk, bk, wv, bv, wo, bo = params
    for t in (z, ws, *params):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: f32 tensors only")
    if z.dim() != 2 or z.stride(1) != 1 or z.shape[0] % T or not all(p.is_contiguous() for p in params):
        raise ValueError(f"{what}: z must be [B*T, R] rows with unit column stride, the parameters contiguous")
    (N, E), (F, R) = emb.shape, wq.shape
    if tuple(wk.shape) != (F, E) or tuple(wv.shape) != (F, E) or tuple(wo.shape) != (F, F) \
            or any(tuple(b.shape) != (F,) for b in (bq, bk, bv, bo)) or z.shape[1] != R:
        raise ValueError(f"{what}: parameter shapes do not fit gst_embs {tuple(emb.shape)} / wq {tuple(wq.shape)}")
    a = L.GstArgs()
    a.z, a.ws = ptr(z), ptr(ws)
    for name, p in zip(GST_PARAMS, params):
        setattr(a, name, ptr(p))
    a.B, a.T, a.R, a.N, a.E, a.F, a.H, a.ldz = z.shape[0] // T, T, R, N, E, F, heads, z.stride(0)
    need = gst_workspace(a.B, N, F, heads, R, E)
    if ws.numel() < need or not ws.is_contiguous():
        raise ValueError(f"{what}: workspace {ws.numel()} < {need} floats")
    _rows(z, z.shape[0], a.ldz, R, f"{what} z")
    return a


def gst_fwd(z, T, params, heads, style, ws):
    """style [B, F] = the style-token layer of mean_t z (vqx_gst_fwd, 2 launches);
    `ws` (gst_workspace floats) keeps what gst_bwd reads."""
    a = _gst_args(z, T, params, heads, ws, "gst_fwd")
    _check_cuda(style)
    if tuple(style.shape) != (a.B, a.F) or not style.is_contiguous() or style.dtype != torch.float32:
        raise ValueError(f"gst_fwd: style must be a contiguous f32 [{a.B}, {a.F}]")
    a.style = ptr(style)
    call("vqx_gst_fwd", ctypes.byref(a), stream_ptr())
    return style


def gst_bwd(z, T, params, heads, d_style, ws, dz, grads):
    """From d_style [B, F] and the `ws` gst_fwd filled (vqx_gst_bwd, 3 launches):
    dz [B*T, >= R] rows and `grads`, nine tensors shaped like `params`; all overwritten."""
    a = _gst_args(z, T, params, heads, ws, "gst_bwd")
    _check_cuda(d_style, dz, *grads)
    if tuple(d_style.shape) != (a.B, a.F) or not d_style.is_contiguous() or d_style.dtype != torch.float32:
        raise ValueError(f"gst_bwd: d_style must be a contiguous f32 [{a.B}, {a.F}]")
    if dz.dim() != 2 or dz.shape[0] != z.shape[0] or dz.shape[1] != a.R or dz.stride(1) != 1 \
            or dz.dtype != torch.float32:
        raise ValueError(f"gst_bwd: dz must be f32 [{z.shape[0]}, {a.R}] rows with unit column stride")
    if len(grads) != len(params) or any(g.shape != p.shape or not g.is_contiguous() or g.dtype != torch.float32
                                        for g, p in zip(grads, params)):
        raise ValueError("gst_bwd: grads must be contiguous f32 tensors shaped like the parameters")
    a.d_style, a.dz, a.lddz = ptr(d_style), ptr(dz), dz.stride(0)
    for name, g in zip(GST_PARAMS, grads):
        setattr(a, "d_gst_embs" if name == "gst_embs" else "d" + name, ptr(g))
    _rows(dz, dz.shape[0], a.lddz, a.R, "gst_bwd dz")
    call("vqx_gst_bwd", ctypes.byref(a), stream_ptr())
    return dz


def attn_workspace(B, T, F, H, dtype):
    """Floats of attn_bwd's workspace (vqx_attn_workspace); raises for a shape the kernels refuse."""
    out = ctypes.c_int64()
    call("vqx_attn_workspace", int(B), int(T), int(F), int(H), dt_code(dtype), ctypes.byref(out))
    return out.value


def _attn_args(qkv, ctx, lse, B, T, H, lengths, what):
    """vqx_attn_args of both directions.  qkv [B*T, >= 3F] rows (q | k | v) and
    ctx [B*T, >= F] rows of one compute dtype with unit column stride, lse f32
    of B*H*T entries; lengths: None or what len_array takes (host values)."""
    arr = None if lengths is None else len_array(lengths, B, f"{what} lengths")  # before any device work
    _check_cuda(qkv, ctx, lse)
    if qkv.dim() != 2 or ctx.dim() != 2 or qkv.stride(1) != 1 or ctx.stride(1) != 1 or qkv.dtype != ctx.dtype \
            or qkv.shape[0] != B * T or ctx.shape[0] != B * T or qkv.shape[1] % 3:
        raise ValueError(f"{what}: qkv must be [{B * T}, 3F] rows and ctx [{B * T}, F] rows of one dtype")
    F = qkv.shape[1] // 3
    if ctx.shape[1] != F or lse.dtype != torch.float32 or lse.numel() < B * H * T or not lse.is_contiguous():
        raise ValueError(f"{what}: ctx must have F = {F} columns, lse {B * H * T} contiguous f32 entries")
    a = L.AttnArgs()
    a.qkv, a.ctx, a.lse = ptr(qkv), ptr(ctx), ptr(lse)
    a.len = ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None  # the caller keeps arr alive over the call
    a.B, a.T, a.F, a.H, a.ldqkv, a.ldc, a.dtype = B, T, F, H, qkv.stride(0), ctx.stride(0), dt_code(qkv.dtype)
    _rows(qkv, B * T, a.ldqkv, 3 * F, f"{what} qkv")
    _rows(ctx, B * T, a.ldc, F, f"{what} ctx")
    return a, arr


def attn_fwd(qkv, ctx, lse, B, T, H, lengths=None):
    """ctx = softmax(q k^T / sqrt(d_k)) v per head over the keys t2 < lengths[b],
    lse its log-sum-exp (vqx_attn_fwd, 1 launch); ctx rows t >= lengths[b] are zeros."""
    a, arr = _attn_args(qkv, ctx, lse, B, T, H, lengths, "attn_fwd")
    call("vqx_attn_fwd", ctypes.byref(a), stream_ptr())
    return ctx


def attn_bwd(qkv, ctx, lse, d_ctx, d_qkv, ws, B, T, H, lengths=None):
    """d_qkv (overwritten) from d_ctx and what attn_fwd left (vqx_attn_bwd, 3
    launches, no atomics); rows t >= lengths[b] of d_ctx are not read and those
    of d_qkv are zeros.  ws: attn_workspace floats."""
    a, arr = _attn_args(qkv, ctx, lse, B, T, H, lengths, "attn_bwd")
    _check_cuda(d_ctx, d_qkv, ws)
    if d_ctx.shape != ctx.shape or d_ctx.stride() != ctx.stride() or d_ctx.dtype != ctx.dtype \
            or d_qkv.shape != qkv.shape or d_qkv.stride() != qkv.stride() or d_qkv.dtype != qkv.dtype:
        raise ValueError("attn_bwd: d_ctx and d_qkv must have the shape, strides and dtype of ctx and qkv")
    need = attn_workspace(B, T, a.F, H, qkv.dtype)
    if ws.dtype != torch.float32 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError(f"attn_bwd: workspace {ws.numel()} < {need} floats")
    a.d_ctx, a.d_qkv, a.ws = ptr(d_ctx), ptr(d_qkv), ptr(ws)
    call("vqx_attn_bwd", ctypes.byref(a), stream_ptr())
    return d_qkv


HIER_MAX_LEVELS = 8  # include/vqx.h vqx_upsample_cat_*


def _hier_levels(levels, B, what, dtype=torch.float32):
    """vqx_hier_level array of frame-major levels [B*T_l, C_l] of `dtype` (rows of stride(0))."""
    if not 1 <= len(levels) <= HIER_MAX_LEVELS:
        raise ValueError(f"{what}: {len(levels)} levels, 1..{HIER_MAX_LEVELS} are supported")
    _check_cuda(*levels)
    arr = (L.HierLevel * len(levels))()
    for e, z in zip(arr, levels):
        if z.dtype != dtype or z.dim() != 2 or z.stride(1) != 1 or z.shape[0] % B:
            raise ValueError(f"{what}: a level must be {dtype} [B*T_l, C_l] rows with unit column stride")
        e.z, e.T_l, e.C, e.ld = ptr(z), z.shape[0] // B, z.shape[1], z.stride(0)
        _rows(z, z.shape[0], e.ld, e.C, f"{what} level")
    return arr


def upsample_cat_fwd(levels, B, T, out):
    """out[b*T + t, off_l + c] = levels[l][b*T_l + min(t // (T // T_l), T_l - 1), c]
    (vqx_upsample_cat_fwd): the levels stretched to T frames by repetition and
    stacked on channels; out f32 or bf16 [B*T, >= sum C_l]."""
    arr = _hier_levels(levels, B, "upsample_cat_fwd")
    _check_cuda(out)
    if out.dim() != 2 or out.shape[0] != B * T or out.stride(1) != 1:
        raise ValueError(f"upsample_cat_fwd: out must be [{B * T}, C] rows with unit column stride")
    _rows(out, out.shape[0], out.stride(0), sum(z.shape[1] for z in levels), "upsample_cat_fwd out")
    call("vqx_upsample_cat_fwd", arr, len(levels), B, T, ptr(out), out.stride(0), dt_code(out.dtype), stream_ptr())
    return out


def upsample_cat_bwd(dlevels, B, T, dout):
    """The adjoint: dlevels[l][b*T_l + s, c] = the sum of dout[b*T + t, off_l + c]
    over the frames t stretched from s, in fp32 in a fixed order (overwritten;
    vqx_upsample_cat_bwd).  With one level of dout's width: per-segment column sums."""
    arr = _hier_levels(dlevels, B, "upsample_cat_bwd")
    _check_cuda(dout)
    if dout.dim() != 2 or dout.shape[0] != B * T or dout.stride(1) != 1:
        raise ValueError(f"upsample_cat_bwd: dout must be [{B * T}, C] rows with unit column stride")
    _rows(dout, dout.shape[0], dout.stride(0), sum(z.shape[1] for z in dlevels), "upsample_cat_bwd dout")
    call("vqx_upsample_cat_bwd", arr, len(dlevels), B, T, ptr(dout), dout.stride(0), dt_code(dout.dtype), stream_ptr())
    return dlevels


def upsample_cat_bwd_to(dlevels, B, T, dout):
    """upsample_cat_bwd with the levels stored in their own dtype (all f32 or
    all bf16; vqx_upsample_cat_bwd_to): the same fp32 sums in the same order,
    rounded once to nearest even for bf16 levels."""
    if not dlevels or any(z.dtype != dlevels[0].dtype for z in dlevels):
        raise ValueError("upsample_cat_bwd_to: the levels must share one dtype")
    arr = _hier_levels(dlevels, B, "upsample_cat_bwd_to", dlevels[0].dtype)
    _check_cuda(dout)
    if dout.dim() != 2 or dout.shape[0] != B * T or dout.stride(1) != 1:
        raise ValueError(f"upsample_cat_bwd_to: dout must be [{B * T}, C] rows with unit column stride")
    _rows(dout, dout.shape[0], dout.stride(0), sum(z.shape[1] for z in dlevels), "upsample_cat_bwd_to dout")
    call("vqx_upsample_cat_bwd_to", arr, len(dlevels), B, T, ptr(dout), dout.stride(0), dt_code(dout.dtype),
         dt_code(dlevels[0].dtype), stream_ptr())
    return dlevels


def _codes_levels(levels, B, what):
    """vqx_codes_level array of dense levels / (idx, codebook, normalize) tuples; returns (array, sum of C_l)."""
    if not 1 <= len(levels) <= HIER_MAX_LEVELS:
        raise ValueError(f"{what}: {len(levels)} levels, 1..{HIER_MAX_LEVELS} are supported")
    arr, total = (L.CodesLevel * len(levels))(), 0
    for e, lv in zip(arr, levels):
        if torch.is_tensor(lv):
            z = lv
            _check_cuda(z)
            if z.dtype != torch.float32 or z.dim() != 2 or z.stride(1) != 1 or z.shape[0] % B:
                raise ValueError(f"{what}: a dense level must be f32 [B*T_l, C_l] rows with unit column "
                                 "stride")
            e.z, e.idx, e.T_l, e.C, e.ld = ptr(z), None, z.shape[0] // B, z.shape[1], z.stride(0)
            _rows(z, z.shape[0], e.ld, e.C, f"{what} level")
        else:
            idx, E, normalize = lv
            _check_cuda(idx, E)
            if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != B or not idx.is_contiguous():
                raise ValueError(f"{what}: indices must be a contiguous int64 ({B}, T_l) tensor")
            if E.dtype != torch.float32 or E.dim() != 2 or E.stride(1) != 1:
                raise ValueError(f"{what}: a codebook must be f32 [K, D] rows with unit column stride")
            e.z, e.idx, e.T_l, e.C, e.ld = ptr(E), ptr(idx), idx.shape[1], E.shape[1], E.stride(0)
            e.K, e.normalize = E.shape[0], int(bool(normalize))
            _span(idx, idx.numel(), f"{what} idx")
            _rows(E, e.K, e.ld, e.C, f"{what} codebook")
        total += e.C
    return arr, total


def codes_upsample_cat(levels, B, T, out):
    """The first decoder's frame-major input from codes in one launch
    (vqx_codes_upsample_cat).  A level is a dense f32 tensor [B*T_l, C_l] (as in
    upsample_cat_fwd) or a tuple (idx int64 (B, T_l), codebook f32 [K, D],
    normalize): out[b*T + t, off_l + c] = codebook[idx[b, src_l(t)], c], divided
    by the row's L2 norm with `normalize`.  out f32 or bf16 [B*T, >= sum C_l].
    The indices are not checked here (the caller's job, Model.synthesize)."""
    arr, total = _codes_levels(levels, B, "codes_upsample_cat")
    _check_cuda(out)
    if out.dim() != 2 or out.shape[0] != B * T or out.stride(1) != 1:
        raise ValueError(f"codes_upsample_cat: out must be [{B * T}, C] rows with unit column stride")
    _rows(out, out.shape[0], out.stride(0), total, "codes_upsample_cat out")
    call("vqx_codes_upsample_cat", arr, len(levels), B, T, ptr(out), out.stride(0), dt_code(out.dtype), stream_ptr())
    return out


# ---- a batch of different lengths (vqx_varlen.hip): `lengths` are host values
def len_array(lengths, B=None, what="lengths"):
    """Per-utterance lengths as the host int32 array the *_len entry points take:
    a sequence of ints or a CPU integer tensor (a device tensor is refused: it
    would cost a read-back), or an array this function returned, passed through."""
    if isinstance(lengths, ctypes.Array):
        arr = lengths
    else:
        if torch.is_tensor(lengths):
            if lengths.is_cuda or lengths.is_floating_point() or lengths.dim() != 1:
                raise ValueError(f"{what} must be host values: a sequence of ints or a 1-D CPU integer tensor, never a "
                                 "device tensor")
            lengths = lengths.tolist()
        vals = list(lengths)
        if not vals or any(isinstance(v, bool) or not isinstance(v, int) for v in vals):
            raise ValueError(f"{what} must be a non-empty sequence of ints")
        if any(not -2 ** 31 <= v < 2 ** 31 for v in vals):
            raise ValueError(f"{what} must fit 32 bits")
        arr = (ctypes.c_int32 * len(vals))(*vals)
    if B is not None and len(arr) != B:
        raise ValueError(f"{what}: {len(arr)} entries for a batch of {B}")
    return arr


def _len_rows(t, T, lengths, what):
    """Checks shared by the *_len ops on rows t [B*T, C]: returns the host array of B lengths."""
    _check_cuda(t)
    if t.dim() != 2 or t.stride(1) != 1 or T < 1 or t.shape[0] % T or t.shape[0] < T:
        raise ValueError(f"{what}: rows must be [B*T, C] with unit column stride, T = {T}")
    return len_array(lengths, t.shape[0] // T, f"{what} lengths")


def groupnorm_stats_len(x, T, G, lengths, partials, mean_rstd, eps=1e-5):
    """groupnorm_stats over rows t < lengths[b] of every utterance (vqx_groupnorm_stats_len)."""
    arr = _len_rows(x, T, lengths, "groupnorm_stats_len")
    B = len(arr)
    _check_cuda(partials, mean_rstd)
    if partials.numel() < B * G * 24 or mean_rstd.numel() < B * G * 2 or partials.dtype != torch.float32 \
            or mean_rstd.dtype != torch.float32:
        raise ValueError(f"groupnorm_stats_len: partials needs {B * G * 24} floats, mean_rstd {B * G * 2}")
    _rows(x, x.shape[0], x.stride(0), x.shape[1], "groupnorm_stats_len x")
    call("vqx_groupnorm_stats_len", ptr(x), x.stride(0), dt_code(x.dtype), x.shape[0], T, x.shape[1], G, arr, eps,
         ptr(partials), ptr(mean_rstd), stream_ptr())
    return mean_rstd


def _gn_len_apply(name, h, g, T, cols, lengths, mean_rstd, gamma, beta, G):
    arr = _len_rows(h, T, lengths, name)
    _check_cuda(g, mean_rstd, gamma, beta)
    if g.dim() != 2 or g.shape[0] != h.shape[0] or g.shape[1] < cols or g.stride(1) != 1 or g.dtype != h.dtype:
        raise ValueError(f"{name}: the output must be [{h.shape[0]}, >= {cols}] rows of the input's dtype")
    if any(t.dtype != torch.float32 for t in (mean_rstd, gamma, beta)) or mean_rstd.numel() < len(arr) * G * 2 \
            or gamma.numel() < h.shape[1] or beta.numel() < h.shape[1]:
        raise ValueError(f"{name}: mean_rstd [B, {G}, 2], gamma and beta [C] must be f32")
    _rows(h, h.shape[0], h.stride(0), h.shape[1], f"{name} in")
    _rows(g, g.shape[0], g.stride(0), cols, f"{name} out")
    call("vqx_" + name, ptr(h), h.stride(0), ptr(g), g.stride(0), dt_code(h.dtype), h.shape[0], T, h.shape[1], arr,
         ptr(mean_rstd), ptr(gamma), ptr(beta), stream_ptr())
    return g


def gn_lrelu_fwd_len(h, g, T, lengths, mean_rstd, gamma, beta):
    """gn_lrelu_fwd on rows t < lengths[b]; rows from lengths[b] up are written as zeros (vqx_gn_lrelu_fwd_len)."""
    return _gn_len_apply("gn_lrelu_fwd_len", h, g, T, h.shape[1], lengths, mean_rstd, gamma, beta, 1)


def gn_glu_fwd_len(u, g, T, lengths, mean_rstd, gamma, beta):
    """gn_glu_fwd on rows t < lengths[b]; rows from lengths[b] up are written as zeros (vqx_gn_glu_fwd_len)."""
    return _gn_len_apply("gn_glu_fwd_len", u, g, T, u.shape[1] // 2, lengths, mean_rstd, gamma, beta, 2)


def mask_tail(x, T, lengths):
    """x[b*T + t, :] = 0 for lengths[b] <= t < T, in place (vqx_mask_tail)."""
    arr = _len_rows(x, T, lengths, "mask_tail")
    _rows(x, x.shape[0], x.stride(0), x.shape[1], "mask_tail x")
    call("vqx_mask_tail", ptr(x), x.stride(0), dt_code(x.dtype), x.shape[0], T, x.shape[1], arr, stream_ptr())
    return x


def nct_to_ntc_len(x_nct, lengths, y):
    """y[b*T + t, c] = x_nct[b, c, t] for t < lengths[b], else 0 (vqx_nct_to_ntc_len):
    nct_to_ntc and mask_tail in one pass; x_nct is not read from lengths[b] up."""
    _check_cuda(x_nct, y)
    if x_nct.dim() != 3 or x_nct.dtype != torch.float32 or not x_nct.is_contiguous():
        raise ValueError("nct_to_ntc_len: x must be a contiguous f32 (B, C, T) tensor")
    B, C, T = x_nct.shape
    arr = len_array(lengths, B, "nct_to_ntc_len lengths")
    if y.dim() != 2 or y.shape[0] != B * T or y.shape[1] < C or y.stride(1) != 1:
        raise ValueError(f"nct_to_ntc_len: y must be [{B * T}, >= {C}] rows with unit column stride")
    _rows(y, B * T, y.stride(0), C, "nct_to_ntc_len y")
    call("vqx_nct_to_ntc_len", ptr(x_nct), B, C, T, arr, ptr(y), y.stride(0), dt_code(y.dtype), stream_ptr())
    return y


def ntc_to_nct_len(y, T, lengths, x_nct):
    """x_nct[b, c, t] = y[b*T + t, c] for t < lengths[b], else 0, over t < T_out = x_nct.shape[2] <= T
    (vqx_ntc_to_nct_len): mask_tail and ntc_to_nct in one pass; the rows of y from lengths[b] up are not read."""
    arr = _len_rows(y, T, lengths, "ntc_to_nct_len")
    _check_cuda(x_nct)
    B = len(arr)
    if x_nct.dim() != 3 or x_nct.dtype != torch.float32 or not x_nct.is_contiguous() or x_nct.shape[0] != B \
            or x_nct.shape[1] > y.shape[1] or not 1 <= x_nct.shape[2] <= T:
        raise ValueError(f"ntc_to_nct_len: x must be a contiguous f32 ({B}, C <= {y.shape[1]}, T_out <= {T}) tensor")
    C, T_out = x_nct.shape[1], x_nct.shape[2]
    _rows(y, B * T, y.stride(0), C, "ntc_to_nct_len y")
    call("vqx_ntc_to_nct_len", ptr(y), y.stride(0), dt_code(y.dtype), B, C, T, arr, ptr(x_nct), T_out, stream_ptr())
    return x_nct


def nct_to_ntc_pad_len(x_nct, T, lengths, y):
    """y[b*T + t, c] = x_nct[b, c, t] for t < lengths[b] <= T_in, else 0, over t < T >= T_in = x_nct.shape[2]
    (vqx_nct_to_ntc_pad_len): nct_to_ntc_len into more rows an utterance than x has frames; x_nct is not read from
    lengths[b] up.  Shapes and dtypes are checked before the device (ValueError)."""
    if x_nct.dim() != 3 or x_nct.dtype != torch.float32 or not x_nct.is_contiguous():
        raise ValueError("nct_to_ntc_pad_len: x must be a contiguous f32 (B, C, T_in) tensor")
    B, C, T_in = x_nct.shape
    if isinstance(T, bool) or not isinstance(T, int) or T < T_in:
        raise ValueError(f"nct_to_ntc_pad_len: T = {T!r} rows an utterance must be an int >= x's {T_in} frames")
    arr = len_array(lengths, B, "nct_to_ntc_pad_len lengths")
    if y.dim() != 2 or y.shape[0] != B * T or y.shape[1] < C or y.stride(1) != 1 \
            or y.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"nct_to_ntc_pad_len: y must be f32 or bf16 [{B * T}, >= {C}] rows with unit column stride")
    _check_cuda(x_nct, y)
    _rows(y, B * T, y.stride(0), C, "nct_to_ntc_pad_len y")
    call("vqx_nct_to_ntc_pad_len", ptr(x_nct), B, C, T_in, T, arr, ptr(y), y.stride(0), dt_code(y.dtype), stream_ptr())
    return y


def index_mask_len(idx, lengths, out):
    """out[b, t] = idx[b, t] for t < lengths[b], else 0, over t < T_out = out.shape[1] <= idx.shape[1]
    (vqx_index_mask_len), both int64: the codes of a padded batch with zeros at the padded positions; idx is not read
    from lengths[b] up.  Shapes and dtypes are checked before the device (ValueError)."""
    if idx.dim() != 2 or idx.dtype != torch.int64 or not idx.is_contiguous():
        raise ValueError("index_mask_len: idx must be a contiguous int64 (B, T) tensor")
    B, T = idx.shape
    if out.dim() != 2 or out.dtype != torch.int64 or not out.is_contiguous() or out.shape[0] != B \
            or not 1 <= out.shape[1] <= T:
        raise ValueError(f"index_mask_len: out must be a contiguous int64 ({B}, T_out <= {T}) tensor")
    arr = len_array(lengths, B, "index_mask_len lengths")
    _check_cuda(idx, out)
    _span(idx, idx.numel(), "index_mask_len idx")
    _span(out, out.numel(), "index_mask_len out")
    call("vqx_index_mask_len", ptr(idx), B, T, arr, ptr(out), out.shape[1], stream_ptr())
    return out


def codes_upsample_cat_len(levels, B, T, lengths, level_lengths, out):
    """codes_upsample_cat for a padded batch (vqx_codes_upsample_cat_len): utterance
    b has lengths[b] <= T output frames and level_lengths[l][b] frames at level
    l (stored with the level's own padded T_l); its rows from lengths[b] up are
    zeros.  Levels as in codes_upsample_cat."""
    arr, total = _codes_levels(levels, B, "codes_upsample_cat_len")
    n_arr = len_array(lengths, B, "codes_upsample_cat_len lengths")
    if len(level_lengths) != len(levels):
        raise ValueError(f"codes_upsample_cat_len: {len(level_lengths)} length lists for {len(levels)} levels")
    per_level = [len_array(m, B, f"codes_upsample_cat_len level {l} lengths") for l, m in enumerate(level_lengths)]
    m_arr = (ctypes.c_int32 * (B * len(levels)))(*[per_level[l][b] for b in range(B) for l in range(len(levels))])
    _check_cuda(out)
    if out.dim() != 2 or out.shape[0] != B * T or out.stride(1) != 1:
        raise ValueError(f"codes_upsample_cat_len: out must be [{B * T}, C] rows with unit column stride")
    _rows(out, out.shape[0], out.stride(0), total, "codes_upsample_cat_len out")
    call("vqx_codes_upsample_cat_len", arr, len(levels), B, T, n_arr, m_arr, ptr(out), out.stride(0),
         dt_code(out.dtype), stream_ptr())
    return out


def segment_mean(z, T, lengths, out):
    """out[b, c] = mean over t < lengths[b] of z[b*T + t, c], f32 (vqx_segment_mean)."""
    arr = _len_rows(z, T, lengths, "segment_mean")
    _check_cuda(out)
    if z.dtype != torch.float32 or out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 \
            or tuple(out.shape) != (len(arr), z.shape[1]):
        raise ValueError(f"segment_mean: z must be f32 rows and out f32 [{len(arr)}, {z.shape[1]}]")
    _rows(z, z.shape[0], z.stride(0), z.shape[1], "segment_mean z")
    call("vqx_segment_mean", ptr(z), z.stride(0), z.shape[0], T, z.shape[1], arr, ptr(out), out.stride(0),
         stream_ptr())
    return out


def nct_to_ntc_lrelu_bwd(g_nct, a, slope, dst):
    """dst[b*T + t, c] = g_nct[b, c, t] * (a[b*T + t, c] > 0 ? 1 : slope)
    (vqx_nct_to_ntc_lrelu_bwd): the f32 (B, C, T) gradient into a LeakyReLU's
    output, through it, as frame-major rows in dst's dtype; a, dst [B*T, >= C]."""
    _check_cuda(g_nct, a, dst)
    B, C, T = g_nct.shape
    if g_nct.dtype != torch.float32 or not g_nct.is_contiguous():
        raise ValueError("nct_to_ntc_lrelu_bwd: g must be a contiguous f32 (B, C, T) tensor")
    for t, what in ((a, "a"), (dst, "dst")):
        if t.dim() != 2 or t.shape[0] != B * T or t.shape[1] < C or t.stride(1) != 1:
            raise ValueError(f"nct_to_ntc_lrelu_bwd: {what} must be [{B * T}, >= {C}] rows with unit column stride")
        _rows(t, B * T, t.stride(0), C, f"nct_to_ntc_lrelu_bwd {what}")
    call("vqx_nct_to_ntc_lrelu_bwd", ptr(g_nct), B, C, T, ptr(a), a.stride(0), dt_code(a.dtype), slope, ptr(dst),
         dst.stride(0), dt_code(dst.dtype), stream_ptr())
    return dst


def ntc_to_nct_scale(y, g, x_nct):
    """x_nct[b, c, t] = y[b*T + t, c] * g[0] (vqx_ntc_to_nct_scale): f32 rows to (B, C, T)
    times a one-element f32 device tensor."""
    _check_cuda(y, g, x_nct)
    B, C, T = x_nct.shape
    if y.dtype != torch.float32 or g.dtype != torch.float32 or x_nct.dtype != torch.float32 or g.numel() != 1 \
            or not x_nct.is_contiguous() or y.dim() != 2 or y.shape[0] != B * T or y.shape[1] < C or y.stride(1) != 1:
        raise ValueError(f"ntc_to_nct_scale: f32 y [{B * T}, >= {C}] rows, a one-element f32 g, contiguous f32 x")
    _rows(y, B * T, y.stride(0), C, "ntc_to_nct_scale y")
    call("vqx_ntc_to_nct_scale", ptr(y), y.stride(0), B, C, T, ptr(g), ptr(x_nct), stream_ptr())
    return x_nct


def _src_map(src_t, T, what):
    if src_t is not None and (not src_t.is_cuda or src_t.dtype != torch.int32 or src_t.numel() != T
                              or not src_t.is_contiguous()):
        raise ValueError(f"{what}: src_t must be a contiguous device int32 tensor of T = {T} entries")


def ntc_to_nct_gather(y, src_t, x_nct):
    """x_nct[b, c, t] = y[b*T + src_t[t], c] (vqx_ntc_to_nct_gather): f32 / bf16 rows
    to f32 (B, C, T) with the jitter's neighbour map (device int32 [T]; None:
    the plain transposition) folded in."""
    _check_cuda(y, x_nct)
    B, C, T = x_nct.shape
    if x_nct.dtype != torch.float32 or not x_nct.is_contiguous() or y.dim() != 2 or y.shape[0] != B * T \
            or y.shape[1] < C or y.stride(1) != 1:
        raise ValueError(f"ntc_to_nct_gather: y [{B * T}, >= {C}] rows, contiguous f32 x")
    _src_map(src_t, T, "ntc_to_nct_gather")
    _rows(y, B * T, y.stride(0), C, "ntc_to_nct_gather y")
    call("vqx_ntc_to_nct_gather", ptr(y), y.stride(0), dt_code(y.dtype), B, C, T, ptr(src_t), ptr(x_nct), stream_ptr())
    return x_nct


def nct_to_ntc_keep(g_nct, src_t, y):
    """y[b*T + t, c] = g_nct[b, c, t] where src_t[t] == t, else 0 (vqx_nct_to_ntc_keep):
    the jitter's backward folded into the layout change; y f32 / bf16 rows."""
    _check_cuda(g_nct, y)
    B, C, T = g_nct.shape
    if g_nct.dtype != torch.float32 or not g_nct.is_contiguous() or y.dim() != 2 or y.shape[0] != B * T \
            or y.shape[1] < C or y.stride(1) != 1:
        raise ValueError(f"nct_to_ntc_keep: contiguous f32 g (B, C, T), y [{B * T}, >= {C}] rows")
    _src_map(src_t, T, "nct_to_ntc_keep")
    _rows(y, B * T, y.stride(0), C, "nct_to_ntc_keep y")
    call("vqx_nct_to_ntc_keep", ptr(g_nct), B, C, T, ptr(src_t), ptr(y), y.stride(0), dt_code(y.dtype), stream_ptr())
    return y


def vq_commit_bwd_g(z, zq, B, T, s, g, dz):
    """dz = (s * g[0]) * (z - zq) (vqx_vq_commit_bwd_g) from contiguous f32 rows
    z, zq [B*T, D]; dz f32 (B, D, T) or [B*T, D] rows (told by its shape); g a
    one-element f32 device tensor or None (= 1): no readback."""
    _check_cuda(z, zq, dz, g)
    D = z.shape[1]
    nct = dz.dim() == 3
    if tuple(z.shape) != (B * T, D) or zq.shape != z.shape or tuple(dz.shape) != ((B, D, T) if nct else (B * T, D)) \
            or not (z.is_contiguous() and zq.is_contiguous() and dz.is_contiguous()) \
            or any(t.dtype != torch.float32 for t in (z, zq, dz)):
        raise ValueError("vq_commit_bwd_g: contiguous f32 z, zq [B*T, D]; dz (B, D, T) or [B*T, D]")
    if g is not None and (g.dtype != torch.float32 or g.numel() != 1):
        raise ValueError("vq_commit_bwd_g: the upstream gradient must be a one-element f32 device tensor")
    call("vqx_vq_commit_bwd_g", ptr(z), ptr(zq), B, D, T, float(s), ptr(g), int(nct), ptr(dz), stream_ptr())
    return dz


def cu_masked_stream(reserve_cus):
    """A torch ExternalStream on all but `reserve_cus` CUs of the current
    device (vqx_stream_create_cu_mask) and the CU count it may use; release it
    with release_stream(stream)."""
    s = ctypes.c_void_p()
    used = ctypes.c_int32()
    call("vqx_stream_create_cu_mask", int(reserve_cus), ctypes.byref(s), ctypes.byref(used))
    return torch.cuda.ExternalStream(s.value), used.value


def release_stream(stream):
    call("vqx_stream_destroy", ctypes.c_void_p(stream.cuda_stream))


class Mailbox:
    """Host mailbox for small per-step statistics (vqx_mailbox_*): `slots`
    slots of `floats` f32 values in mapped pinned host memory, each with a
    sequence number the publishing kernel stores last (system-scope release).
    publish() enqueues the copy on the current stream; read(seq, slot) polls
    the slot's number on the host -- no event, no copy on the stream."""

    def __init__(self, slots=64, floats=16):
        import numpy as np
        self.slots, self.floats = int(slots), int(floats)
        h, d = ctypes.c_void_p(), ctypes.c_void_p()
        call("vqx_mailbox_create", self.slots, self.floats, ctypes.byref(h), ctypes.byref(d))
        self._host, self._dev = h.value, d.value
        n = self.slots + self.slots * self.floats
        buf = (ctypes.c_uint32 * n).from_address(self._host)
        self._seq = np.frombuffer(buf, dtype=np.uint32, count=self.slots)
        self._val = np.frombuffer(buf, dtype=np.float32, count=self.slots * self.floats,
                                  offset=4 * self.slots).reshape(self.slots, self.floats)
        self._next = 1

    def publish(self, src, dev_copy=None):
        """Publish src (f32 device tensor, <= floats values) as the next
        sequence number; returns (seq, slot)."""
        _check_cuda(src, dev_copy)
        n = src.numel()
        if n > self.floats or not src.is_contiguous() or src.dtype != torch.float32:
            raise ValueError(f"Mailbox.publish: contiguous f32 tensor of <= {self.floats} values")
        seq, slot = self.reserve()
        call("vqx_mailbox_publish", ptr(src), n, ptr(dev_copy), self._dev, slot, self.slots, self.floats, seq,
             stream_ptr())
        return seq, slot

    def reserve(self):
        """The next (seq, slot), for a launch that publishes itself
        (vq_ema_update(publish=...))."""
        seq, self._next = self._next, self._next + 1
        return seq, seq % self.slots

    def try_read(self, seq, slot, n):
        """The values of `seq` once published (None while pending); raises
        LookupError when the slot has been reused by a later step."""
        s = int(self._seq[slot])
        if s < seq:
            return None
        if s > seq:
            raise LookupError("mailbox slot reused")
        v = self._val[slot, :n].copy()
        if int(self._seq[slot]) != seq:  # overwritten while copying
            raise LookupError("mailbox slot reused")
        return v

    def __del__(self):
        try:
            if getattr(self, "_host", None):
                L.load().vqx_mailbox_destroy(ctypes.c_void_p(self._host))
                self._host = None
        except Exception:
            pass
