"""vqvae2b without a GPU: the model's tree equals the fixtures' key lists
(tests/golden/make_golden_vqvae2b.py), an unconditioned ResSkip block owns no
conv_cond, the refusals and decode's argument checks are loud, and
vqx_upsample_cat_bwd_to is declared, bound and validates before launching,
with the ABI still 130."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests.hier_model_ref import fixture

MODEL_CASES = ("ema_gst", "plain_last", "pooled_ema")
NEW = "vqx_upsample_cat_bwd_to"


def _model(meta, **over):
    from vae_npvc_amd.model.vqvae2b import Model
    return Model(dict(meta["arch"], **over))


# ------------------------------------------------------------------ entry point
def test_new_symbol_is_declared_bound_and_the_abi_is_130():
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd import ops
    header = (ROOT / "include" / "vqx.h").read_text()
    assert re.search(rf"\bint {NEW}\(", header)
    assert NEW in L._SIGS and NEW in L.EXPORTS and hasattr(L.load(), NEW)
    assert L._SIGS[NEW] == L._SIGS["vqx_upsample_cat_bwd"][:-1] + [ctypes.c_int32, ctypes.c_void_p]
    assert L.ABI_VERSION == 130 and "#define VQX_ABI_VERSION 130" in header
    assert callable(ops.upsample_cat_bwd_to)


def test_new_symbol_validates_before_launching():
    """Every -1 condition is checked on the host: none of these calls reaches a device."""
    from vae_npvc_amd import _lib as L
    lib = L.load()
    F32, BF16 = L.VQX_F32, L.VQX_BF16

    def levels(*specs):
        arr = (L.HierLevel * len(specs))()
        for e, (z, Tl, C, ld) in zip(arr, specs):
            e.z, e.T_l, e.C, e.ld = z, Tl, C, ld
        return arr
    ok = levels((64, 3, 8, 8))
    bad = [
        (ok, 1, 2, 7, 64, 8, F32, 7),                          # level_dtype neither F32 nor BF16
        (ok, 1, 2, 7, 64, 8, F32, -1),
        (None, 1, 2, 7, 64, 8, F32, BF16),                     # null levels
        (ok, 0, 2, 7, 64, 8, F32, BF16),                       # n_levels out of 1..8
        (levels(*[(64, 1, 4, 4)] * 9), 9, 2, 7, 64, 36, F32, BF16),
        (ok, 1, 2, 7, 64, 8, 7, BF16),                         # dout dtype
        (ok, 1, 0, 7, 64, 8, F32, BF16),                       # B < 1
        (ok, 1, 2, 0, 64, 8, F32, BF16),                       # T < 1
        (ok, 1, 1 << 16, 1 << 16, 64, 8, F32, BF16),           # B*T >= 2^31
        (ok, 1, 2, 7, 0, 8, F32, BF16),                        # null dout
        (ok, 1, 2, 7, 72, 8, F32, BF16),                       # dout not 16-B aligned
        (levels((0, 3, 8, 8)), 1, 2, 7, 64, 8, F32, BF16),     # null level
        (levels((72, 3, 8, 8)), 1, 2, 7, 64, 8, F32, BF16),    # unaligned level
        (levels((64, 8, 8, 8)), 1, 2, 7, 64, 8, F32, BF16),    # T_l > T
        (levels((64, 0, 8, 8)), 1, 2, 7, 64, 8, F32, BF16),    # T_l < 1
        (levels((64, 3, 6, 8)), 1, 2, 7, 64, 8, F32, BF16),    # C not a multiple of 4
        (levels((64, 3, 8, 4)), 1, 2, 7, 64, 8, F32, BF16),    # ld < C
        (levels((64, 3, 8, 10)), 1, 2, 7, 64, 8, F32, BF16),   # ld not a multiple of 4
        (ok, 1, 2, 7, 64, 4, F32, BF16),                       # sum C_l > ldo
        (ok, 1, 2, 7, 64, 10, F32, BF16),                      # ldo not a multiple of 4
    ]
    for args in bad:
        assert getattr(lib, NEW)(*args, None) == -1, args[1:]
        assert NEW.encode() in lib.vqx_last_error(), args[1:]
    assert getattr(lib, NEW)(*bad[0], None) == -1 and b"level_dtype" in lib.vqx_last_error()


# ------------------------------------------------------------------ unconditioned blocks
def test_unconditioned_resskip_block_owns_no_conv_cond():
    from vae_npvc_amd.model.layers import ResSkipBlock
    cond = ResSkipBlock(32, 16, 16)
    keys = list(cond.state_dict().keys())
    for none in (0, None):
        blk = ResSkipBlock(32, none, 16)
        assert blk.conv_cond is None
        assert list(blk.state_dict().keys()) == [k for k in keys if not k.startswith("conv_cond.")]
        assert [k for k, _ in blk.named_parameters()] == [k for k, _ in cond.named_parameters()
                                                          if not k.startswith("conv_cond.")]
    assert any(k.startswith("conv_cond.") for k in keys)


def test_decoder_plan_indexes_six_tensors_per_unconditioned_block():
    from vae_npvc_amd.model.hier_decoder import Decoder, Plan as _Plan
    args = fixture("vq2b", "ema_gst")[0]["arch"]["final_decoder"]
    free, cond = Decoder(**args), Decoder(**dict(args, cond_channels=16))
    blocks = sum(args["stacks"])
    assert _Plan(free).n_tensors == len(_Plan.tensors(free)) == 2 + 6 * blocks + 4
    assert _Plan(cond).n_tensors == len(_Plan.tensors(cond)) == 2 + 8 * blocks + 4
    assert _Plan(free).cond == 0 and all(st[2] is None for st in _Plan(free).steps if st[0] == "block")
    assert not any(".conv_cond." in k for k in free.state_dict())


def test_decoder_conditioning_argument_checks():
    from vae_npvc_amd.model.vqvae2 import Decoder
    args = fixture("vq2b", "ema_gst")[0]["arch"]["final_decoder"]
    x = torch.zeros(2, 96, 8)
    with pytest.raises(ValueError, match="unconditioned"):
        Decoder(**args)((x, torch.zeros(2, 16, 8)))
    with pytest.raises(ValueError, match="unconditioned"):
        Decoder(**args)((x, [torch.zeros(2, 16, 1)]))
    with pytest.raises(ValueError, match="None"):
        Decoder(**dict(args, cond_channels=16))((x, None))


def test_flat_model_still_refuses_an_unconditioned_decoder():
    import yaml
    from vae_npvc_amd.model.vqvae import Model
    cfg = yaml.safe_load(open(ROOT / "vae_npvc_amd" / "conf" / "vcc20.yaml"))
    cfg["decoder"] = dict(cfg["decoder"], cond_channels=0)
    with pytest.raises(NotImplementedError, match="cond_channels 0"):
        Model(cfg)


# ------------------------------------------------------------------ model
@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_tree_is_the_reference_tree(case):
    meta, arr = fixture("vq2b", case)
    m = _model(meta)
    assert list(m.state_dict().keys()) == meta["keys"]
    assert [k for k, _ in m.named_parameters()] == meta["params"]
    assert [k for k, _ in m.named_buffers()] == meta["buffers"]
    assert [n for n, _ in m.named_children()] == ["encoders", "quantizers", "decoders", "embeds", "final_decoder",
                                                  "jitter"]
    assert not any(".conv_cond." in k for k in meta["keys"] if k.startswith("final_decoder."))
    m.load_state_dict({k: torch.from_numpy(arr["param." + k].copy()) for k in meta["keys"]}, strict=True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), arr["param." + k]), k
    assert meta["gap"] >= 1e-3
    assert meta["tiled_gap_ratio"] is None or meta["tiled_gap_ratio"] >= 1.0
    ys = arr["ys"]
    assert ys.shape == (meta["B"], m.levels) and all(len(set(r)) == m.levels for r in ys.tolist())


def test_refused_configurations_raise_at_construction():
    from vae_npvc_amd.model.vqvae2b import Model
    plain = fixture("vq2b", "plain_last")[0]["arch"]
    gst = fixture("vq2b", "ema_gst")[0]["arch"]
    with pytest.raises(NotImplementedError, match="jitter_p"):
        Model(dict(plain, pooling_last=True))  # a pooled quantized top with jitter
    Model(dict(plain, pooling_last=True, jitter_p=0.0))
    with pytest.raises(NotImplementedError, match="pooling_last"):
        Model(dict(gst, pooling_last=False))  # the style layer would receive a 3-D tensor
    with pytest.raises(NotImplementedError, match="resampling"):
        Model(dict(plain, **{"decoder.1": dict(plain["decoder.1"], upsample_scales=[2])}))
    with pytest.raises(ValueError, match="compute_dtype"):
        Model(dict(plain, compute_dtype="fp16"))
    with pytest.raises(ValueError, match="levels"):
        Model(dict(plain, levels=4))
    with pytest.raises(ValueError, match="cond_channels"):
        Model(dict(plain, final_decoder=dict(plain["final_decoder"], cond_channels=16)))
    with pytest.raises(ValueError, match="final_channels"):
        Model(dict(plain, final_decoder=dict(plain["final_decoder"], in_channels=[64])))
    one = dict(gst, levels=1, jitter_p=0.0, final_decoder=dict(gst["final_decoder"], in_channels=[32]))
    assert Model(one).use_gst is False  # forced off at one level
    assert Model(gst).pooling_last is True and Model(plain).upsample_last is True


def test_decode_argument_checks_and_cpu_inputs():
    from vae_npvc_amd._lib import VqxError
    meta, arr = fixture("vq2b", "ema_gst")
    m = _model(meta)
    B = meta["B"]
    zs = [torch.from_numpy(arr[f"enc.{i}"].copy()) for i in range(3)]
    zs[2] = zs[2].float()
    ys = torch.from_numpy(arr["ys"].copy())
    bad = [
        ((zs[:2], ys), "one tensor per level"),
        ((zs, ys[:, :2]), r"\(B, levels\)"),
        ((zs, ys[:1]), r"\(B, levels\)"),
        ((zs, ys.float()), r"\(B, levels\)"),
        (([zs[0].float(), zs[1], zs[2]], ys), "int64 indices"),
        (([zs[0], zs[1], zs[2][:, :8]], ys), "style level"),
        (([zs[0], zs[1][:1], zs[2]], ys), "batch size"),
        (([zs[0].clone().index_fill_(1, torch.tensor([3]), 16), zs[1], zs[2]], ys), "level 0 has indices in 0..16"),
        (([zs[0], zs[1].clone().index_fill_(1, torch.tensor([0]), -1), zs[2]], ys), "level 1 has indices in -1"),
        ((zs, ys.clone().index_fill_(1, torch.tensor([1]), 4)), "speakers"),
    ]
    for inp, msg in bad:
        with pytest.raises(ValueError, match=msg):
            m.decode(inp)
    with pytest.raises(ValueError, match="do not stretch"):
        m.decode((zs, ys), time=40)  # 64 frames do not fit 40
    x, y = torch.from_numpy(arr["x"].copy()), torch.from_numpy(arr["y"].copy())
    assert tuple(ys.shape) == (B, 3)
    for f in (lambda: m((x, y)), lambda: m.encode(x), lambda: m.convert((x, y)), lambda: m.decode((zs, ys)),
              lambda: m.infer((x, ys))):
        with pytest.raises(VqxError):
            f()
