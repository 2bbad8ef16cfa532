"""The style-token (GST) layer without a GPU: the C ABI declares and exports
vqx_gst_workspace / vqx_gst_fwd / vqx_gst_bwd, the ctypes mirror GstArgs has
gcc's layout of vqx_gst_args, the envelope is validated before any launch,
and the module has the reference's parameter tree (fixture gst_vae2)."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

from tests.helpers import GOLD, ROOT, load_fixture

HEADER = ROOT / "include" / "vqx.h"
GST_FUNCTIONS = ("vqx_gst_workspace", "vqx_gst_fwd", "vqx_gst_bwd")


def _lib():
    from vae_npvc_amd import _lib as L
    return L, L.load()


def test_header_declares_and_library_exports_the_gst_entry_points():
    L, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(vqx_\w+)\s*\(", text, flags=re.M))
    for f in GST_FUNCTIONS:
        assert f in declared, f
        assert hasattr(lib, f), f
        assert f in L._SIGS, f
    assert "vqx_gst_args" in text


def _c_layout(struct, fields):
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           f'  printf("%zu\\n", sizeof({struct}));']
    src += [f'  printf("%zu\\n", offsetof({struct}, {f}));' for f in fields]
    src += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        with open(c, "w") as f:
            f.write("\n".join(src))
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    return [int(v) for v in out]


def test_gst_args_layout_matches_header():
    L, _ = _lib()
    names = [f[0] for f in L.GstArgs._fields_]
    got = _c_layout("vqx_gst_args", names)
    assert got[0] == ctypes.sizeof(L.GstArgs)
    assert got[1:] == [getattr(L.GstArgs, n).offset for n in names]


def _valid_args(L):
    """The vae2 shapes with dummy non-null pointers: validation fails before
    anything could read them."""
    a = L.GstArgs()
    for name, ctype in L.GstArgs._fields_:
        if ctype is ctypes.c_void_p:
            setattr(a, name, 0x1000)
    a.B, a.T, a.R, a.N, a.E, a.F, a.H, a.ldz, a.lddz = 3, 4, 128, 10, 32, 128, 4, 128, 128
    return a


@pytest.mark.parametrize("fn", ["vqx_gst_fwd", "vqx_gst_bwd"])
def test_gst_validation_errors_are_loud(fn):
    """Bad arguments return non-zero with a message; nothing is launched."""
    L, lib = _lib()
    f = getattr(lib, fn)
    assert f(None, None) != 0
    assert b"null args" in lib.vqx_last_error()
    ld = "ldz" if fn == "vqx_gst_fwd" else "lddz"
    for field, value, word in (("H", 3, b"multiple of H"), ("N", 33, b"tokens"), ("R", 130, b"multiple of 4"),
                               (ld, 127, ld.encode()), ("ws", None, b"null pointer")):
        a = _valid_args(L)
        setattr(a, field, value)
        assert f(ctypes.byref(a), None) != 0, field
        err = lib.vqx_last_error()
        assert fn.encode() in err and word in err, (field, err)
    a = _valid_args(L)
    a.H = 3
    with pytest.raises(L.VqxError, match="multiple of H"):
        L.call(fn, ctypes.byref(a), None)


def test_gst_workspace_is_positive_and_grows_with_batch():
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd import ops
    small = ops.gst_workspace(3, 10, 128, 4, 128, 32)
    large = ops.gst_workspace(96, 10, 128, 4, 128, 32)
    assert 0 < small < large
    # at least what the backward needs saved: ref, a, ctx per row; K, V, tok per token
    assert small >= 3 * (128 + 4 * 10 + 128) + 10 * (128 + 128 + 32)
    with pytest.raises(L.VqxError, match="tokens"):
        ops.gst_workspace(3, 33, 128, 4, 128, 32)


def test_module_has_the_reference_parameter_tree():
    from vae_npvc_amd.model.layers_gst import StyleTokenLayer
    meta, arr = load_fixture("gst_vae2")
    layer = StyleTokenLayer(ref_embed_dim=meta["R"], gst_tokens=meta["N"], gst_token_dim=meta["F"],
                            gst_heads=meta["H"])
    assert list(layer.state_dict().keys()) == meta["keys"]
    sd = {k: torch.from_numpy(arr["param." + k]) for k in meta["keys"]}
    layer.load_state_dict(sd, strict=True)
    assert torch.equal(layer.mha.linear_out.weight.detach(), sd["mha.linear_out.weight"])
    # constructor defaults are the reference's: 10 tokens of 256 / 4 = 64, ref_embed_dim 128
    shapes = {k: tuple(v.shape) for k, v in StyleTokenLayer().state_dict().items()}
    assert shapes["gst_embs"] == (10, 64) and shapes["mha.linear_q.weight"] == (256, 128)
    assert shapes["mha.linear_k.weight"] == (256, 64) and shapes["mha.linear_out.weight"] == (256, 256)


def test_fixtures_stay_below_the_committed_file_limit():
    files = sorted(GOLD.glob("gst_*"))
    assert len(files) >= 10
    assert max(f.stat().st_size for f in files) < (1 << 20)


def test_dropout_is_not_built():
    from vae_npvc_amd.model.layers_gst import StyleTokenLayer
    with pytest.raises(NotImplementedError):
        StyleTokenLayer(dropout_rate=0.1)


def test_cpu_input_raises():
    """No CPU fallback: the HIP kernels are the only implementation."""
    from vae_npvc_amd import _lib as L
    from vae_npvc_amd.model.layers_gst import StyleTokenLayer
    layer = StyleTokenLayer(ref_embed_dim=128, gst_tokens=10, gst_token_dim=128, gst_heads=4)
    with pytest.raises(L.VqxError):
        layer(torch.randn(2, 128))
    with pytest.raises(L.VqxError):
        layer.pool_forward(torch.randn(2, 128, 4))
