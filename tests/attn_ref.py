"""What the self-attention tests share: the fixtures of
tests/golden/make_golden_attn.py, loaded once and read-only."""
import json

import numpy as np

from tests.helpers import GOLD

CASES = ("one_tile", "single_frame", "odd_T", "multi_tile", "peaked", "ragged", "ragged64", "recipe_T")
TENSORS = ("out", "dx", "linear_q.weight", "linear_q.bias", "linear_k.weight", "linear_v.weight", "linear_v.bias",
           "linear_out.weight", "linear_out.bias")  # linear_k.bias is bounded absolutely (abs32 / abs_bf16)
KB = "linear_k.bias"
_cache = {}


def fixture(case, prefix="attn"):
    """(meta, arrays) of a case, its .npz parts merged."""
    key = (prefix, case)
    if key not in _cache:
        meta = json.load(open(GOLD / f"{prefix}_{case}.json"))
        arr = {}
        for name in meta["files"]:
            arr.update(np.load(GOLD / name, allow_pickle=False))
        for v in arr.values():
            v.setflags(write=False)
        _cache[key] = (meta, arr)
    return _cache[key]
