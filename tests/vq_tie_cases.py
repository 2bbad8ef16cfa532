"""Inputs on which vqx_vq_forward's first-minimum rule decides the answer
(tests/test_gpu_vq_ties.py), built in plain torch on the CPU, with the
preconditions that tests/test_vq_ties_host.py proves from float64 alone.

The expected index of a frame is always the rule's: the lowest index among the
codes at the float64 minimum distance (`first_min`).  It is never taken from
the kernel.

The kernel scores code c at LDS step c // 64, in code split (c % 64) // 16, in
lane c % 16 (vq_forward_kernel, vqx_vq.hip): a strict '<' keeps the first
minimum of a lane over the steps, a 16-lane shuffle merge and then an LDS
merge over the four splits break ties towards the lower index.  The planted
twins below are named for the stage that has to decide them.
"""
from types import SimpleNamespace

import torch

DIMS = (64, 128, 256)
FRAMES_PER_TWIN = 40

# name -> (K, groups of identical rows (lowest index first), frames per group)
PLANTED = {
    # (3, 9) shuffle merge; (15, 16) neighbouring splits, the lower index in the higher lane; (63, 64) last split
    # of step 0 against first split of step 1; (5, 69) same lane and split, next step; two pairs of mixed stages
    "k256_pairs": (256, ((3, 9), (15, 16), (63, 64), (5, 69), (20, 200), (70, 135)), FRAMES_PER_TWIN),
    # row 135 cannot equal both row 70 and row 7, so the triple has a codebook of its own
    "k256_triple": (256, ((7, 71, 135),), FRAMES_PER_TWIN),
    "k256_n33": (256, ((15, 16), (63, 64), (5, 69)), 11),  # N = 33: one full workgroup and one frame
    "k2048_ends": (2048, ((0, 2047),), FRAMES_PER_TWIN),
    "k16_ends": (16, ((0, 15),), FRAMES_PER_TWIN),
    "k128_all_rows": (128, (tuple(range(128)),), FRAMES_PER_TWIN),  # every row identical: every frame gets 0
}
GRID_K = (16, 128, 1024, 2048)
GRID_N = 777
NONFINITE = dict(N=70, K=128, D=128, nan_elem=5, nan_row=40, inf_elem=66, big_elem=68)


def distances(z, E):
    """The reference's distance order, (||z||^2 + ||e||^2) - 2 z.e, in the dtype of z and E."""
    return (z.pow(2).sum(1, keepdim=True) + E.pow(2).sum(1)) - 2 * z @ E.t()


def distances_by_code(z, E):
    """`distances` with each code's dot products formed by the same elementwise operations, so that identical
    codebook rows get bit-identical distances whatever a BLAS does with different columns."""
    dot = torch.stack([(z * E[k]).sum(1) for k in range(E.shape[0])], dim=1)
    return (z.pow(2).sum(1, keepdim=True) + E.pow(2).sum(1)) - 2 * dot


def first_min(dist):
    """The lowest index among the codes at each row's minimum."""
    K = dist.shape[1]
    at_min = dist == dist.min(1, keepdim=True).values
    return torch.where(at_min, torch.arange(K), K).min(1).values


def last_min(dist):
    at_min = dist == dist.min(1, keepdim=True).values
    return torch.where(at_min, torch.arange(dist.shape[1]), -1).max(1).values


def planted(name, D):
    """E = randn(K, D) with each group's rows overwritten by its first; frames z = E[a] + 0.05 randn, the groups
    interleaved frame by frame so that each has frames in the last, partial 32-frame workgroup.  Returns z, E,
    expect (the group's lowest index per frame) and groups."""
    K, groups, per = PLANTED[name]
    gen = torch.Generator().manual_seed(1000 * K + D + len(groups))
    E = torch.randn(K, D, generator=gen)
    for g in groups:
        E[list(g[1:])] = E[g[0]].clone()
    N = per * len(groups)
    expect = torch.tensor([groups[n % len(groups)][0] for n in range(N)])
    z = E[expect] + 0.05 * torch.randn(N, D, generator=gen)
    assert N % 32, "the last workgroup must be partial"
    return SimpleNamespace(name=name, K=K, D=D, N=N, z=z, E=E, expect=expect, groups=groups, per=per)


def grid(K, D):
    """z (777, D) and E (K, D) with entries from {-1, 0, 1}: every product, norm and partial sum is a small
    integer, so any summation order gives the float64 distance exactly, in float32 too."""
    gen = torch.Generator().manual_seed(77 * K + D)

    def draw(n):  # -1, 0, 1 with probability 1/3 each
        zero = torch.rand(n, D, generator=gen) < 1 / 3
        sign = torch.where(torch.rand(n, D, generator=gen) < 0.5, -1.0, 1.0)
        return torch.where(zero, torch.zeros(()), sign)

    E, z = draw(K), draw(GRID_N)
    expect = first_min(distances(z.double(), E.double()))
    return SimpleNamespace(K=K, D=D, N=GRID_N, z=z, E=E, expect=expect)


def duplicated_halves(K, D, seed, scale=1.0):
    """A codebook with E[K/2:] = E[:K/2]: every frame's nearest code has a twin K/2 above it."""
    E = torch.randn(K, D, generator=torch.Generator().manual_seed(seed)) * scale
    E[K // 2:] = E[:K // 2]
    return E


def nonfinite():
    """70 frames near codes of a randn codebook, four of them poisoned (two in the last, partial workgroup of 6
    frames): one NaN element, an all-NaN row, one +inf element, one element of 3e38 whose square overflows.
    `clean` holds zeros in the poisoned rows."""
    c = NONFINITE
    gen = torch.Generator().manual_seed(4040)
    E = torch.randn(c["K"], c["D"], generator=gen)
    code = torch.randint(0, c["K"], (c["N"],), generator=gen)
    clean = E[code] + 0.05 * torch.randn(c["N"], c["D"], generator=gen)
    poisoned = [c["nan_elem"], c["nan_row"], c["inf_elem"], c["big_elem"]]
    clean[poisoned] = 0.0
    z = clean.clone()
    z[c["nan_elem"], 17] = float("nan")
    z[c["nan_row"]] = float("nan")
    z[c["inf_elem"], 100] = float("inf")
    z[c["big_elem"], 3] = 3e38
    finite = torch.ones(c["N"], dtype=torch.bool)
    finite[poisoned] = False
    return SimpleNamespace(z=z, clean=clean, E=E, finite=finite, poisoned=poisoned, **c)
