"""Preconditions of the tie cases of tests/vq_tie_cases.py, proved on the CPU
from float64 (and stock float32) torch alone: what tests/test_gpu_vq_ties.py
then demands of vqx_vq_forward follows from the first-minimum rule, not from
the kernel."""
import pytest
import torch

from tests import vq_tie_cases as C


@pytest.mark.parametrize("D", C.DIMS)
@pytest.mark.parametrize("name", list(C.PLANTED))
def test_planted_twins_tie_exactly_and_nothing_else_is_near(name, D):
    c = C.planted(name, D)
    dist = C.distances_by_code(c.z.double(), c.E.double())
    assert torch.equal(C.first_min(dist), c.expect) and torch.equal(dist.argmin(1), c.expect)
    in_last = torch.arange(c.N) >= c.N // 32 * 32
    worst = float("inf")
    for g in c.groups:
        rows = c.expect == g[0]
        assert int(rows.sum()) == c.per, g
        if name == "k256_n33":  # one full workgroup and one frame
            assert c.N == 33 and int(in_last.sum()) == 1
        else:
            assert c.per == 40 and bool((rows & in_last).any()) and bool((rows & ~in_last).any()), g
        for b in g[1:]:
            assert g[0] < b and torch.equal(c.E[b], c.E[g[0]])
            assert torch.equal(dist[rows, b], dist[rows, g[0]]), (g, b)  # the twins' distances are equal
        others = torch.ones(c.K, dtype=torch.bool)
        others[list(g)] = False
        if others.any():
            third = dist[rows][:, others].min(1).values
            worst = min(worst, float(((third - dist[rows, g[0]]) / third).min()))
    print(f"planted {name} D={D}: smallest relative gap to the best other code {worst:.3f}")
    assert worst >= 0.5


@pytest.mark.parametrize("D", C.DIMS)
@pytest.mark.parametrize("K", C.GRID_K)
def test_grid_distances_are_exact_and_ties_arise(K, D):
    c = C.grid(K, D)
    d64 = C.distances(c.z.double(), c.E.double())
    assert torch.equal(C.distances(c.z, c.E).double(), d64)  # float32 in stock torch is exact here
    assert torch.equal(d64, d64.round())
    tied = (d64 == d64.min(1, keepdim=True).values).sum(1) > 1
    differs = C.first_min(d64) != C.last_min(d64)
    print(f"grid K={K} D={D}: {int(tied.sum())} frames with a tied minimum, {int(differs.sum())} first != last")
    assert int(tied.sum()) >= 20 and int(differs.sum()) >= 20
    assert torch.equal(c.expect, d64.argmin(1))  # torch.argmin returns the first minimum
    # a strictly nearer higher-indexed code must still win: some frames' minimum is unique and not at code 0
    assert int((~tied & (c.expect > 0)).sum()) >= 20


def test_nonfinite_frames_sit_where_the_case_says():
    c = C.nonfinite()
    assert (c.N, c.K, c.D) == (70, 128, 128) and tuple(c.z.shape) == (70, 128)
    last = c.N // 32 * 32
    assert sorted(c.poisoned) == sorted([c.nan_elem, c.nan_row, c.inf_elem, c.big_elem])
    assert sum(r >= last for r in c.poisoned) == 2 and c.N % 32
    assert int(torch.isnan(c.z[c.nan_elem]).sum()) == 1 and bool(torch.isnan(c.z[c.nan_row]).all())
    assert int(torch.isinf(c.z[c.inf_elem]).sum()) == 1
    assert bool(torch.isfinite(c.z[c.big_elem]).all()) and bool(torch.isinf(c.z[c.big_elem].pow(2).sum()))
    assert bool(torch.isfinite(c.z[c.finite]).all()) and torch.equal(c.z[c.finite], c.clean[c.finite])
    assert not bool(c.clean[c.poisoned].any()) and int(c.finite.sum()) == c.N - 4
    # torch.argmin gives 0 on a row of NaN distances
    dist = C.distances(c.z, c.E)
    for r in (c.nan_elem, c.nan_row):
        assert bool(torch.isnan(dist[r]).all()) and int(dist[r].argmin()) == 0
    # the finite frames have one clear nearest code
    d64 = C.distances(c.clean.double(), c.E.double())[c.finite]
    top2 = torch.topk(d64, 2, dim=1, largest=False).values
    assert float(((top2[:, 1] - top2[:, 0]) / top2[:, 1]).min()) >= 0.5


@pytest.mark.parametrize("K,D", [(16, 64), (512, 128)])
def test_duplicated_halves_put_a_twin_above_every_code(K, D):
    E = C.duplicated_halves(K, D, 5)
    assert torch.equal(E[K // 2:], E[:K // 2])
    z = torch.randn(50, D, generator=torch.Generator().manual_seed(6))
    assert int(C.first_min(C.distances_by_code(z.double(), E.double())).max()) < K // 2
