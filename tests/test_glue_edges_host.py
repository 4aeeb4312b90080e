"""tests/glue_edges.py on the CPU, before any kernel sees it: the cases hold every pixel class they are meant to, the float64 reference has the structural
zeros the GPU tests demand of the kernel, the hole rim is finite on both torch evaluations, and a second fp32 evaluation of the same map (`direct_glue`:
no matrix product, another rounding) passes every per-class bar with K = 2 against torch's own fp32 evaluation as the floor."""
import numpy as np
import pytest
import torch

from tests import glue_edges as ge

ALL = {"hole rim", "deep hole", "column seams", "row seams", "last partial tiles", "border ring", "rest"}
EXPECTED = {          # the non-empty classes of every case
    "197x29 holes": ALL,
    "197x29": ALL - {"hole rim", "deep hole"},
    "64x8": {"column seams", "row seams", "border ring", "rest"},                       # exact multiples of the tile: no partial tile
    "128x16": {"column seams", "row seams", "border ring", "rest"},
    "65x9": {"column seams", "row seams", "last partial tiles", "border ring", "rest"},
    "63x7": {"column seams", "row seams", "last partial tiles", "border ring"},          # one partial tile: every pixel is in it
    "3x3": {"column seams", "row seams", "last partial tiles", "border ring"},
    "2x5": {"column seams", "row seams", "last partial tiles", "border ring"},
    "5x2": {"column seams", "row seams", "last partial tiles", "border ring"},
    "2x2": {"column seams", "row seams", "last partial tiles", "border ring"},
}


@pytest.mark.parametrize("case", sorted(ge.CASES))
def test_classes_and_reference(case):
    r = ge.reference(case)
    assert {n for n in ALL if r.masks[n].any()} == EXPECTED[case]
    assert ge.structural_zeros(r.n64, r.g64, r.masks) == []
    covered = np.zeros((r.H, r.W), bool)
    for n in ALL:
        covered |= r.masks[n]
    assert covered.all()                                                    # every pixel is compared in some class
    interior = ~r.masks["border"]
    if interior.any() and not r.masks["hole rim"].any():
        assert (np.abs(r.n64[:, interior]).sum(0) > 0).all()               # a hole-free map has a normal everywhere inside
    else:
        assert interior.any() == (min(r.W, r.H) >= 3)


def test_the_holes_reach_the_clamp_branch():
    r = ge.reference("197x29 holes")
    g = ge.gradient_classes(r.masks, r.g64)
    assert g["hole rim, huge"].sum() >= 20 and g["hole rim, ordinary"].sum() >= 100 and r.masks["deep hole"].sum() >= 20
    assert 1e15 < np.abs(r.g64).max() < 1e25                              # far inside fp32's range
    assert np.abs(r.g64[~(r.masks["hole rim"] | r.masks["deep hole"])]).max() < ge.HUGE
    # the holes sit where they are meant to: on a column and a row seam, in the corner, in the last partial tile at the right edge
    z = r.depth.numpy() == 0
    assert z[7, 63] and z[8, 64] and z[0, 0] and z[20, 100] and z[25, 196] and not z[28, 196]
    assert (r.masks["hole rim"] & (np.arange(r.W)[None, :] >= 192) & (np.arange(r.H)[:, None] >= 24)).any()


@pytest.mark.parametrize("case", sorted(ge.CASES))
def test_a_second_fp32_evaluation_passes_every_bar(case):
    r = ge.reference(case)
    floor = ge.evaluate(ge.torch_glue, r.cam, r.depth, r.cot, torch.float32, "cpu")
    cand = ge.evaluate(ge.direct_glue, r.cam, r.depth, r.cot, torch.float32, "cpu")
    assert ge.structural_zeros(*cand, r.masks) == [] and ge.structural_zeros(*floor, r.masks) == []
    _, bad_n = ge.class_distances(case + " normal", cand[0], floor[0], r.n64, ge.normal_classes(r.masks), K=2.0)
    _, bad_g = ge.class_distances(case + " dL/ddepth", cand[1], floor[1], r.g64, ge.gradient_classes(r.masks, r.g64), K=2.0)
    assert bad_n == [] and bad_g == []


@pytest.mark.parametrize("case", ["197x29 holes", "197x29", "65x9"])
def test_lattice_cotangent_support(case):
    r = ge.reference(case, lattice=True)
    s = ge.lattice_support(r.W, r.H)
    assert s.any() and (~s).any() and (r.g64[~s] == 0).all()
    assert (r.g64[s] != 0).mean() > 0.5
    assert (r.cot.numpy() != 0).any(0).sum() == len(range(1, r.H, 3)) * len(range(1, r.W, 3))


def test_a_wrong_seam_is_seen_by_its_classes():
    """The point of the classes: a one-column error at a tile seam is far over the bar of every class that holds the column, and the rest is as it was."""
    r = ge.reference("197x29")
    floor = ge.evaluate(ge.torch_glue, r.cam, r.depth, r.cot, torch.float32, "cpu")[1]
    cand = floor.copy()
    cand[:, 64] = floor[:, 65]                                              # what an off-by-one in the right-neighbour term does to the first column of a tile
    rows, bad = ge.class_distances("mutant", cand, floor, r.g64, ge.gradient_classes(r.masks, r.g64), K=2.0)
    assert "column seams" in bad and "rest" not in bad
    ratio = dict((n, c / f) for n, _, c, f in rows)["column seams"]
    assert ratio > 1000


def test_guarded_buffers_on_the_host():
    g = ge.Guarded(5, data=torch.arange(5.0), device="cpu")
    assert g.guards_intact() and g.untouched() and g.view.tolist() == [0, 1, 2, 3, 4]
    assert g.ptr() == g.buf.data_ptr() + 4 * ge.GUARD_WORDS and torch.isnan(g.buf.view(torch.float32)[:ge.GUARD_WORDS]).all()
    g.view[4] = 9.0
    assert g.guards_intact() and not g.untouched()
    g.buf[g.lo + 5] = 0
    assert not g.guards_intact()
    o = ge.Guarded(3, device="cpu", shift=1)
    assert (o.bits() == ge.FRESH_BITS).all() and o.ptr() % 16 == 4 and torch.isnan(o.view).all()
