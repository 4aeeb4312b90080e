"""Edges of the colour blend loops, forward and backward, on the smallest frames that reach them -- against the oracle, through the helpers and the
bars of tests/test_gpu_parity.py (run, check_color, check_grads, GRAD_TOL).

What the scenes are for:
  * list lengths 1 .. 65 on ONE 16 x 16 tile: every remainder of the backward's 16-entry chunk and the forward's 64-entry round, and a chunk that
    holds a single entry;
  * clamped stacks (opacity 1, G = 1 to within the clamp): every alpha is 0.99 exactly, final_T at termination is the oracle's to the bit;
  * stacks of opacity-0.99 Gaussians: pixels that terminate at even and odd list positions, in consecutive entries, and quadrants of one tile that
    terminate at different entries (a terminated pixel keeps the transmittance it had before the entry that ended it);
  * small Gaussians in quadrant 1, 2, 3 or 1 + 3 of the tile alone: the first quadrant a wave evaluates is not quadrant 0, the others are skipped;
  * 17 x 17 and 33 x 19: edge tiles with pixels outside the image, and a tile with an empty list;
  * the deterministic slab mode on the length-17 list (the butterfly reducer and the slab's own addressing).
Every case runs on a black and on a non-black background (the backward sums through LDS on the first and through the butterfly on the second), with
and without a gradient for means2D_abs (the two tile-wave kernels), one wave per tile; a subset also one wave per quadrant.

check_color's allowance for pixels whose n_contrib differs is a SHARE of the frame; at 256 pixels it must be zero.  The seeds below are those for which
the oracle's two float builds (operation by operation / contracted) agree on n_contrib in every pixel -- no pair sits within rounding of the 1/255
test or of the 1e-4 termination test; test_seeds_leave_no_pixel_undecided checks that, and what each scene claims to contain, without a GPU.

final_T against the oracle.  n_contrib is compared exactly everywhere, and so is the invariant final_T >= 1e-4 (a blend that would take T below the
threshold is not made and the pixel keeps its old T).  final_T itself cannot be the oracle's to the bit in general: alpha = o G comes from two different
exponentials (expf of the power / the hardware's exp2 of the staged exponent E); on the two-entry list 95 of 256 pixels already differ in the last bit.
It is compared to the bit where it can be: in the two clamped-stack scenes every blended alpha is the clamp 0.99 on both sides (1 - 0.99f is exact, so
T (1 - alpha) with one rounding equals the library's T - alpha T with one rounding), the pixels end inside the list, and the CPU test asserts that those
pixels exist; and in pixels nothing touches (T = 1).  Everywhere else the bound is derived: E is three products of magnitude <= log2(255) = 8 with
about six roundings of 2^-24 between them, |dE| <= 6 * 8 * 2^-24 = 2.9e-6, d alpha / alpha = ln 2 dE <= 2^-19, and a blend moves T by at most
alpha T * 2^-19 <= 2^-19: (list length) * 2^-19 per pixel."""
import numpy as np
import pytest
import torch

import oracle
from ibgs_amd import rasterizer, synthetic as syn
from tests import hipref
from tests.metrics import rel_l2
from tests.test_gpu_parity import GRAD_TOL, check_color, check_grads, run

LENGTHS = (1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65)
QUADRANTS = {"q1": (1,), "q2": (2,), "q3": (3,), "q13": (1, 3)}
BACKGROUNDS = {"black": (0.0, 0.0, 0.0), "colour": (0.3, 0.6, 0.9)}


def _base(P, W, H, seed):
    return syn.make_scene(P, W, H, sh_degree=1, seed=seed)          # (its colours and its random rotations are kept)


def _place(inp, uv, depth, sigma_px, opacity):
    """Gaussians whose centres project to the pixel coordinates uv (P,2) at the given camera depths, about sigma_px wide on screen: axes of 0.85, 1 and 1.15 times
    that size under the scene's random rotations (an isotropic Gaussian has a rotation gradient of exactly zero, which only rounding noise would fill)."""
    cam, W, H = inp["_cam"], inp["W"], inp["H"]
    uv = np.asarray(uv, np.float64); depth = np.asarray(depth, np.float64)
    x = ((2.0 * uv[:, 0] + 1.0) / W - 1.0) * cam["tanfovx"] * depth
    y = ((2.0 * uv[:, 1] + 1.0) / H - 1.0) * cam["tanfovy"] * depth
    pc = np.stack([x, y, depth], axis=1)
    R = np.asarray(cam["R"], np.float64)
    inp["means3D"] = (pc @ R.T + np.asarray(cam["campos"], np.float64)).astype(np.float32)
    focal = W / (2.0 * cam["tanfovx"])
    s = np.asarray(sigma_px, np.float64) * depth / focal
    inp["scales"] = (s[:, None] * np.array([0.85, 1.0, 1.15])).astype(np.float32)
    inp["opacities"] = np.asarray(opacity, np.float32).reshape(-1, 1)
    return inp


def length_scene(n, seed=None):
    """n wide, faint Gaussians near the centre of one 16 x 16 frame: the tile's list has n entries and nobody terminates."""
    rng = np.random.default_rng(100 + n if seed is None else seed)
    inp = _base(n, 16, 16, seed=n)
    uv = 7.5 + rng.uniform(-1.0, 1.0, (n, 2))
    return _place(inp, uv, 3.5 + 0.01 * rng.permutation(n), rng.uniform(4.0, 6.0, n), rng.uniform(0.04, 0.12, n))


def termination_scene(seed=1):
    """Twenty-four opacity-0.99 Gaussians of 3 .. 7 pixels scattered over the tile: every pixel ends somewhere between the 4th and the last entry."""
    rng = np.random.default_rng(seed)
    n = 24
    inp = _base(n, 16, 16, seed=40)
    return _place(inp, rng.uniform(1.0, 14.0, (n, 2)), 3.5 + 0.02 * rng.permutation(n), rng.uniform(3.0, 7.0, n), np.full(n, 0.99))


def clamped_stack_scene(front, seed=9):
    """Six opacity-1 Gaussians 120 pixels wide behind one another: G >= 0.99 in every pixel of the tile, so every alpha is the clamp 0.99 in the oracle's
    arithmetic and in the library's alike (-log2 1 = 0 exactly, exp2(-E) >= 0.99 for E <= 0.0145).  T goes 1 -> fl(1 - 0.99f) and the next entry ends
    the pixel (T (1 - 0.99f) = 9.99998e-5 < 1e-4).  front = 1: a one-pixel Gaussian in quadrant 3 in front of the stack -- the pixels it does not reach
    skip it and end one list position later."""
    rng = np.random.default_rng(seed)
    n = 6 + front
    inp = _base(n, 16, 16, seed=70 + front)
    uv = 7.5 + rng.uniform(-0.5, 0.5, (n, 2)); sig = np.full(n, 120.0); op = np.full(n, 1.0); depth = 3.6 + 0.02 * rng.permutation(n)
    if front:
        uv[0] = (11.5, 11.5); sig[0] = 0.9; op[0] = 0.5; depth[0] = 3.5
    return _place(inp, uv, depth, sig, op)


def quadrant_scene(which, seed=5):
    """Five Gaussians of about one pixel (1.2 .. 1.4 with the low-pass filter) at the centre of each named 8 x 8 quadrant of the tile (1 = right top, 2 = left bottom, 3 = right bottom)."""
    rng = np.random.default_rng(seed)
    qs = QUADRANTS[which]
    n = 5 * len(qs)
    c = np.concatenate([np.tile([[3.5 + 8 * (q & 1), 3.5 + 8 * (q >> 1)]], (5, 1)) for q in qs])
    inp = _base(n, 16, 16, seed=50)
    return _place(inp, c + rng.uniform(-0.3, 0.3, (n, 2)), 3.5 + 0.02 * rng.permutation(n), rng.uniform(0.85, 1.1, n), rng.uniform(0.3, 0.6, n))


def ragged_scene(W, H, seed=7):
    """Forty Gaussians of 1.5 .. 3 pixels along the top of a frame whose last tile column is mostly outside the image and whose last tile row they do not reach."""
    rng = np.random.default_rng(seed)
    n = 40
    inp = _base(n, W, H, seed=60)
    uv = np.stack([rng.uniform(1.0, W - 4.0, n), rng.uniform(1.0, 5.0, n)], axis=1)
    return _place(inp, uv, 3.5 + 0.01 * rng.permutation(n), rng.uniform(1.5, 3.0, n), rng.uniform(0.2, 0.7, n))


CASES = {("len", n): (lambda n=n: length_scene(n)) for n in LENGTHS}
CASES[("term", 0)] = termination_scene
CASES.update({("quad", k): (lambda k=k: quadrant_scene(k)) for k in QUADRANTS})
CASES[("clamp", 0)] = lambda: clamped_stack_scene(0)
CASES[("clamp", 1)] = lambda: clamped_stack_scene(1)
CASES[("ragged", 17)] = lambda: ragged_scene(17, 17)
CASES[("ragged", 33)] = lambda: ragged_scene(33, 19)
# one wave per tile everywhere; one wave per quadrant where the list length or the termination is what the case is about
RUNS = [(c, "tile") for c in CASES] + [(c, "quadrant") for c in (("len", 1), ("len", 17), ("len", 65), ("term", 0), ("clamp", 0), ("clamp", 1), ("ragged", 33))]
T_ONE_CLAMPED_BLEND = np.float32(np.float32(1.0) * (np.float32(1.0) - np.float32(0.99)))          # T after one blend at the clamp; a second one would end below 1e-4 and is never stored
T_END = np.float32(0.0001)


def all_clamped(ref):
    """Pixels whose blends were all at alpha = 0.99 (the clamped stacks): there final_T can be, and must be, the oracle's to the bit."""
    return ref["final_T"] == T_ONE_CLAMPED_BLEND


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def test_seeds_leave_no_pixel_undecided():
    """CPU: the oracle's two float builds agree on n_contrib in every pixel of every scene, and the scenes hold what their names say."""
    for case, make in CASES.items():
        inp = make()
        ref = oracle.forward(inp, cull=True)
        with oracle.variant("fma"):
            alt = oracle.forward(inp, cull=True)
        assert np.array_equal(ref["n_contrib"], alt["n_contrib"]), case
        assert np.array_equal(ref["point_list"], alt["point_list"]), case
        W, H = inp["W"], inp["H"]
        nc = ref["n_contrib"].reshape(H, W); fT = ref["final_T"].reshape(H, W)
        rg = ref["ranges"].astype(np.int64); ln = rg[:, 1] - rg[:, 0]
        if case[0] == "len":
            assert ln.tolist() == [case[1]], (case, ln)
            assert fT.min() > 1e-3 and (nc > 0).all()
        if case[0] == "term":
            done = (fT < 0.0101) & (nc <= ln[0] - 4)          # T (1 - alpha) < 1e-4 with alpha <= 0.99 needs T < 0.01; and well inside the list
            ends = np.unique(nc[done])
            assert ends.size >= 3 and (ends % 2 == 0).any() and (ends % 2 == 1).any() and (np.diff(ends) == 1).any(), ends
            per_q = [set(nc[qy:qy + 8, qx:qx + 8][done[qy:qy + 8, qx:qx + 8]].tolist()) for qy in (0, 8) for qx in (0, 8)]
            assert sum(1 for s in per_q if s) >= 3 and len(set(map(frozenset, per_q))) >= 3, per_q
            assert done.mean() > 0.5
        if case[0] == "clamp":
            cl = all_clamped(ref).reshape(H, W)
            assert ln.tolist() == [6 + case[1]]
            assert (nc[cl] < ln[0]).all() and (nc[cl] >= 1).all()          # blended once, ended inside the list
            if case[1] == 0:
                assert cl.all() and (nc == 1).all()
            else:          # the front Gaussian's pixels are not exact; the others skipped it and blended list position 2
                assert 150 < cl.sum() < 256 and set(nc[cl].tolist()) == {2} and not cl[8:, 8:].all() and cl[:8, :8].all()
        if case[0] == "quad":
            hit = {(2 * (y >= 8) + (x >= 8)) for y, x in zip(*np.nonzero(nc))}
            assert hit == set(QUADRANTS[case[1]]), (case, hit)
        if case[0] == "ragged":
            gx = (W + 15) // 16
            assert (ln == 0).any() and ln.max() > 16
            edge = [t for t in range(ln.size) if ln[t] > 0 and ((t % gx) * 16 + 16 > W or (t // gx) * 16 + 16 > H)]
            assert edge, "no edge tile with a list"


def _with_bg(inp, bg):
    inp = dict(inp)
    inp["bg"] = np.array(BACKGROUNDS[bg], np.float32)
    return inp


def _hip_grads_without_abs(inp, g):
    """The same call with means2D_abs needing no gradient (IBGS_FLAG_NO_ABS_GRAD: the noabs kernels)."""
    st = hipref.settings_from(inp, "cuda")
    lv = hipref.leaf_inputs(inp, "cuda")
    lv["means2D_abs"] = torch.zeros_like(lv["means2D_abs"])
    out = rasterizer.GaussianRasterizer(st)(means3D=lv["means3D"], means2D=lv["means2D"], means2D_abs=lv["means2D_abs"], opacities=lv["opacities"],
                                            shs=lv["shs"], scales=lv["scales"], rotations=lv["rotations"])
    (out[0] * torch.as_tensor(g, device="cuda")).sum().backward()
    torch.cuda.synchronize()
    return out[0].detach().cpu().numpy(), lv


@pytest.mark.gpu
@pytest.mark.parametrize("bg", sorted(BACKGROUNDS))
@pytest.mark.parametrize("case,shape", RUNS, ids=[_ids(c) + "-" + s for c, s in RUNS])
def test_blend_loop_edge(case, shape, bg):
    inp = _with_bg(CASES[case](), bg)
    H, W = inp["H"], inp["W"]
    g = np.random.default_rng(11).normal(size=(3, H, W)).astype(np.float32)
    old = rasterizer.WAVE_SHAPE
    rasterizer.WAVE_SHAPE = shape
    try:
        ref, o, ist, leaves, gb = run(inp, {"color": g}, cull=True)
        col_noabs, lv_noabs = _hip_grads_without_abs(inp, g)
    finally:
        rasterizer.WAVE_SHAPE = old
    check_color(o, ist, ref, frac_contrib=0.0)
    assert np.array_equal(ist["n_contrib"], ref["n_contrib"])
    n_list = int((ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]).max())
    dT = np.abs(ist["final_T"] - ref["final_T"])
    clamped = all_clamped(ref)
    print("\n[%s %s %s] final_T: max |d| %.3e (bound %.3e), %d of %d pixels differ in a bit, %d all-clamped pixels of which %d differ"
          % (_ids(case), shape, bg, dT.max(), n_list * 2.0 ** -19, int((dT > 0).sum()), dT.size, int(clamped.sum()), int((dT[clamped] > 0).sum())))
    assert dT.max() <= n_list * 2.0 ** -19
    # exact, whatever the alphas: a pixel never keeps a transmittance below the termination threshold -- the blend that would take it there is not made, and the
    # pixel keeps the T it had (a kernel that stored the tested value instead would fall below)
    assert (ist["final_T"] >= T_END).all() and (ref["final_T"] >= T_END).all()
    untouched = ref["n_contrib"] == 0
    assert np.array_equal(ist["final_T"][untouched], ref["final_T"][untouched]) and (ref["final_T"][untouched] == 1.0).all()
    if case[0] == "clamp":
        assert clamped.sum() > 150, "the clamped stack must leave pixels whose final_T is exact"
        assert np.array_equal(ist["final_T"][clamped].view(np.uint32), ref["final_T"][clamped].view(np.uint32))
        assert (ist["n_contrib"][clamped] < n_list).all()          # ... and they ended inside the list
    check_grads(leaves, gb, tol=GRAD_TOL)
    assert np.array_equal(col_noabs, o["color"])                         # the forward does not know about the statistic
    assert lv_noabs["means2D_abs"].grad is None
    check_grads({k: v for k, v in lv_noabs.items() if k != "means2D_abs"}, gb, tol=GRAD_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("bg", sorted(BACKGROUNDS))
@pytest.mark.parametrize("shape", ["tile", "quadrant"])
def test_deterministic_slab_on_a_seventeen_entry_list(shape, bg):
    """As tests/test_gpu_deterministic.py checks the mode: two runs equal to the bit, the atomic mode's sums in another order, the oracle's gradients."""
    inp = _with_bg(length_scene(17), bg)
    g = np.random.default_rng(12).normal(size=(3, 16, 16)).astype(np.float32)
    names = ("means3D", "means2D", "means2D_abs", "shs", "opacities", "scales", "rotations")

    def grads(det):
        rasterizer.DETERMINISTIC = det
        outs, lv, _ = hipref.run_forward(inp)
        (outs["color"] * torch.as_tensor(g, device="cuda")).sum().backward()
        torch.cuda.synchronize()
        return lv

    old = (rasterizer.WAVE_SHAPE, rasterizer.DETERMINISTIC)
    rasterizer.WAVE_SHAPE = shape
    try:
        a, b, c = grads(True), grads(True), grads(False)
    finally:
        rasterizer.WAVE_SHAPE, rasterizer.DETERMINISTIC = old
    for k in names:
        assert torch.equal(a[k].grad, b[k].grad), "%s differs between two deterministic runs" % k
        assert float(a[k].grad.abs().max()) > 0, k
        assert rel_l2(a[k].grad.cpu().numpy(), c[k].grad.cpu().numpy()) < 1e-5, k
    ref = oracle.forward(inp, cull=True)
    check_grads(a, oracle.backward(inp, ref, g), tol=GRAD_TOL)
