"""Plain chunks of the colour blend (csrc/common.h: clamp_free; render_fwd.hip, render_bwd.hip) against the same kernels with IBGS_FLAG_NO_PLAIN_CHUNKS.

A chunk of staged records (64 in the forward, 16 in the backward) none of which can reach the alpha clamp (-log2 opacity >= CLAMP_FREE_NLO) and none of which is
near-singular is walked by loops without the clamp and without the near-singular branches.  min(0.99, .) is the identity on such a chunk, so nothing may change by
one bit, in either pass -- and therefore nothing says which loop ran: these tests ask through the switch (rasterizer.PLAIN_CHUNKS = False sets the flag) that the
two sets of loops agree, on scenes where every chunk is plain, where none is, and where they mix inside one tile; that the plain loops are the ones running on the
headline workload is read from the instruction counters (profiles/r10_parent_ab.txt).

  * forward: colour, final_T, n_contrib and tile_walked bit-identical with and without the switch, on every set;
  * deterministic backward: two runs with plain chunks are bit-identical, and bit-identical to the switch-off run, on every set (white background, opacities on
    either side of the boundary, a needle's rows included);
  * both builds meet the float64 arbiter's bar (tests/test_gpu_anisotropic.py: |HIP - f64| <= max(1e-3, F64_K |oracle fp32 - f64|) in relative L2);
  * float atomics, one wave per tile: the deterministic mode keeps the butterfly reduce (render_bwd.hip: lds_red needs float-atomic accumulation), so the cases above
    never run the LDS-reduce loops and their plain twins -- the loops of render_bwd_color_kernel on the headline workload.  Those run on scenes whose every Gaussian
    lies inside ONE tile (test_lds_reduce_loops_under_the_switch): each accumulation row then receives one atomic per column, from one wave, onto zeros, so the default
    mode is deterministic there too and is held to the same equalities -- two runs, and the switch -- on all-plain tiles and on tiles that mix plain and ordinary chunks.
    (On frames where rows collect atomics from several tiles an on-vs-off distance samples the order of the atomics: one array's run-to-run relative L2 moved between
    1.9e-8 and 5.7e-8 in four runs of ONE build on the 72 x 56 scenes below, so no such bar is asserted here; at C3 every gradient of this build lies 0.95 .. 1.26 x the
    parent's own run-to-run distance from the parent's, bar 2: profiles/r10_outputs_ab.txt.)

What these tests cannot show: WHICH loop ran.  The plain loops compute the ordinary loops' bits by design, so a dispatch that never chose them would pass every test of
this file; on the device, which side of CLAMP_FREE_NLO a staged record falls on is not observable either (the host's compile of clamp_free is asked at the threshold
+- 1 ulp, nothing more).  That the plain loops are taken rests on the instruction counters alone (SQ_INSTS_VALU per launch, profiles/r10_parent_ab.txt).

(The plain backward loop could also form q = (alpha T) dL/dalpha instead of (o G) (dL/dalpha T), one multiply less per pair.  That was built and measured here, MI355X,
both wave shapes: deterministic on-vs-off relative L2 1e-8 .. 4.3e-7 per gradient array, within twice the distance between the oracle's plain and fma builds on
every set (rho: 6e-8 .. 9e-7); but under float atomics dL/dscales and dL/drotations sat 3.2e-7 .. 4.0e-7 from the switch-off run against a run-to-run distance of
1.2e-7 .. 1.3e-7 -- ratios 2.5 .. 3.2, over the bar of 2 -- so the loops keep the ordinary form and the bars above became equalities.)

Frames of 72 x 56 pixels (5 x 4 tiles, the right column and the bottom row cut), 600 Gaussians sized so that every tile's list spans several chunks in both
passes, SH degree 3.  Every case runs with rasterizer.WAVE_SHAPE = "tile" (render_fwd_kernel<0, 4, 4> and render_bwd_color_kernel, the 1080p kernels) and with the
default shape (on 20 tiles: the quadrant-wave kernels, whose black-background loops are the butterfly pair).
"""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
from ibgs_amd import _lib, rasterizer
from tests import hipref
from tests.scenes import scene
from tests.test_gpu_anisotropic import check_grads_aniso, f64_truth
from tests.test_gpu_background import with_needles
from tests.test_gpu_hybrid import NAMES, arena_words
from tests.test_gpu_parity import rnd

W, H, P = 72, 56, 600
NT = ((W + 15) // 16) * ((H + 15) // 16)
SCALE_MUL = 2.0          # footprints of ~3 x 3 tiles: lists of 150-300 entries per tile
WHITE = (1.0, 1.0, 1.0)
SHAPES = ["tile", None]

def _ulps(x, k):
    """float32 x moved by k units in the last place"""
    return (np.array([x], np.float32).view(np.int32) + np.int32(k)).view(np.float32)[0]


def boundary_opacities():
    """Opacities around the two boundaries.  `thr` = the float32 nearest 2^-CLAMP_FREE_NLO; 4 ulp of an opacity near 0.98 are 3.5e-7 in -log2(o), several times
    what v_log_f32 can be off by there, so `free` stages above the threshold and `bound` below it whatever the hardware's last bit; `at` may fall on either side."""
    t = float(_lib.load().ibgs_clamp_free_threshold())
    thr = np.float32(2.0 ** -np.float64(t))
    c = np.float32(0.99)
    return SimpleNamespace(free=_ulps(thr, -4), at=thr, bound=_ulps(thr, 4), clamp=(_ulps(c, -1), c, _ulps(c, 1)))


def mixed_opacities(op, name, rng):
    """Sets (b) / (e): 5 % of the Gaussians opaque; set c_mix: a tenth on and around both boundaries -- plain and ordinary chunks inside one tile either way"""
    n = op.shape[0]
    op = op.copy()
    if name == "c_mix":
        b = boundary_opacities()
        idx = rng.choice(n, n // 10, replace=False)
        vals = np.array([b.free, b.at, b.bound, *b.clamp], np.float32)
        op[idx, 0] = vals[np.arange(idx.size) % vals.size]
    else:
        idx = rng.choice(n, n // 20, replace=False)
        op[idx[::2]] = 0.995; op[idx[1::2]] = 0.9999
    return op


PER_TILE = 72          # one-tile scenes: entries per tile list = two staging rounds of the forward, five chunks of the backward


@functools.lru_cache(maxsize=None)
def one_tile_scene(name):
    """PER_TILE small Gaussians per tile, every one of them inside its tile: centres 5 pixels from the tile's inner edges, sigma <= 1 pixel (+ the 0.3 low-pass), the
    exact cull's reach 2.6 sigma (opacity 0.1) .. 3.4 sigma (opacity 1) -- so every accumulation row gets its atomics from ONE wave.  Opacities: set (a), (b) or c_mix."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    n = PER_TILE * gx * gy
    base = scene(P=n, W=W, H=H, deg=3, seed=33, opacity="init")
    rng = np.random.default_rng(12)
    V = np.asarray(base["viewmatrix"], np.float64).reshape(4, 4)
    right, up, fwd = V[:3, 0], V[:3, 1], V[:3, 2]
    cam = np.asarray(base["campos"], np.float64)
    fx = W / (2.0 * float(base["tanfovx"])); fy = H / (2.0 * float(base["tanfovy"]))
    d0 = float(np.median((base["means3D"] - cam) @ fwd))
    xyz, sc = np.zeros((n, 3)), np.zeros((n, 3))
    i = 0
    for ty in range(gy):
        for tx in range(gx):
            x1, y1 = min(16 * tx + 16, W), min(16 * ty + 16, H)          # (nothing lies beyond the frame's edge: the cut tiles are open there)
            for _ in range(PER_TILE):
                u = rng.uniform(16 * tx + 5.0, x1 - 5.0 if x1 < W else W - 0.5); v = rng.uniform(16 * ty + 5.0, y1 - 5.0 if y1 < H else H - 0.5)
                dep = d0 * rng.uniform(0.8, 1.2)
                xyz[i] = cam + fwd * dep + right * (u - W / 2) * dep / fx + up * (v - H / 2) * dep / fy
                sc[i] = rng.uniform(0.5, 1.0) * dep / fx
                i += 1
    inp = dict(base)
    inp["means3D"], inp["scales"] = xyz.astype(np.float32), sc.astype(np.float32)
    op = np.full((n, 1), 0.1, np.float32)
    inp["opacities"] = op if name == "a" else mixed_opacities(op, name, rng)
    return inp, {"color": rnd((3, H, W), 19)}


@functools.lru_cache(maxsize=None)
def get_scene(name):
    """(oracle-style inputs, upstream gradient of the colour).  Read-only: shared by the tests below."""
    if name.startswith("one_tile_"):
        return one_tile_scene(name[len("one_tile_"):])
    base = scene(P=P, W=W, H=H, deg=3, seed=31, opacity="init", scale_mul=SCALE_MUL)          # every opacity 0.1
    rng = np.random.default_rng(5)
    inp = dict(base)
    op = base["opacities"].copy()
    b = boundary_opacities()
    if name in ("b", "e", "c_mix"):
        op = mixed_opacities(op, name, rng)
    elif name == "c_free":          # every record just on the free side: every chunk plain
        op[:] = b.free
    elif name == "c_bound":         # every record on the clamped side of the threshold: no chunk plain
        vals = np.array([b.bound, *b.clamp], np.float32)
        op[:, 0] = vals[np.arange(P) % vals.size]
    elif name == "d":               # one near-singular needle across the frame: its chunks are ordinary, the others plain
        inp = with_needles(base, seed=9, n=1, sigma_px=60.0)
        op = inp["opacities"].copy()
    else:
        assert name == "a", name
    inp["opacities"] = op.astype(np.float32)
    if name == "e":
        inp["bg"] = np.asarray(WHITE, np.float32)
    return inp, {"color": rnd((3, H, W), 17)}


@functools.lru_cache(maxsize=None)
def oracles(name):
    """fp32 oracle forward and gradients, and the float64 arbiter's gradients"""
    inp, g = get_scene(name)
    r = oracle.forward(inp, tex_quant=rasterizer.TEX_QUANT, cull=True)
    gb = oracle.backward(inp, r, g["color"], tex_quant=rasterizer.TEX_QUANT)
    return r, gb, f64_truth(inp, g)[1]


@contextlib.contextmanager
def library(shape, plain, det):
    old = (rasterizer.WAVE_SHAPE, rasterizer.PLAIN_CHUNKS, rasterizer.DETERMINISTIC)
    rasterizer.WAVE_SHAPE, rasterizer.PLAIN_CHUNKS, rasterizer.DETERMINISTIC = shape, plain, det
    rasterizer._order_hints.clear()
    try:
        yield
    finally:
        rasterizer.WAVE_SHAPE, rasterizer.PLAIN_CHUNKS, rasterizer.DETERMINISTIC = old
        rasterizer._order_hints.clear()


def hip_pass(name, shape, plain, det):
    inp, grads = get_scene(name)
    with library(shape, plain, det):
        lv = hipref.leaf_inputs(inp, "cuda", True)
        outs = dict(zip(NAMES, rasterizer.GaussianRasterizer(hipref.settings_from(inp, "cuda"))(
            means3D=lv["means3D"], means2D=lv["means2D"], means2D_abs=lv["means2D_abs"], opacities=lv["opacities"], shs=lv["shs"],
            colors_precomp=lv["colors_precomp"], scales=lv["scales"], rotations=lv["rotations"], cov3D_precomp=lv["cov3D_precomp"], all_map=lv["all_map"])))
        ist = hipref.internal_state(outs, inp)
        ipt = int(arena_words(outs, inp, "meta", 32)[10])          # waves per tile of the forward variant that ran: that many words per tile
        walked = arena_words(outs, inp, "tile_walked", NT * ipt).reshape(NT, ipt)
        (outs["color"] * torch.as_tensor(grads["color"], device="cuda")).sum().backward()
        torch.cuda.synchronize()
    g = {k: v.grad.cpu().numpy() for k, v in lv.items() if v is not None and v.grad is not None}
    return SimpleNamespace(color=outs["color"].detach().cpu().numpy(), ist=ist, walked=walked, g=g, leaves=lv)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def check_forward_same(on, off):
    assert same_bits(on.color, off.color), "colour"
    for k in ("final_T", "n_contrib"):
        assert same_bits(on.ist[k], off.ist[k]), k
    assert np.array_equal(on.walked, off.walked), "tile_walked"


def test_clamp_free_on_the_host():
    """csrc/common.h: clamp_free.  The threshold lies above -log2(0.99), where the clamp starts to bind, with the margin the comment there asks for; NaN and -0 are
    not free."""
    lib = _lib.load()
    t = np.float32(lib.ibgs_clamp_free_threshold())
    assert abs(float(t) + np.log2(0.98)) < 1e-6 and float(t) > -np.log2(0.99) + 0.01
    free = lambda x: int(lib.ibgs_clamp_free(float(np.float32(x))))
    assert free(t) == 1 and free(np.nextafter(t, np.float32(1))) == 1 and free(np.nextafter(t, np.float32(0))) == 0
    assert free(-np.log2(0.1)) == 1 and free(np.inf) == 1          # opacity 0.1; opacity 0 stages to +inf (and passes no alpha test)
    assert free(-np.log2(0.99)) == 0 and free(0.0) == 0 and free(-0.0) == 0 and free(-1.0) == 0 and free(-np.inf) == 0
    assert free(np.nan) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["tile", "default"])
@pytest.mark.parametrize("name", ["a", "b", "c_mix", "c_free", "c_bound", "d", "e"])
def test_plain_chunks_against_the_switch(name, shape):
    ref, gb, g64 = oracles(name)
    on, on2, off = hip_pass(name, shape, True, True), hip_pass(name, shape, True, True), hip_pass(name, shape, False, True)
    # the scene does what it is for: lists of several chunks in both passes, in every tile; edge tiles
    n = (on.ist["ranges"][:, 1] - on.ist["ranges"][:, 0]).astype(np.int64)
    far = on.walked.max(axis=1)
    deep = 16 if name in ("c_free", "c_bound") else 64          # (every Gaussian near-opaque: a pixel is finished after three hits, the walks are short)
    assert n.min() > 64 and (far > deep).mean() >= 0.5, (n.min(), far)
    assert W % 16 != 0 and H % 16 != 0
    # forward: not one bit
    check_forward_same(on, off)
    assert np.abs(on.color - ref["color"]).mean() < 1e-5
    # deterministic backward: the same from run to run and under the switch; the arbiter's bar
    for k in on.g:
        assert same_bits(on.g[k], on2.g[k]), "%s differs between two runs with plain chunks" % k
        assert same_bits(on.g[k], off.g[k]), "%s differs under the switch" % k
    assert max(np.abs(v).max() for v in on.g.values()) > 0
    check_grads_aniso(on.leaves, gb, g64)
    print("[plain] %s / %s: R %d, lists %d..%d, walked %d..%d" % (name, shape, on.ist["R"], n.min(), n.max(), far.min(), far.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c_mix"])
def test_lds_reduce_loops_under_the_switch(name):
    """render_bwd_color_kernel as the headline runs it: float-atomic accumulation on a black background, i.e. the LDS-reduce loops and their plain twins.  Every
    Gaussian lies inside one tile, so a row's atomics come from one wave and land on zeros: the same bits from run to run, and the same under the switch."""
    scn = "one_tile_" + name
    inp, _ = get_scene(scn)
    ref, gb, g64 = oracles(scn)
    n_g = inp["means3D"].shape[0]
    assert ref["num_rendered"] == n_g and int(ref["tiles_touched"].max()) == 1, "a Gaussian reaches a second tile"
    on, on2, off = hip_pass(scn, "tile", True, False), hip_pass(scn, "tile", True, False), hip_pass(scn, "tile", False, False)
    n = (on.ist["ranges"][:, 1] - on.ist["ranges"][:, 0]).astype(np.int64)
    assert on.ist["R"] == n_g and n.min() == PER_TILE and on.walked.shape[1] == 1 and on.walked.min() > 16, (on.ist["R"], n, on.walked.ravel())
    # the backward's chunks of 16, counted down from where the forward stopped: which hold a record that is certainly ordinary, which only certainly plain ones
    bo = boundary_opacities()
    both = 0
    for t in range(NT):
        ids = on.ist["point_list"][on.ist["ranges"][t, 0]:on.ist["ranges"][t, 0] + int(on.walked[t, 0])]
        o = inp["opacities"].reshape(-1)[ids][::-1]
        kinds = {("ordinary" if (c >= bo.bound).any() else ("plain" if (c <= bo.free).all() else "either")) for c in (o[i:i + 16] for i in range(0, o.size, 16))}
        both += {"ordinary", "plain"} <= kinds
    assert both == 0 if name == "a" else both >= NT // 2, "tiles that mix plain and ordinary chunks: %d of %d" % (both, NT)
    check_forward_same(on, off)
    assert np.abs(on.color - ref["color"]).mean() < 1e-5
    for k in on.g:
        assert same_bits(on.g[k], on2.g[k]), "%s differs between two float-atomic runs: a row collected atomics from two waves" % k
        assert same_bits(on.g[k], off.g[k]), "%s differs under the switch" % k
    assert max(np.abs(v).max() for v in on.g.values()) > 0
    check_grads_aniso(on.leaves, gb, g64)
    print("[plain] %s / tile, float atomics: R %d, lists %d, walked %d..%d" % (scn, on.ist["R"], n.min(), on.walked.min(), on.walked.max()))
