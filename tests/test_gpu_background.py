"""The blend kernels on non-black backgrounds (train.py --white_background, --random_background) against the oracle.

A background that is not black is a code path of its own: every backward blend body splits on `bg0` into chunk forms, and only the
non-black ones carry the term dL/dalpha += -T_final (bg . dL/dC) / (1 - alpha) (render_bwd.hip); the forward adds T_final * bg per channel
(render_fwd.hip).  The scenes of the other parity files all render on black.  Here every backward entry point launch_render_backward can pick
and every forward variant launch_render_forward can pick meets the oracle with a non-black background, and the background term is judged on
its own: the same scene, flags and upstream gradients run at bg = b and at bg = 0, and the DIFFERENCE of the two gradients (what the term
contributes) is held to the oracle's difference.  The scenes leave part of the frame empty so that the term has weight (final_T > 0.5 on at
least 30 % of the pixels).  Which variant ran is read from the arena, not inferred from the flags."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
from ibgs_amd import _lib, rasterizer, synthetic as syn
from tests import hipref
from tests.metrics import l1, rel_l2
from tests.scenes import add_sources, quat_z_to, scene
from tests.test_gpu_anisotropic import F64_K, check_grads_aniso, f64_truth
from tests.test_gpu_hybrid import NAMES, SPLIT, arena_words
from tests.test_gpu_parity import GEO_GRAD_TOL, GRAD_TOL, check_color, check_grads, check_stages, rnd

pytestmark = pytest.mark.gpu

WHITE = (1.0, 1.0, 1.0)
RAND = tuple(float(v) for v in torch.rand(3, generator=torch.Generator().manual_seed(248)))          # a train.py:248 draw, fixed
ZERO_CH = (0.0, 0.5, 1.0)          # not black, but one channel is: a bg0 test that read one channel would pick the black form
BLACK = (0.0, 0.0, 0.0)
DIFF_TOL = 1e-3          # rel L2 of the background differential grad(b) - grad(0), HIP against the oracle
GEO_UP = 0.1             # the normal / depth / warp upstream gradients, scaled so that the colour loss keeps its weight in dL/dopacity


def left_part(inp, cut):
    """The Gaussians whose centres project left of NDC x = cut: the rest of the frame stays (nearly) empty, final_T ~ 1 there."""
    P = inp["means3D"].shape[0]
    h = np.concatenate([inp["means3D"].astype(np.float64), np.ones((P, 1))], 1) @ np.asarray(inp["projmatrix"], np.float64).reshape(4, 4)
    keep = h[:, 0] / h[:, 3] < cut
    out = dict(inp)
    for k, v in inp.items():
        if k != "bg" and isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == P:
            out[k] = np.ascontiguousarray(v[keep])
    return out


def with_needles(base, seed=9, n=3, sigma_px=60.0):
    """`base` plus n needles (sub-pixel thin, sigma_px long on screen, 20-40 degrees off the image axes): conics past the blend's near-singular
    threshold (BLEND_REF_POWER_RISK, common.h), so the tiles they reach are flagged (tile_risky) and the others are not.  A frame-long needle
    (tests.scenes.giant_needles) would flag every tile of these frames: near-singular conics keep their whole rectangle."""
    rng = np.random.default_rng(seed)
    V = np.asarray(base["viewmatrix"], np.float64).reshape(4, 4)
    right, up, fwd = V[:3, 0], V[:3, 1], V[:3, 2]
    cam = np.asarray(base["campos"], np.float64)
    W, H = int(base["W"]), int(base["H"])
    fx = W / (2.0 * float(base["tanfovx"])); fy = H / (2.0 * float(base["tanfovy"]))
    P0 = base["means3D"].shape[0]
    depth = float(np.median((base["means3D"] - cam) @ fwd))
    mx, ang = [], []
    for i in range(n):
        u, v = rng.uniform(0.3, 0.8) * W, rng.uniform(0.3, 0.7) * H          # screen position of the centre: mid-frame, the needle reaching into the empty part
        mx.append(cam + fwd * depth + right * (u - W / 2) * depth / fx + up * (v - H / 2) * depth / fy)
        ang.append(np.deg2rad(rng.uniform(20.0, 40.0)) * rng.choice([-1.0, 1.0]))
    d = np.stack([np.cos(a) * right + np.sin(a) * up for a in ang])
    s_long = sigma_px * depth / fx
    out = dict(base)
    out["means3D"] = np.concatenate([base["means3D"], np.asarray(mx, np.float32)]).astype(np.float32)
    out["scales"] = np.concatenate([base["scales"], np.tile(np.array([[1e-4 * s_long, 1e-4 * s_long, s_long]], np.float32), (n, 1))]).astype(np.float32)
    out["rotations"] = np.concatenate([base["rotations"], quat_z_to(d).astype(np.float32)]).astype(np.float32)
    out["opacities"] = np.concatenate([base["opacities"], np.full((n, 1), 0.8, np.float32)]).astype(np.float32)
    out["shs"] = np.concatenate([base["shs"], base["shs"][rng.integers(0, P0, n)]]).astype(np.float32)
    if "all_map" in base:
        out["all_map"] = syn.plane_all_map(out["means3D"], out["scales"], out["rotations"], base["_cam"])
    assert out["means3D"].shape[0] == P0 + n
    out["_needles"] = n          # (the last n rows)
    return out


def _geo_grads(H, W):
    return {"color": rnd((3, H, W), 7), "normal_map": GEO_UP * rnd((3, H, W), 8), "median_depth": GEO_UP * rnd((1, H, W), 9),
            "warped_image": GEO_UP * rnd((15, H, W), 10)}


@functools.lru_cache(maxsize=None)
def get_scene(name):
    """(oracle-style inputs on black, upstream gradients).  Frames: 208 x 144 and 176 x 112 (below 768 tiles: quadrant by default, both shapes forced
    here), 648 x 328 = 861 tiles (the hybrid kernels when no shape is forced)."""
    if name in ("colour", "colour_precomp"):
        inp = left_part(scene(P=3000, W=208, H=144, deg=2, seed=3, opacity="trained"), 0.1)
        if name == "colour_precomp":
            inp = {k: v for k, v in inp.items() if k != "shs"}
            inp["sh_degree"] = 0
            inp["colors_precomp"] = np.random.default_rng(2).uniform(0, 1, (inp["means3D"].shape[0], 3)).astype(np.float32)
        return inp, {"color": rnd((3, 144, 208), 1)}
    if name == "hybrid":          # tests/test_gpu_hybrid.uneven_scene's recipe: half of the Gaussians in one blob
        inp = syn.make_scene(12000, 648, 328, sh_degree=1, seed=5, opacity="trained", cluster=0.5)
        inp["scales"] = (inp["scales"] * 2.0).astype(np.float32)
        return left_part(inp, -0.1), {"color": rnd((3, 328, 648), 2)}
    if name in ("geo", "geo_L5"):
        base = left_part(scene(P=2500, W=176, H=112, deg=2, seed=21, opacity="trained", planes=True, scale_mul=1.5), -0.1)
        return add_sources(base, n_src=3, L=5 if name == "geo_L5" else 4), _geo_grads(112, 176)
    if name == "geo_hybrid":
        inp = syn.make_scene(9000, 648, 328, sh_degree=1, seed=99, opacity="trained", with_planes=True, anisotropy="plane", cluster=0.5)
        inp["scales"] = (inp["scales"] * 1.5).astype(np.float32)
        inp["all_map"] = syn.plane_all_map(inp["means3D"], inp["scales"], inp["rotations"], inp["_cam"])
        return add_sources(left_part(inp, -0.2), n_src=3, L=4), _geo_grads(328, 648)
    if name == "needles":
        return with_needles(left_part(scene(P=2500, W=208, H=144, deg=1, seed=7, opacity="trained"), 0.1)), {"color": rnd((3, 144, 208), 3)}
    if name == "needles_geo":
        base = left_part(scene(P=2500, W=176, H=112, deg=1, seed=23, opacity="trained", planes=True, scale_mul=1.5), -0.1)
        return add_sources(with_needles(base, seed=11), n_src=3, L=4), _geo_grads(112, 176)
    raise KeyError(name)


def with_bg(inp, b):
    d = dict(inp)
    d["bg"] = np.asarray(b, np.float32)
    return d


@functools.lru_cache(maxsize=None)
def oracle_at(name, b, variant=None):
    inp, g = get_scene(name)
    inp = with_bg(inp, b)
    if variant == "f64":
        return f64_truth(inp, g)
    r = oracle.forward(inp, tex_quant=rasterizer.TEX_QUANT, cull=True)
    return r, oracle.backward(inp, r, g["color"], g.get("normal_map"), g.get("median_depth"), g.get("warped_image"), tex_quant=rasterizer.TEX_QUANT)


@contextlib.contextmanager
def library_flags(shape=None, det=False, ref_arith=False, hint_geo=False):
    old = (rasterizer.WAVE_SHAPE, rasterizer.DETERMINISTIC, rasterizer.REF_ARITH, rasterizer.ORDER_HINT_GEO)
    rasterizer.WAVE_SHAPE, rasterizer.DETERMINISTIC, rasterizer.REF_ARITH, rasterizer.ORDER_HINT_GEO = shape, det, ref_arith, hint_geo
    rasterizer._order_hints.clear()          # no launch order left by an earlier test's camera (hints are keyed by the view matrix's address)
    try:
        yield
    finally:
        rasterizer.WAVE_SHAPE, rasterizer.DETERMINISTIC, rasterizer.REF_ARITH, rasterizer.ORDER_HINT_GEO = old
        rasterizer._order_hints.clear()


def hip_pass(inp, grads, abs_grad=True, st=None):
    """One forward + backward through the Python surface (debug off: the rendered hint and the launch order hints are live).  The arena words are
    read before (meta, tile_risky: written by the forward) and after the backward (tile_order: written by the backward)."""
    st = st if st is not None else hipref.settings_from(inp, "cuda")
    lv = hipref.leaf_inputs(inp, "cuda", True)
    if not abs_grad:
        lv["means2D_abs"] = torch.zeros_like(lv["means2D_abs"])          # needs no gradient: IBGS_FLAG_NO_ABS_GRAD
    outs = dict(zip(NAMES, rasterizer.GaussianRasterizer(st)(means3D=lv["means3D"], means2D=lv["means2D"], means2D_abs=lv["means2D_abs"],
                                                            opacities=lv["opacities"], shs=lv["shs"], colors_precomp=lv["colors_precomp"],
                                                            scales=lv["scales"], rotations=lv["rotations"], cov3D_precomp=lv["cov3D_precomp"],
                                                            all_map=lv["all_map"])))
    W, H = int(inp["W"]), int(inp["H"])
    nt = ((W + 15) // 16) * ((H + 15) // 16)
    ist = hipref.internal_state(outs, inp)
    meta = arena_words(outs, inp, "meta", 32)
    risky = arena_words(outs, inp, "tile_risky", nt * 4).reshape(nt, 4)
    loss = 0
    for k, g in grads.items():
        loss = loss + (outs[k] * torch.as_tensor(g, device="cuda")).sum()
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    order = arena_words(outs, inp, "tile_order", int(_lib.load().ibgs_tile_order_slots(W, H)))
    g = {k: v.grad.cpu().numpy() for k, v in lv.items() if v is not None and v.grad is not None}
    return SimpleNamespace(o=hipref.to_np(outs), ist=ist, leaves=lv, g=g, meta=meta, risky=risky, order=order, nt=nt)


def hip_run(inp, grads, abs_grad, passes):
    """`passes` calls with ONE settings object (one camera): the second call gets the launch order the first call's backward left."""
    st = hipref.settings_from(inp, "cuda")
    for _ in range(passes):
        h = hip_pass(inp, grads, abs_grad, st)
    return h


# The differential's leaves: every gradient the background term reaches (the colour gradients do not depend on bg at all: test below)
DIFF_PAIRS = [("opacities", "dL_dopacity"), ("means2D", "dL_dmeans2D"), ("means2D_abs", "dL_dmeans2D_abs"), ("means3D", "dL_dmeans3D"),
              ("scales", "dL_dscales"), ("rotations", "dL_drotations"), ("all_map", "dL_dall_map")]

# (id, scene, WAVE_SHAPE, bg, means2D_abs wanted, deterministic whole-gradient run, REF_ARITH, passes) -- a covering set: every backward entry point
# (name in the comment) with a non-black background, ABS and no-ABS where there are both, every forward variant.  The differential always runs
# deterministic; the float-atomic cases check the whole gradient on a float-atomic run.
CASES = [
    # colour, one wave per tile: render_bwd_color_kernel / _noabs_kernel; forward render_fwd_kernel<COLOR,4,4> over the tile map, and under a launch order hint
    ("colour-tile-white-abs-atomic", "colour", "tile", WHITE, True, False, False, 1),
    ("colour-tile-rand-noabs-det", "colour", "tile", RAND, False, True, False, 1),
    ("colour-tile-zeroch-abs-det-hint", "colour", "tile", ZERO_CH, True, True, False, 2),
    ("colour-tile-white-noabs-atomic-hint", "colour", "tile", WHITE, False, False, False, 2),
    # colour, one wave per quadrant: render_bwd_color_small_kernel (no no-ABS twin: the flag must be harmless); forward render_fwd_kernel<COLOR,1,4>
    ("colour-quadrant-white-noabs-atomic", "colour", "quadrant", WHITE, False, False, False, 1),
    ("colour-quadrant-rand-abs-det", "colour", "quadrant", RAND, True, True, False, 1),
    ("colour-quadrant-zeroch-abs-atomic", "colour", "quadrant", ZERO_CH, True, False, False, 1),
    ("colour-precomp-quadrant-white-abs-det", "colour_precomp", "quadrant", WHITE, True, True, False, 1),
    ("colour-precomp-tile-rand-noabs-det", "colour_precomp", "tile", RAND, False, True, False, 1),
    # colour, 861 tiles, no shape forced: render_bwd_color_hybrid_kernel<true / false>; forward render_fwd_color_hybrid_kernel without and with a hint
    ("hybrid-white-abs-det", "hybrid", None, WHITE, True, True, False, 1),
    ("hybrid-rand-noabs-atomic", "hybrid", None, RAND, False, False, False, 1),
    ("hybrid-zeroch-noabs-det-hint", "hybrid", None, ZERO_CH, False, True, False, 2),
    ("hybrid-white-abs-atomic-hint", "hybrid", None, WHITE, True, False, False, 2),
    # geo, tile waves: render_bwd_geo4_kernel / geo4_noabs_kernel; forward render_fwd_kernel<GEO,2,4> over the tile map and under a hint (ORDER_HINT_GEO)
    ("geo-tile-white-abs-atomic", "geo", "tile", WHITE, True, False, False, 1),
    ("geo-tile-rand-noabs-det", "geo", "tile", RAND, False, True, False, 1),
    ("geo-tile-zeroch-abs-det-hint", "geo", "tile", ZERO_CH, True, True, False, 2),
    ("geo-tile-white-noabs-atomic", "geo", "tile", WHITE, False, False, False, 1),
    # geo, quadrant waves: render_bwd_geo_kernel (no no-ABS twin); forward render_fwd_kernel<GEO,1,4>, and <GEO,1,8> for L = 5
    ("geo-quadrant-white-noabs-det", "geo", "quadrant", WHITE, False, True, False, 1),
    ("geo-quadrant-rand-abs-atomic", "geo", "quadrant", RAND, True, False, False, 1),
    ("geo-quadrant-zeroch-abs-det", "geo", "quadrant", ZERO_CH, True, True, False, 1),
    ("geoL5-quadrant-rand-abs-det", "geo_L5", "quadrant", RAND, True, True, False, 1),
    ("geoL5-tile-white-noabs-atomic", "geo_L5", "tile", WHITE, False, False, False, 1),
    # geo, 861 tiles, no shape forced: render_bwd_geo_hybrid_kernel<true / false> (the forward keeps quadrant waves there)
    ("geo-hybrid-white-abs-det", "geo_hybrid", None, WHITE, True, True, False, 1),
    ("geo-hybrid-zeroch-noabs-atomic", "geo_hybrid", None, ZERO_CH, False, False, False, 1),
    # IBGS_FLAG_REF_ARITH on needles: the flagged tiles go to render_bwd_color_risk_kernel / render_bwd_geo_risk_kernel <true / false> behind the fast kernels
    ("needles-tile-white-abs-refarith", "needles", "tile", WHITE, True, True, True, 1),
    ("needles-quadrant-rand-noabs-refarith", "needles", "quadrant", RAND, False, True, True, 1),
    ("needles-default-zeroch-abs-refarith", "needles", None, ZERO_CH, True, True, True, 1),
    ("needles-geo-tile-white-noabs-refarith", "needles_geo", "tile", WHITE, False, True, True, 1),
    ("needles-geo-quadrant-zeroch-abs-refarith", "needles_geo", "quadrant", ZERO_CH, True, True, True, 1),
    # black controls: the same machinery on the black form
    ("colour-tile-black-abs-det", "colour", "tile", BLACK, True, True, False, 1),
    ("geo-quadrant-black-abs-atomic", "geo", "quadrant", BLACK, True, False, False, 1),
]


def check_variant(h, scene_name, shape, ref_arith, passes):
    """Which forward and backward variant ran, from the arena: meta[10] = waves per tile of the forward, meta[11] = 1 when a launch order hint was
    accepted, the split bits of the backward's launch order, the flagged tiles of IBGS_FLAG_REF_ARITH."""
    geo = scene_name.startswith("geo") or scene_name == "needles_geo"
    hybrid_size = 768 <= h.nt < 4096
    if shape == "tile":
        assert h.meta[10] == (2 if geo and int(get_scene(scene_name)[0]["buffer_length"]) <= 4 else (4 if geo else 1)), h.meta[10]
    else:
        assert h.meta[10] == 4, h.meta[10]          # quadrant waves, the hybrid colour kernel (four words per tile), the geo forward below 4 096 tiles
    if passes > 1:
        assert h.meta[11] == 1, "the launch order hint was not accepted"
    tiles = h.order[h.order != 0xFFFFFFFF]
    if shape == "tile" or (shape is None and hybrid_size):          # the backward built a launch order: every tile once
        assert np.array_equal(np.sort(tiles & ~np.uint32(SPLIT)), np.arange(h.nt, dtype=np.uint32))
        nsplit = int(((tiles & SPLIT) != 0).sum())
        if shape == "tile":
            assert nsplit == 0
        else:
            assert 0 < nsplit < h.nt, ("no mixture of split and unsplit tiles", nsplit, h.nt)
    flagged = int(h.risky.any(axis=1).sum())
    if ref_arith:
        assert 0 < flagged < h.nt, ("the risk kernel and the fast kernels must both have tiles", flagged, h.nt)
    return flagged


def diff_check(name, hb, h0, gbb, gb0, arb=None, rows=slice(None)):
    """Background differential: grad(b) - grad(0) of the HIP path against the oracle's, over the Gaussians `rows`.  arb = (float64 grads at b, at 0):
    on needles the bar is the arbiter's, F64_K times the fp32 oracle's own distance from the float64 differential."""
    dist = {}
    for lk, rk in DIFF_PAIRS:
        if lk not in hb.g or rk not in gbb:
            continue
        a = (hb.g[lk].astype(np.float64) - h0.g[lk])[rows].reshape(-1)
        b = (gbb[rk].astype(np.float64) - gb0[rk]).reshape(hb.g[lk].shape)[rows].reshape(-1)
        if np.abs(b).max() == 0:
            assert np.abs(a).max() == 0, "%s: the oracle's gradient does not depend on bg, the HIP path's does" % lk
            continue
        e = rel_l2(a, b)
        if arb is None:
            dist[lk] = e
            assert e <= DIFF_TOL, "%s: background differential relL2 %.3e" % (lk, e)
        else:
            t = (np.asarray(arb[0][rk], np.float64) - arb[1][rk]).reshape(hb.g[lk].shape)[rows].reshape(-1)
            e64, floor = rel_l2(a, t), rel_l2(b, t)
            dist[lk] = e64
            assert e64 <= max(DIFF_TOL, F64_K * floor), "%s: background differential relL2 vs float64 %.3e (oracle fp32: %.3e)" % (lk, e64, floor)
    print("[bg] %s: differential relL2 %s" % (name, ", ".join("%s %.1e" % kv for kv in dist.items())))
    return dist


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_background_against_the_oracle(case):
    name, sname, shape, b, abs_grad, det, ref_arith, passes = case
    inp0, grads = get_scene(sname)
    inpb = with_bg(inp0, b)
    geo = bool(inp0.get("render_geo"))
    refb, gbb = oracle_at(sname, b)
    ref0, gb0 = oracle_at(sname, BLACK)
    with library_flags(shape, det=True, ref_arith=ref_arith, hint_geo=geo and passes > 1):
        hb = hip_run(inpb, grads, abs_grad, passes)
    with library_flags(shape, det=True, ref_arith=ref_arith, hint_geo=geo and passes > 1):
        h0 = hip_run(inp0, grads, abs_grad, passes)
    flagged = check_variant(hb, sname, shape, ref_arith, passes)
    assert (hb.ist["final_T"] > 0.5).mean() >= 0.3, "the background has too little weight in this scene"
    if not abs_grad:
        assert "means2D_abs" not in hb.g
    # forward: the oracle at b, and C(b) - C(0) = fl(final_T * b) per pixel and channel (final_T itself does not depend on bg)
    check_stages(hb.ist, hb.o, refb)
    if ref_arith:          # (as tests/test_gpu_anisotropic.test_geo_and_depth_only_passes_on_giant_needles)
        assert l1(hb.o["color"], refb["color"]) <= 1e-5 and (hb.ist["n_contrib"] != refb["n_contrib"]).mean() <= 2e-4
        assert l1(hb.ist["final_T"], refb["final_T"]) < 1e-5
    else:
        check_color(hb.o, hb.ist, refb)
    assert np.array_equal(hb.ist["final_T"], h0.ist["final_T"]) and np.array_equal(hb.ist["n_contrib"], h0.ist["n_contrib"])
    H, W = int(inp0["H"]), int(inp0["W"])
    want = (hb.ist["final_T"].reshape(1, H, W) * np.asarray(b, np.float32)[:, None, None]).astype(np.float64)
    got = hb.o["color"].astype(np.float64) - h0.o["color"]
    err = float(np.abs(got - want).max())
    assert err <= 2.5e-7, "C(b) - C(0) differs from final_T * b by %.3e" % err
    if geo:          # nothing but the colour depends on bg
        for k in ("normal_map", "median_depth", "cam_feat", "warped_image", "min_depth_diff", "camera_ray", "use_first_src_frame_mask"):
            assert np.array_equal(hb.o[k], h0.o[k]), k
    # backward, whole gradient at b: deterministic run, or a float-atomic one
    whole = hb
    if not det:
        with library_flags(shape, det=False, ref_arith=ref_arith, hint_geo=geo and passes > 1):
            whole = hip_run(inpb, grads, abs_grad, passes)
    arb = None
    if ref_arith:
        arb = (oracle_at(sname, b, "f64")[1], oracle_at(sname, BLACK, "f64")[1])
        check_grads_aniso(whole.leaves, gbb, arb[0], only=[lk for lk, v in whole.leaves.items() if v is not None and v.grad is not None])
    else:
        check_grads(whole.leaves, gbb, tol=GEO_GRAD_TOL if geo else GRAD_TOL, skip=() if abs_grad else ("means2D_abs",))
    # backward, the background differential.  On the needle scenes the three needles carry most of it (their pairs go through the risk kernels'
    # reference-arithmetic term; dL/dscales of a needle is where the fp32 oracle itself is farthest from float64, so the arbiter's bar is loose there).
    # The ordinary Gaussians' rows are judged again on their own: their pairs take the fast form of the term, in the fast kernels on unflagged tiles and
    # in the risk kernels' ordinary branch on flagged ones.  The fast kernels' term is covered at full strength by the cases without needles.
    diff_check(name, hb, h0, gbb, gb0, arb)
    if ref_arith:
        diff_check(name + " (without the needles' rows)", hb, h0, gbb, gb0, arb, rows=slice(0, -int(inp0["_needles"])))
    if b == WHITE:          # the term has weight here: a scene where it did not would pass any test of it
        d = np.linalg.norm(gbb["dL_dopacity"].astype(np.float64) - gb0["dL_dopacity"])
        assert d >= 0.05 * np.linalg.norm(gbb["dL_dopacity"]), "the background term is %.3f of dL/dopacity" % (d / np.linalg.norm(gbb["dL_dopacity"]))
    if b == BLACK:
        for lk in hb.g:
            assert np.array_equal(hb.g[lk], h0.g[lk]), lk
    # the colour gradients do not depend on bg: bit-identical in deterministic mode
    for lk in ("shs", "colors_precomp"):
        if lk in hb.g:
            assert np.array_equal(hb.g[lk], h0.g[lk]), "%s depends on the background" % lk
    print("[bg] %s: R %d, meta[10] %d, final_T > 0.5 on %.2f, flagged tiles %d of %d, bg share of dL/dopacity %.3f"
          % (name, hb.ist["R"], hb.meta[10], (hb.ist["final_T"] > 0.5).mean(), flagged, hb.nt,
             np.linalg.norm(gbb["dL_dopacity"].astype(np.float64) - gb0["dL_dopacity"]) / np.linalg.norm(gbb["dL_dopacity"])))


@pytest.mark.parametrize("L", [4, 5])
def test_depth_only_pass_ignores_the_background(L):
    """render_fwd_kernel<DEPTH,4,4> and <DEPTH,4,8>: bit-identical depth for a white and a black background."""
    inp = dict(get_scene("geo")[0])
    inp.update(render_geo=False, render_depth_only=True, buffer_length=L)
    res = []
    for b in (WHITE, BLACK):
        outs, _, _ = hipref.run_forward(with_bg(inp, b), requires_grad=False)
        res.append(hipref.to_np(outs))
    assert np.abs(res[0]["median_depth"]).max() > 0
    assert np.array_equal(res[0]["median_depth"], res[1]["median_depth"]) and np.array_equal(res[0]["radii"], res[1]["radii"])


def test_batched_depth_pass_ignores_the_background():
    from ibgs_amd import renderer
    from tests.test_gpu_depth_batch import _setup
    dev, pc, cams, scn, pipe, args, _ = _setup(3000, 160, 112, 4, seed=17)
    with torch.no_grad():
        a = renderer.render_depth_batch(cams[:4], pc, scn, pipe, args, torch.ones(3, device=dev), True, 3, 4)
        z = renderer.render_depth_batch(cams[:4], pc, scn, pipe, args, torch.zeros(3, device=dev), True, 3, 4)
    assert float(a.abs().max()) > 0 and torch.equal(a, z)


def renderer_setup(P=4000, W=448, H=448, n_views=6, seed=11, cut=0.0):
    """tests/test_gpu_renderer._setup's model, cameras and images, keeping only the Gaussians whose centres project left of NDC x = cut in camera 0:
    a third of that view shows the background (final_T > 0.5), so a wrong background moves the gradients far past the whole-gradient bar."""
    from ibgs_amd import simple_scene
    dev = torch.device("cuda")
    g = syn.make_gaussians(P, seed, sh_degree=2, max_coeffs=9, opacity="trained")
    g["scales"] = (g["scales"] * 1.6).astype(np.float32)
    rng = np.random.default_rng(seed)
    g["normal"] = rng.normal(size=(P, 3)).astype(np.float32); g["offset"] = (0.02 * rng.normal(size=(P, 1))).astype(np.float32)
    cams = simple_scene.orbit_cameras(W, H, n_views=n_views, device=dev, nearest=3)
    h = np.concatenate([g["means3D"].astype(np.float64), np.ones((P, 1))], 1) @ cams[0].full_proj_transform.cpu().numpy().astype(np.float64)
    keep = h[:, 0] / h[:, 3] < cut
    g = {k: np.ascontiguousarray(v[keep]) for k, v in g.items()}
    pc = simple_scene.SimpleGaussians(g, sh_degree=2, device=dev)
    imgs = torch.rand(n_views, 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    return dev, g, pc, cams, simple_scene.SimpleScene(cams, images=imgs, device=dev)


@pytest.mark.parametrize("geo", [False, True])
def test_random_background_iterations_through_the_renderer(geo):
    """train.py --random_background: two consecutive iterations on one camera, each with its own torch.rand(3) background, through renderer.render
    with the Python layer's live state left in place (rendered hint, launch order hint, gradient scratch), deterministic backward.
      * Each iteration matches its own oracle, and grad(it 1) - grad(it 0) matches the oracle's difference (DIFF_TOL).
      * Iteration 1 is bit-identical to the same call made after a fresh state (caches cleared) was warmed up at iteration 1's OWN background: the two
        differ only in the background of the call before, so anything carried over from it shows.  (A cold call is no reference: without a launch
        order hint the hybrid forward splits every tile, and the deterministic sums follow the shapes.)
    28 x 28 tiles: the colour pass takes the hybrid kernels, the second call under the launch order the first call's backward left (meta[11]); the geo
    pass takes no order hint by default (rasterizer.ORDER_HINT_GEO)."""
    from ibgs_amd import renderer, simple_scene
    from tests.test_gpu_renderer import _oracle_inputs
    dev, g, pc, cams, scn = renderer_setup()
    pipe, args = simple_scene.default_pipe(), simple_scene.default_args()
    cam = cams[0]
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(7)
    bgs = [torch.rand(3, generator=gen) for _ in range(2)]          # train.py:248, once per iteration
    extra = {}
    if geo:
        with torch.no_grad():
            for j in cam.nearest_id:
                scn.rendered_depth_list[j] = renderer.render_depth(cams[j], pc, scn, pipe, args, torch.zeros(3, device=dev), True, 3, 4)
        chosen = cam.nearest_id[:3]
        r2s, scp = syn.ref_to_src({"viewmatrix": cam.world_view_transform.cpu().numpy()},
                                  [{"viewmatrix": cams[j].world_view_transform.cpu().numpy()} for j in chosen])
        extra = dict(render_geo=True, n_src=3, buffer_length=4, depth_thr=0.01, ref_to_src=r2s, src_cam_pos=scp,
                     src_images=scn.original_image_list[chosen].cpu().numpy(), src_depths=scn.rendered_depth_list[chosen].cpu().numpy())
    gc = rnd((3, H, W), 21); gn = GEO_UP * rnd((3, H, W), 22)

    def iteration(bg):
        for p in pc.parameters():
            p.grad = None
        out = renderer.render(cam, pc, scn, pipe, args, bg.to(dev), learnt_normal=True, nb_src_frames=3, buffer_length=4, render_geo=geo)
        o = {"color": out["render"]}
        meta = arena_words(o, {"W": W, "H": H}, "meta", 32)
        final_T = arena_words(o, {"W": W, "H": H}, "final_T", H * W).view(np.float32)
        loss = (out["render"] * torch.as_tensor(gc, device=dev)).sum()
        if geo:
            loss = loss + (out["rendered_normal"] * torch.as_tensor(gn, device=dev)).sum()
        loss.backward()
        torch.cuda.synchronize()
        return SimpleNamespace(img=out["render"].detach().cpu().numpy(), nrm=out["rendered_normal"].detach().cpu().numpy() if geo else None,
                               meta=meta, final_T=final_T, g={"means2D": out["viewspace_points"].grad.cpu().numpy(),
                                                              "means2D_abs": out["viewspace_points_abs"].grad.cpu().numpy(),
                                                              "opacity": pc._opacity.grad.cpu().numpy()})

    old = rasterizer.DETERMINISTIC
    try:
        rasterizer.DETERMINISTIC = True
        renderer.clear_caches()
        live = [iteration(b) for b in bgs]
        renderer.clear_caches()
        iteration(bgs[1])
        replay = iteration(bgs[1])
    finally:
        rasterizer.DETERMINISTIC = old
        renderer.clear_caches()
    if not geo:
        assert live[0].meta[11] == 0 and live[1].meta[11] == 1 and replay.meta[11] == 1, "the launch order hint was not taken"
    assert (live[0].final_T > 0.5).mean() >= 0.3, "the background has too little weight in this view"
    assert np.array_equal(live[1].img, replay.img)
    for k in live[1].g:
        assert np.array_equal(live[1].g[k], replay.g[k]), "%s of iteration 1 depends on the previous call's background" % k
    # each iteration against its own oracle; dL/dopacity through the activation (sigmoid) of the model's raw parameter
    am = syn.plane_all_map(g["means3D"], pc.get_scaling.detach().cpu().numpy(), pc.get_rotation.detach().cpu().numpy(),
                           {"viewmatrix": cam.world_view_transform.cpu().numpy(), "campos": cam.camera_center.cpu().numpy()},
                           normal=g["normal"], offset=g["offset"])
    want = []
    for it, (bg, h) in enumerate(zip(bgs, live)):
        inp = _oracle_inputs(g, pc, cam, am, dict(extra, bg=bg.numpy().astype(np.float32)))
        ref = oracle.forward(inp, cull=True)
        gb = oracle.backward(inp, ref, gc, gn if geo else None)
        assert l1(h.img, ref["color"]) < 1e-6, it
        if geo:
            assert l1(h.nrm, ref["normal_map"]) < 1e-5, it
        (gop,) = torch.autograd.grad(pc.get_opacity, pc._opacity, torch.as_tensor(gb["dL_dopacity"].reshape(-1, 1), device=dev))
        w = {"means2D": gb["dL_dmeans2D"].reshape(h.g["means2D"].shape), "means2D_abs": gb["dL_dmeans2D_abs"].reshape(h.g["means2D_abs"].shape),
             "opacity": gop.cpu().numpy()}
        e = {k: rel_l2(h.g[k], w[k]) for k in w}
        print("[bg] renderer geo=%s iteration %d, bg %s: relL2 %s" % (geo, it, np.round(bg.numpy(), 3), ", ".join("%s %.1e" % kv for kv in e.items())))
        assert max(e.values()) <= GRAD_TOL, (it, e)
        want.append(w)
    # the background differential between the two iterations; it must be large enough that a stale background fails the bars above as well
    for k in want[0]:
        a = live[1].g[k].astype(np.float64) - live[0].g[k]
        b = want[1][k].astype(np.float64) - want[0][k]
        share = np.linalg.norm(b) / np.linalg.norm(want[1][k])
        print("[bg] renderer geo=%s: %s differential relL2 %.1e (%.3f of the gradient)" % (geo, k, rel_l2(a, b), share))
        assert rel_l2(a, b) <= DIFF_TOL, k
        assert share >= 10 * GRAD_TOL, (k, share)
