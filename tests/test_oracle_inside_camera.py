"""Cameras INSIDE the scene and unequal focal lengths (fx != fy): the inputs of tests/test_gpu_inside_camera.py, checked here without a GPU.

Every other camera of the suite is synthetic.make_camera's: outside the cloud (radius 4 against a half-extent of 1.3), fovy derived from fovx's focal length
(fx == fy), fovx 0.6911.  An fx written where fy belongs is invisible there (tanfovx and tanfovy do differ wherever W != H, so the clamp limits are
told apart; the focal lengths of the Jacobian, of the pixel ray and of the source reprojection are not), and no Gaussian is near-culled, lies behind the
camera or has a footprint many times the frame.  The scenes below (tests/scenes.camera_at, inside_cloud, surface_scene with poses) leave both habits.

(a) REGIME: the counts that make these scenes what they are, asserted on the fp32 oracle at about half of what the committed builders give (the measured
    values are in each test's docstring), so that an edited seed cannot silently leave the regime.
(b) CLOSED FORMS hold for the oracle on the surface scene seen from a low camera, at both focal ratios, with and without the texture unit's weight rounding.
(c) THE REFERENCES ALONE MEET THE GPU BARS: the oracle's fma-contracted build judged against the oracle proper passes the equalities of check_stages, the
    colour bars of check_color and the decision budgets; the fp32 gradients lie within GRAD_TOL / GEO_GRAD_TOL of the float64 build.  A bar that the
    reference's own arithmetic cannot keep would test the oracle's build flags.
(d) TEETH: the oracle run with tanfovx and tanfovy exchanged fails the closed forms of median_depth, camera_ray and the warped colours.

THE min_depth_diff BAR OF THE LOW CAMERAS.  min_depth_diff is min over the valid sources of |d_src(u, v) - z_src| / z_src, where z_src is the depth of the
pixel's surface point in the source frame and d_src(u, v) the source's depth map read at the point's projection.  The oracle reads that map as the reference's
texture unit does (ibgs_oracle.c tex_1: the four texels around (u, v), bilinear weights), so even where both views see the same plane exactly the figure is the
error of interpolating the map LINEARLY between texel centres.  Along a plane the depth is z = c / (a u + b v + d): convex in (u, v), its chords lie above it
by up to z'' / 8 per texel squared, i.e. a relative error of (z' / z)^2 / 4 with z' / z the relative depth step from one texel to the next.  From the
outside camera (ground 3 .. 5 units away, seen from 20 degrees above) that step is below 1 %: 2e-5, closed_form_errors' default bar.  From 0.30 above the ground, looking
along it, the step reaches 3 .. 7 % per texel row (more with fy = 91 than with fy = 142): (0.045)^2 / 4 = 5e-4 and (0.07)^2 / 4 = 1.2e-3.
test_min_depth_diff_is_the_interpolation_error_of_a_convex_depth_map confirms this reading: a bilinear read of the EXACT plane depths at the source's texel
centres reproduces the figure.  The bar for these two cameras is F64_K = 2 times what the float64 build of the oracle gives on the same input (nothing in it
comes from the HIP path):

    fovx / fovy    fp32 oracle    float64 build    bar (2 x float64)
    1.25 / 0.75    4.976e-4       4.977e-4         9.954e-4
    0.8  / 1.1     1.319e-3       1.320e-3         2.639e-3

The agreement of the HIP path with the oracle on that plane stays with check_planes' 1e-4."""
import functools
import math

import numpy as np
import pytest

import oracle
from ibgs_amd import synthetic as syn
from tests.metrics import l1, psnr, rel_l2
from tests.scenes import GROUND_Z, add_sources, camera_at, inside_cloud, surface_scene, valid_source_histogram
from tests.test_oracle_surface import MIN_MEAN_VALID, closed_form_errors, surface_truth

F64_K = 2.0                   # tests/test_gpu_anisotropic.F64_K
GRAD_TOL = 1e-3               # tests/test_gpu_parity.GRAD_TOL and GEO_GRAD_TOL
L1_TOL = 1e-4                 # tests/test_gpu_parity.L1_TOL

# ---- the scenes (shared with tests/test_gpu_inside_camera.py; built once, never written to) -------------------------------------------------------------
EYE_A, TARGET_A = (0.3, -0.2, 0.1), (1.0, 0.6, 0.0)               # inside the cloud (half-extent 1.3), looking at a point inside it
EYE_B, TARGET_B = (-0.4, 0.5, -0.3), (0.9, -0.6, 0.2)
GZ = float(GROUND_Z)
LOW_EYE, LOW_TARGET = (1.45, 0.35, GZ + 0.30), (-0.6, -0.5, GZ + 0.05)          # 0.30 above the ground square, looking along it past the sphere
SRC_OFFSETS = ((0.06, 0.10, 0.0), (-0.05, -0.10, 0.03), (0.0, 0.15, 0.05), (0.08, -0.12, -0.04))
FOCAL_RATIOS = ((1.25, 0.75), (0.8, 1.1))                          # (fovx, fovy) of the surface cases: fx / fy = 122 / 142 and 208 / 91

CLOUDS = {
    # name: (P, W, H, eye, target, fovx, fovy, opacity, scale_mul)
    "small": (3000, 176, 112, EYE_A, TARGET_A, 1.2, 0.7, "trained", 1.0),
    "ragged": (3000, 197, 131, EYE_A, TARGET_A, 1.3, 0.8, "trained", 1.0),
    "wide": (3000, 400, 304, EYE_A, TARGET_A, 1.3, 0.8, "trained", 1.0),
    "wide_big": (1500, 400, 304, EYE_B, TARGET_B, 0.8, 1.2, "init", 2.0),
}


@functools.lru_cache(None)
def cloud(name):
    P, W, H, eye, target, fovx, fovy, opacity, scale_mul = CLOUDS[name]
    return inside_cloud(P, W, H, eye, target, fovx, fovy, seed=3, deg=3, opacity=opacity, scale_mul=scale_mul)


def _offset(eye, d):
    return tuple(float(e + x) for e, x in zip(eye, d))


@functools.lru_cache(None)
def low_surface(fovx, fovy):
    return surface_scene(P=20000, W=176, H=112, seed=7, L=4, images="linear", ref_pose=(LOW_EYE, LOW_TARGET),
                         src_poses=[(_offset(LOW_EYE, d), LOW_TARGET) for d in SRC_OFFSETS], fovx=fovx, fovy=fovy)


@functools.lru_cache(None)
def plane_inside():
    """Plane-like Gaussians (one axis 1e-2 .. 1e-3 of the others) around the camera, geo inputs from three sources placed like low_surface's first three at a
    quarter of the distance: what this camera sees is 0.2 .. 1 away, not 1 .. 3, and at the full offsets the parallax leaves a valid source on 6 % of the
    pixels (at a quarter: on 65 %, with every count 0 .. 3 on more than a tenth of them).  depth_thr 0.05 as on the other random clouds."""
    W, H, fovx, fovy = 176, 112, 0.9, 1.1
    base = inside_cloud(3000, W, H, EYE_A, TARGET_A, fovx, fovy, seed=3, deg=2, opacity="trained", anisotropy="plane", planes=True)
    return add_sources(base, L=4, srcs=[camera_at(W, H, _offset(EYE_A, tuple(0.25 * x for x in d)), TARGET_A, fovx, fovy) for d in SRC_OFFSETS[:3]])


@functools.lru_cache(None)
def depth_batch_views():
    """Four views of one size that differ in everything a batched depth pass takes per view, all of low_surface's discs (depth_batch_gaussians): the suite's
    outside camera; the inside camera of the "small" cloud, which here stands inside the sphere; low_surface's low camera (fovx 1.25 / fovy 0.75); the
    outside camera's pose with fovx 0.8 / fovy 1.1."""
    W, H = 176, 112
    el = math.radians(20.0)
    eye_out = (4.0 * math.cos(el), 0.0, 4.0 * math.sin(el))                                  # make_camera's default eye
    return (syn.make_camera(W, H), cloud("small")["_cam"], camera_at(W, H, LOW_EYE, LOW_TARGET, 1.25, 0.75), camera_at(W, H, eye_out, (0.0, 0.0, 0.0), 0.8, 1.1))


def depth_batch_gaussians():
    """The Gaussians of the batched depth pass: low_surface's 20 000 discs.  NOT a random cloud: there the plane of a Gaussian is its smallest axis, a random
    direction, and in every view a few pixels' rays run within rounding of parallel to a plane they blend -- ray/plane depths of 1e3 .. 2e4 that move by
    per cents when the plane map moves by one float32 rounding, which the mean-relative bar of tests/test_gpu_depth_batch.py then measures instead of the
    pass (on the "small" cloud: 3e-4 .. 9e-4 from +-1 ulp on the oracle's own plane map, against a bar of 1e-4; the library builds its plane map in the
    kernel, a few roundings away from numpy's).  The discs face their surfaces: the same perturbation moves these views by 1e-6 (test_regime_depth_batch_views)."""
    return low_surface(*FOCAL_RATIOS[0])["_g"]


def depth_only_input(cam, L=4):
    """the oracle's depth-only input of depth_batch_gaussians for one camera (numpy plane map of the smallest axis)"""
    g = depth_batch_gaussians()
    inp = {k: g[k] for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    inp.update(all_map=syn.plane_all_map(g["means3D"], g["scales"], g["rotations"], cam), W=cam["W"], H=cam["H"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
               viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"], bg=np.zeros(3, np.float32), sh_degree=2,
               render_depth_only=True, buffer_length=L)
    return inp


def moved_by_ulps(a, k, seed):
    """every element of the float32 array moved by a random whole number of roundings in -k .. k"""
    r = np.random.default_rng(seed).integers(-k, k + 1, size=a.shape)
    out = a.copy()
    for s in range(1, k + 1):
        out = np.where(r >= s, np.nextafter(out, np.float32(np.inf)), out)
        out = np.where(r <= -s, np.nextafter(out, np.float32(-np.inf)), out)
    return out.astype(np.float32)


def depth_bars(d, ref):
    """tests/test_gpu_depth_batch's bars of one depth map against the oracle's: (mean relative error < 1e-4, share of pixels off by more than 1e-3 relative < 2e-3)"""
    e = np.abs(np.asarray(d, np.float64) - ref)
    return e.mean() / (np.abs(ref).mean() + 1e-9), (e > 1e-3 * (1 + np.abs(ref))).mean()


def rnd(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def upstream(inp):
    """the upstream gradients of one case: colour alone, or every differentiable geo output (tests/test_gpu_parity's seeds)"""
    H, W = inp["H"], inp["W"]
    if not inp["render_geo"]:
        return {"color": rnd((3, H, W), 1)}
    return {"color": rnd((3, H, W), 7), "normal_map": rnd((3, H, W), 8), "median_depth": rnd((1, H, W), 9), "warped_image": rnd((15, H, W), 10)}


def canon_valid(v):
    """valid_src_indices is only defined up to its -1 terminator (tests/test_gpu_parity.canon_valid)"""
    return np.where(np.cumprod(v != -1, axis=0) > 0, v, -1)


def oracle_run(inp, build="plain", backward=True):
    """forward (culled lists) and backward of one build of the oracle"""
    g = upstream(inp)
    with oracle.variant(build):
        r = oracle.forward(inp, cull=True)
        gb = oracle.backward(inp, r, g["color"], g.get("normal_map"), g.get("median_depth"), g.get("warped_image")) if backward else None
    return r, gb


_cached_run = functools.lru_cache(None)(lambda kind, key, build: oracle_run({"cloud": cloud, "low": lambda k: low_surface(*k), "plane": lambda k: plane_inside()}[kind](key), build))

ALL_SCENES = [("cloud", n) for n in CLOUDS] + [("low", fr) for fr in FOCAL_RATIOS] + [("plane", None)]


def scene_of(kind, key):
    return cloud(key) if kind == "cloud" else low_surface(*key) if kind == "low" else plane_inside()


# ---- (a) regime ------------------------------------------------------------------------------------------------------------------------------------------
def camera_frame(inp):
    """positions in the camera frame (float64 on the float32 inputs) and the two fields' 1.3 tan clamp"""
    vm = np.asarray(inp["viewmatrix"], np.float64).reshape(4, 4)
    m = np.asarray(inp["means3D"], np.float64)
    t = m @ vm[:3, :3] + vm[3, :3]
    z = t[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        clamp = (np.abs(t[:, 0] / z) > 1.3 * float(inp["tanfovx"])) | (np.abs(t[:, 1] / z) > 1.3 * float(inp["tanfovy"]))
    return t, clamp


def cloud_regime(inp, out):
    """the counts of the issue's table for one cloud scene"""
    W, H = inp["W"], inp["H"]
    t, clamp = camera_frame(inp)
    z = t[:, 2]
    vis = out["radii"] > 0
    m2 = out["means2D"]
    off = (m2[:, 0] < 0) | (m2[:, 0] > W) | (m2[:, 1] < 0) | (m2[:, 1] > H)
    r = out["rect4"].astype(np.int64)
    w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    area = w * h
    return {"near": int((z <= 0.2).sum()), "behind": int((z < 0).sum()), "visible": int(vis.sum()), "clamped": int((clamp & vis).sum()),
            "off_frame": int((off & vis).sum()), "min_z": float(z[vis].min()), "max_radius": int(out["radii"].max()),
            "max_tiles": int(out["tiles_touched"].max()), "tiles": ((W + 15) // 16) * ((H + 15) // 16),
            "small": int(((area > 0) & (area <= 64)).sum()), "mid": int(((area > 64) & (area <= 256)).sum()), "large": int((area > 256).sum()),
            "tall": int((h > 16).sum()), "R": int(out["num_rendered"])}


def test_regime_small_cloud():
    """176 x 112, 3 000 Gaussians, eye (0.3, -0.2, 0.1) -> (1.0, 0.6, 0), fovx 1.2 / fovy 0.7 (fx 128.6, fy 153.4).  Measured: 1 878 of the 3 000 fail z > 0.2 (1 554 lie behind
    the camera), 495 are visible down to z = 0.2025, 288 of those beyond the 1.3 tan clamp and 342 with their centre off the frame; the largest radius is 440 px
    and the largest footprint all 77 tiles."""
    inp = cloud("small")
    n = cloud_regime(inp, _cached_run("cloud", "small", "plain")[0])
    print("\n[regime small]", n)
    assert abs(inp["W"] / (2 * inp["tanfovx"]) - inp["H"] / (2 * inp["tanfovy"])) > 20          # fx != fy
    assert n["near"] > 900 and n["behind"] > 750 and n["visible"] > 250 and n["clamped"] > 65 and n["off_frame"] > 100
    assert n["min_z"] < 0.25 and n["max_radius"] > 220 and n["max_tiles"] == n["tiles"]


def test_regime_ragged_cloud():
    """197 x 131 (no multiple of the tile in either direction), the same pose, fovx 1.3 / fovy 0.8.  Measured: 571 visible, 319 of them beyond
    the clamp, 61 rectangles of 65 .. 256 tiles, the largest footprint all 117 tiles."""
    n = cloud_regime(cloud("ragged"), _cached_run("cloud", "ragged", "plain")[0])
    print("\n[regime ragged]", n)
    assert n["visible"] > 280 and n["mid"] > 30 and n["clamped"] > 65 and n["max_tiles"] == n["tiles"]


@pytest.mark.parametrize("name", ["wide", "wide_big"])
def test_regime_footprint_classes(name):
    """400 x 304 = 25 x 19 tiles: all three footprint classes of the tile cull and the tall-rectangle walk from one scene.  Measured (wide / wide_big):
    rectangles of at most 64 tiles 171 / 80, of 65 .. 256 tiles 255 / 449, of more than 256 tiles 59 / 405, taller than 16 tile rows 103 / 290; visible beyond the
    clamp 289 / 613, visible with the centre off the frame 361 / 720, largest radius 1 057 / 3 825 px; culled lists of 52 187 / 197 957 entries against
    94 368 / 390 725 of the reference's bounding boxes."""
    inp = cloud(name)
    out = _cached_run("cloud", name, "plain")[0]
    n = cloud_regime(inp, out)
    full = oracle.forward(inp, cull=False)
    print("\n[regime %s]" % name, n, "AABB lists", full["num_rendered"])
    floors = {"wide": dict(small=85, mid=125, large=30, tall=50, clamped=145, off_frame=180, max_radius=1000),
              "wide_big": dict(small=40, mid=225, large=200, tall=145, clamped=100, off_frame=100, max_radius=1900)}[name]
    for k, v in floors.items():
        assert n[k] > v, (k, n[k], v)
    assert 0.3 * full["num_rendered"] < n["R"] < 0.7 * full["num_rendered"]          # the per-tile test removes about half the reference's list entries
    for k in ("color", "radii", "final_T"):
        assert np.array_equal(out[k], full[k]), k


def surface_regime(inp, out):
    t, _ = camera_frame(inp)
    hist, mean = valid_source_histogram(out["valid_src_idx"], out["final_T"], inp["n_src"])
    return {"near": int((t[:, 2] <= 0.2).sum()), "behind": int((t[:, 2] < 0).sum()), "visible": int((out["radii"] > 0).sum()),
            "covered": float((out["final_T"] < 0.5).mean()), "mean_valid": mean, "all_valid": float(hist[-1]),
            "mask": surface_truth(inp)["pix"].size / float(inp["W"] * inp["H"]), "fx": inp["W"] / (2 * inp["tanfovx"]), "fy": inp["H"] / (2 * inp["tanfovy"])}


@pytest.mark.parametrize("fovx,fovy", FOCAL_RATIOS)
def test_regime_low_surface(fovx, fovy):
    """The multi-view-consistent discs (20 000, 176 x 112) from 0.30 above the ground with four sources within 0.16 of the reference eye.  Measured
    (fovx 1.25 / fovy 0.75, then 0.8 / 1.1): fx / fy 122.0 / 142.3 and 208.1 / 91.3; 919 Gaussians fail the near cull, 500 lie behind; 3.66 and 3.47 valid
    sources per covered pixel, all four valid on 0.754 and 0.671 of them; the closed forms' ground mask holds 34.7 % and 37.5 % of the frame."""
    inp = low_surface(fovx, fovy)
    n = surface_regime(inp, _cached_run("low", (fovx, fovy), "plain")[0])
    print("\n[regime low %g / %g]" % (fovx, fovy), n)
    assert inp["n_src"] == 4 and len(inp["_srcs"]) == 4
    assert abs(n["fx"] - n["fy"]) > 15
    assert n["mean_valid"] >= MIN_MEAN_VALID and n["all_valid"] > 0.33
    assert n["mask"] > 0.10
    assert n["near"] > 200 and n["behind"] > 100          # (the eye stands on the ground square: discs around and behind it)


def test_regime_plane_like_cloud():
    """Plane-like Gaussians from inside, fovx 0.9 / fovy 1.1, three sources.  Measured: 1 878 near-culled, 800 visible (516 beyond the clamp, 603 centres off
    the frame), largest radius 747 px, aspect^2 > 25 on 0.071 of the visible footprints; the first slot is valid on 0.649 of the pixels, 0 / 1 / 2 / 3 valid
    sources on 0.351 / 0.267 / 0.253 / 0.129 of them."""
    inp = plane_inside()
    out = _cached_run("plane", None, "plain")[0]
    n = cloud_regime(inp, out)
    co = out["conic_opacity"][out["radii"] > 0]
    aspect2 = (co[:, 0] * co[:, 2]) / np.maximum(co[:, 0] * co[:, 2] - co[:, 1] ** 2, 1e-30)
    warp = float((out["valid_src_idx"][0] >= 0).mean())
    hist, mean = valid_source_histogram(out["valid_src_idx"], out["final_T"], 3)
    print("\n[regime plane]", n, "aspect^2 > 25 on %.3f of the visible, first slot valid on %.3f of the pixels, share at 0..3 valid sources %s" % (
        (aspect2 > 25).mean(), warp, np.round(hist, 3)))
    assert n["near"] > 900 and n["visible"] > 400 and n["clamped"] > 250 and n["max_radius"] > 370
    assert (aspect2 > 25.0).mean() > 0.03 and warp > 0.3 and hist.min() > 0.06


def test_regime_depth_batch_views_and_mark_visible():
    """The four views of the batched depth pass: the same frame size, four different (tanfovx, tanfovy) pairs, three poses; the inside and the low view cull
    Gaussians at the near plane, the outside views none.  Measured (visible / near-culled per view): 16 503 / 0, 992 / 12 264, 11 146 / 919, 19 709 / 0.  The input is WELL CONDITIONED under
    test_gpu_depth_batch's bars (see depth_batch_gaussians): the float64 build of the oracle, and the oracle on a plane map moved by up to 4 roundings per
    component, both stay within a tenth of them -- measured: mean relative difference at most 3.9e-6, no pixel off by 1e-3.
    mark_visible from the inside camera of the "small" cloud: 1 122 visible, 1 878 not."""
    cams = depth_batch_views()
    assert np.array_equal(cams[3]["viewmatrix"], cams[0]["viewmatrix"]) and not np.array_equal(cams[3]["projmatrix"], cams[0]["projmatrix"])
    assert len({(round(c["tanfovx"], 6), round(c["tanfovy"], 6)) for c in cams}) == 4
    vis, near, cond = [], [], []
    for v, c in enumerate(cams):
        inp = depth_only_input(c)
        out = oracle.forward(inp)
        t, _ = camera_frame(inp)
        vis.append(int((out["radii"] > 0).sum())); near.append(int((t[:, 2] <= 0.2).sum()))
        assert (out["median_depth"] > 0).mean() > 0.4
        with oracle.variant("f64"):
            r64 = oracle.forward(inp)
        moved = oracle.forward(dict(inp, all_map=moved_by_ulps(inp["all_map"], 4, seed=5)))
        for other in (r64, moved):
            rel, off = depth_bars(other["median_depth"], out["median_depth"])
            cond.append(rel)
            assert rel < 1e-5 and off < 2e-4, (v, rel, off)
    print("\n[regime views] visible %s, near-culled %s, float64 build / plane map moved by 4 ulp: mean rel at most %.1e" % (vis, near, max(cond)))
    assert min(vis) > 450 and near[0] == near[3] == 0 and near[1] > 6000 and near[2] > 450 and vis[3] != vis[0]
    inp = cloud("small")
    mv = oracle.mark_visible(inp["means3D"], inp["viewmatrix"])
    print("[regime mark_visible] %d visible, %d not" % (mv.sum(), (~mv).sum()))
    assert mv.sum() > 560 and (~mv).sum() > 900


# ---- (b) closed forms on the low camera -------------------------------------------------------------------------------------------------------------------
def _mdd_row(inp, out):
    """the figure of closed_form_errors' `min_depth_diff max (>= 1 valid source)` row"""
    fig = {}
    closed_form_errors(inp, out, out["valid_src_idx"], out["final_T"], tex_quant=False, say=lambda s: None, mdd_bar=np.inf, figures=fig)
    return fig["min_depth_diff max (>= 1 valid source)"][0]


@functools.lru_cache(None)
def mdd_bar(fovx, fovy):
    """F64_K x the float64 oracle's own min_depth_diff on the ground pixels of this camera (see the module docstring)"""
    inp = low_surface(fovx, fovy)
    r64 = _cached_run("low", (fovx, fovy), "f64")[0]
    return F64_K * _mdd_row(inp, r64)


@pytest.mark.parametrize("fovx,fovy", FOCAL_RATIOS)
def test_closed_forms_hold_for_the_oracle_from_a_low_camera(fovx, fovy):
    inp = low_surface(fovx, fovy)
    out = _cached_run("low", (fovx, fovy), "plain")[0]
    bar = mdd_bar(fovx, fovy)
    print("\n[low %g / %g] min_depth_diff on the ground: fp32 oracle %.3e, float64 build %.3e, bar %.3e" % (fovx, fovy, _mdd_row(inp, out), bar / F64_K, bar))
    assert 2e-5 < bar < 5e-3          # well above the outside camera's 2e-5 and still well below depth_thr
    fails = closed_form_errors(inp, out, out["valid_src_idx"], out["final_T"], tex_quant=False, mdd_bar=bar)
    assert not fails, fails
    q = oracle.forward(inp, tex_quant=True, cull=True)
    fails = closed_form_errors(inp, q, q["valid_src_idx"], q["final_T"], tex_quant=True, mdd_bar=bar)
    assert not fails, fails


@pytest.mark.parametrize("fovx,fovy", FOCAL_RATIOS)
def test_min_depth_diff_is_the_interpolation_error_of_a_convex_depth_map(fovx, fovy):
    """The cause of the low cameras' large min_depth_diff, from first principles: put the EXACT depth of the ground plane at every texel centre of a source's
    map, read it bilinearly at the closed-form projection of each ground pixel and compare with the point's exact source depth.  The largest relative error
    over the clear ground pixels reproduces the oracle's figure (same pixels, the minimum over the valid sources) within 10 %; the map's curvature, not
    the rasterizer, makes it."""
    inp = low_surface(fovx, fovy)
    out = _cached_run("low", (fovx, fovy), "f64")[0]
    W, H = inp["W"], inp["H"]
    tr = surface_truth(inp)
    fx, fy = W / (2.0 * float(inp["tanfovx"])), H / (2.0 * float(inp["tanfovy"]))
    keep = np.asarray(out["final_T"]).reshape(-1)[tr["pix"]] < 0.5
    ok = tr["clear"].all(0) & keep & tr["valid"].any(0)
    X = tr["campos"] + tr["depth"][:, None] * (tr["ray"] / (tr["ray"] @ np.asarray(inp["viewmatrix"], np.float64).reshape(4, 4)[:3, 2])[:, None])
    err = np.full((inp["n_src"], tr["pix"].size), np.inf)
    py, px = np.mgrid[0:H, 0:W]
    for si, s in enumerate(inp["_srcs"]):
        ws = np.asarray(s["viewmatrix"], np.float64).reshape(4, 4).T
        Rs, Cs = ws[:3, :3], np.linalg.inv(ws)[:3, 3]
        d = np.stack([(px - 0.5 * W) / fx, (py - 0.5 * H) / fy, np.ones((H, W))], -1) @ Rs          # world directions of the source's texel centres
        with np.errstate(divide="ignore"):
            zmap = (GZ - Cs[2]) / d[..., 2]                                                          # exact plane depth per texel
        u, v = tr["u"][si], tr["v"][si]
        i0 = np.clip(np.floor(u).astype(int), 0, W - 2); j0 = np.clip(np.floor(v).astype(int), 0, H - 2)
        a, b = u - i0, v - j0
        read = (1 - a) * (1 - b) * zmap[j0, i0] + a * (1 - b) * zmap[j0, i0 + 1] + (1 - a) * b * zmap[j0 + 1, i0] + a * b * zmap[j0 + 1, i0 + 1]
        zs = (X - Cs) @ Rs[2]
        e = np.abs(read - zs) / zs
        err[si, tr["valid"][si]] = e[tr["valid"][si]]
    model = float(err.min(0)[ok].max())
    got = _mdd_row(inp, out)
    print("\n[low %g / %g] min_depth_diff max: float64 oracle %.3e, bilinear read of the exact plane depths %.3e" % (fovx, fovy, got, model))
    assert abs(got - model) <= 0.1 * model


# ---- (c) the references alone meet the GPU bars -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,key", ALL_SCENES, ids=lambda v: str(v))
def test_the_fma_build_passes_the_gpu_bars_against_the_oracle_proper(kind, key):
    """check_stages' equalities, check_color's bars and check_decisions' floors with the oracle's fma-contracted build in the place of the HIP path.  Worst
    measured over the scenes: lists identical everywhere; n_contrib differs on at most 5.1e-5 of the pixels (bar 2e-4); colour mean L1 at most 2.5e-7 (bar 1e-6),
    largest single-pixel difference 2.5e-3 on the low camera at 0.8 / 1.1 (bar 5e-3: one pair on either side of the alpha = 1 / 255 skip); no window and no
    valid-source set flips."""
    inp = scene_of(kind, key)
    ref, tw = _cached_run(kind, key, "plain")[0], _cached_run(kind, key, "fma")[0]
    for k in ("radii", "tiles_touched", "point_list", "ranges"):
        assert np.array_equal(tw[k], ref[k]), k
    assert tw["num_rendered"] == ref["num_rendered"]
    d = np.abs(tw["color"] - ref["color"])
    bad = float((tw["n_contrib"] != ref["n_contrib"]).mean())
    print("\n[fma twin %s %s] colour mean L1 %.2e max %.2e, n_contrib differs on %.2e of the pixels, final_T L1 %.2e" % (kind, key, d.mean(), d.max(), bad, l1(tw["final_T"], ref["final_T"])))
    assert l1(tw["color"], ref["color"]) <= L1_TOL * 1e-2 and float(d.max()) < 5e-3          # check_color
    assert bad <= 2e-4
    assert l1(tw["final_T"], ref["final_T"]) < 1e-6
    tgt = np.random.default_rng(0).uniform(0, 1, ref["color"].shape)
    assert abs(psnr(tw["color"], tgt)[0] - psnr(ref["color"], tgt)[0]) <= 0.05
    if inp["render_geo"]:                                                                  # check_decisions' floors
        win = (tw["cache_low"] == ref["cache_low"]) & (tw["cache_high"] == ref["cache_high"])
        same = np.all(canon_valid(tw["valid_src_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
        print("    windows differ on %d px, valid-source sets on %d px" % ((~win).sum(), (~same).sum()))
        assert (~win).mean() <= 1e-5 and ((~same).mean() <= 1e-4 or (~same).sum() <= 2)


def test_the_fma_build_passes_the_depth_batch_bars_against_the_oracle_proper():
    """test_gpu_depth_batch's bars with the fma build in the place of the batched pass.  Worst over the four views: mean relative difference 1.0e-6 (bar 1e-4), no
    pixel off by 1e-3 relative (bar 2e-3 of them), radii identical."""
    for v, c in enumerate(depth_batch_views()):
        inp = depth_only_input(c)
        ref = oracle.forward(inp)
        with oracle.variant("fma"):
            tw = oracle.forward(inp)
        rel, off = depth_bars(tw["median_depth"], ref["median_depth"])
        print("\n[fma twin depth view %d] mean rel %.2e, px off by > 1e-3 rel: %.2e" % (v, rel, off))
        assert np.array_equal(tw["radii"], ref["radii"]) and rel < 1e-4 and off < 2e-3, v


GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dmeans2D_abs", "dL_dsh", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dall_map")


@pytest.mark.parametrize("kind,key", [s for s in ALL_SCENES if s[0] != "plane"], ids=lambda v: str(v))
def test_the_fp32_gradients_lie_within_the_gpu_bar_of_the_float64_build(kind, key):
    """relative L2 of every gradient of the fp32 oracle against the float64 build <= GRAD_TOL (the plane-like scene is judged by the arbiter on the GPU, as
    tests/test_gpu_anisotropic.py judges its kind).  Worst measured: 2.4e-4 (dL/dscales, low camera at 1.25 / 0.75); the clouds stay below 1.8e-4."""
    g32, g64 = _cached_run(kind, key, "plain")[1], _cached_run(kind, key, "f64")[1]
    worst = {}
    for k in GRADS:
        if np.abs(g64[k]).max() == 0:
            assert np.abs(g32[k]).max() == 0, k
            continue
        worst[k] = rel_l2(g32[k], g64[k])
    print("\n[fp32 vs float64 %s %s] " % (kind, key) + ", ".join("%s %.1e" % kv for kv in worst.items()))
    assert max(worst.values()) <= GRAD_TOL, worst


# ---- (d) teeth --------------------------------------------------------------------------------------------------------------------------------------------
W_ROW = "warped_image (linear sources) max |d|"
V_ROW = "valid-source sets (pixels that differ, clear px)"


@pytest.mark.parametrize("fovx,fovy", FOCAL_RATIOS)
def test_closed_forms_see_exchanged_fields_of_view(fovx, fovy):
    """The oracle fed tanfovx <-> tanfovy (projmatrix kept: the front end still places every Gaussian right; the pixel rays, the ray/plane depths and the
    source reprojection use the wrong focal lengths) must fail the closed forms of the true camera.  On the equal-focal scenes of the rest of the suite this
    exchange changes nothing at all.

    Run as it stands, the exchange fails median_depth (0.39 / 0.35 relative), camera_ray (0.25 / 0.15) and the valid-source sets -- on EVERY clear pixel: the
    depths are so wrong that no source passes depth_thr 0.01.  The per-slot rows (cam_feat, warped colours) are judged where the valid sources match the
    closed form, which is then nowhere, and a row judged on no pixel reports 0: the warped colours' row says nothing about this exchange.  That is a
    property of the check, and it is resolved here rather than waived: a second run opens the depth test (depth_thr 10: a source is valid wherever the point
    projects into its frame and its depth map is not empty), so that the sets agree with the closed form wherever the sphere hides nothing and the wrong
    projection stays inside the frame.  There the warped colours are judged on thousands of slots and fail; with the true fields of view the same
    opened run passes that row, so the failure is the exchange's."""
    inp = low_surface(fovx, fovy)
    bar = mdd_bar(fovx, fovy)
    swap = lambda d: dict(d, tanfovx=d["tanfovy"], tanfovy=d["tanfovx"])
    rows, fig = [], {}
    out = oracle.forward(swap(inp), cull=True)
    fails = closed_form_errors(inp, out, out["valid_src_idx"], out["final_T"], tex_quant=False, say=rows.append, mdd_bar=bar, figures=fig)
    print("\n[exchanged %g / %g]" % (fovx, fovy)); print("\n".join(rows))
    for name in ("median_depth max rel", "camera_ray max |d|", V_ROW):
        assert name in fails, (name, fails)
    assert fig["median_depth max rel"][0] > 0.1 and fig["camera_ray max |d|"][0] > 0.05
    opened = dict(inp, depth_thr=10.0)
    rows, fig = [], {}
    out = oracle.forward(swap(opened), cull=True)
    fails = closed_form_errors(opened, out, out["valid_src_idx"], out["final_T"], tex_quant=False, say=rows.append, mdd_bar=bar, figures=fig)
    print("[exchanged %g / %g, depth test opened]" % (fovx, fovy)); print("\n".join(rows))
    assert W_ROW in fails and fig[W_ROW][2] > 1000 and fig[W_ROW][0] > 1e-2, fig[W_ROW]
    rows, fig = [], {}
    out = oracle.forward(opened, cull=True)
    fails = closed_form_errors(opened, out, out["valid_src_idx"], out["final_T"], tex_quant=False, say=rows.append, mdd_bar=bar, figures=fig)
    print("[true fields of view, depth test opened]"); print("\n".join(rows))
    assert W_ROW not in fails and fig[W_ROW][2] > 1000, fig[W_ROW]
    assert "median_depth max rel" not in fails and "camera_ray max |d|" not in fails
