"""The geo path at the trainer's validity: the multi-view-consistent surface scene (tests/scenes.surface_scene, depth_thr 0.01), where most covered pixels
see 3-5 valid sources -- slots 1-4 of cam_feat / warped_image / valid_idx / valid_w, the full list without a -1 terminator, the cumulative depth gradient
of the window pass over several sources (quirk Q2), texel clamps at frame borders, min_depth_diff far below 1 -- against the oracle AND against the
closed forms of tests/test_oracle_surface.py (ground pixels: ray/plane depth, ground normal, source ray cosines, linear source images).

(a) small frames, both wave shapes, five (n_src, L); (b) 1 M surface Gaussians at 1920 x 1080 through full_size_geo_parity; (c) the trainer's chain --
render_depth_batch fills the depth cache, render() reads it as a table with the fused plane map -- against the oracle pushed through the torch glue;
(d) the deterministic backward is bit-reproducible on (b)'s scene."""
import functools

import numpy as np
import pytest
import torch

import oracle
from ibgs_amd import _lib, rasterizer, renderer, simple_scene
from tests import hipref
from tests.metrics import l1, rel_l2
from tests.scenes import quat_z_to, surface_discs, surface_scene, valid_source_histogram
from tests.test_gpu_anisotropic import F64_K, f64_truth
from tests.test_gpu_fullsize_geo import full_size_geo_parity
from tests.test_gpu_parity import (GEO_GRAD_TOL, GRAD_PAIRS, canon_valid, check_color, check_stages, rnd, run,  # noqa: F401
                                   wave_shape)
from tests.test_oracle_surface import MIN_ALL_VALID_5, MIN_MEAN_VALID, closed_form_errors

pytestmark = pytest.mark.gpu
MAX_VIEWS = _lib.MAX_VIEWS

PLANE_TOL = (("normal_map", 1e-5), ("median_depth", 1e-5), ("warped_image", 1e-5), ("cam_feat", 1e-5), ("camera_ray", 1e-5), ("min_depth_diff", 1e-4))


def check_decisions(win_hip, same, win_tw, same_tw, label):
    """The decision-flip budgets of full_size_geo_parity: median-buffer windows and valid-source sets may differ from the oracle's on no more pixels than
    max(a floor, 3 x what the oracle's own fma-contracted build flips) -- windows 1e-5 of the pixels (none on a small frame), valid-source sets 1e-4 or
    2 pixels.  win_*: per-pixel window equality, same*: per-pixel valid-set equality, against the oracle proper."""
    n = same.size
    print("%s windows differ on %d px (fma twin %d), valid-source sets on %d px (fma twin %d) of %d"
          % (label, int((~win_hip).sum()), int((~win_tw).sum()), int((~same).sum()), int((~same_tw).sum()), n))
    assert (~win_hip).mean() <= max(1e-5, 3 * (~win_tw).mean()), "more window flips than the reference's own arithmetic leaves open"
    assert (~same).mean() <= max(1e-4, 3 * (~same_tw).mean()) or (~same).sum() <= max(2, 3 * int((~same_tw).sum())), \
        "more valid-source flips than the reference's own arithmetic leaves open"


def check_planes(o, ref, ok, label=""):
    """The seven geo planes on the pixels whose valid-source sets agree (a slot shifted by one source is a different quantity), mean-relative bars of
    full_size_geo_parity; the mask exactly."""
    H, W = ok.shape
    for k, tol in PLANE_TOL:
        a, b = np.asarray(o[k]).reshape(-1, H, W), np.asarray(ref[k]).reshape(-1, H, W)
        dd = np.abs(a - b)[:, ok]
        rel = dd.mean() / (np.abs(b[:, ok]).mean() + 1e-12)
        print("%s    %-14s mean |d| %.2e (rel %.2e) max %.2e" % (label, k, dd.mean(), rel, dd.max()))
        assert rel < tol, (k, rel)
    assert np.array_equal(np.asarray(o["use_first_src_frame_mask"]).reshape(H, W)[ok], np.asarray(ref["use_first_src_frame_mask"]).reshape(H, W)[ok])


def check_grads_arbitered(pairs, label=""):
    """pairs: [(name, HIP, oracle fp32, f64 thunk)] -- relative L2 <= GEO_GRAD_TOL, or within F64_K x the fp32 oracle's own distance from the float64 build."""
    failed = []
    for name, a, b, t64 in pairs:
        if np.abs(b).max() == 0:
            assert np.abs(a).max() == 0, name
            continue
        e32 = rel_l2(a, b)
        if e32 <= GEO_GRAD_TOL:
            print("%s    %-12s %.2e" % (label, name, e32))
            continue
        t = t64()
        e64, floor = rel_l2(a, t), rel_l2(b, t)
        print("%s    %-12s %.2e | vs f64 %.2e, oracle fp32 vs f64 %.2e  %s" % (label, name, e32, e64, floor, "ok by the arbiter" if e64 <= F64_K * floor else "FAIL"))
        if e64 > F64_K * floor:
            failed.append(name)
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------
# (a) small frames: every slot level and L, both wave shapes
def small_frame_geo_checks(inp, grads, label, regime=None):
    """One small geo frame through the product path, judged like test_surface_scene_small_frames: stages and colour, the decision budgets against the
    oracle's fma twin, sum_w, the seven planes and the per-source weights on the pixels whose valid sources agree, every gradient by the arbiter.
    regime(mean, hist): asserts the oracle's valid-source histogram before anything is compared.  Returns (ref, o, ist)."""
    H, W, n_src = inp["H"], inp["W"], inp["n_src"]
    ref, o, ist, leaves, gb = run(inp, grads)
    h_ref, m_ref = valid_source_histogram(ref["valid_src_idx"], ref["final_T"], n_src)
    h_hip, m_hip = valid_source_histogram(ist["valid_idx"], ist["final_T"], n_src)
    print("\n%s valid sources per covered pixel: oracle mean %.2f [%s], HIP mean %.2f [%s]" % (label, m_ref, " ".join("%.3f" % x for x in h_ref), m_hip,
                                                                                             " ".join("%.3f" % x for x in h_hip)))
    if regime is not None:
        regime(m_ref, h_ref)
    check_stages(ist, o, ref); check_color(o, ist, ref)
    with oracle.variant("fma"):
        tw = oracle.forward(inp, tex_quant=rasterizer.TEX_QUANT, cull=True)
    win = (ist["low_high"][:, 0] == ref["cache_low"]) & (ist["low_high"][:, 1] == ref["cache_high"])
    win_tw = (tw["cache_low"] == ref["cache_low"]) & (tw["cache_high"] == ref["cache_high"])
    same = np.all(canon_valid(ist["valid_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    same_tw = np.all(canon_valid(tw["valid_src_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    check_decisions(win, same, win_tw, same_tw, label)
    assert l1(ist["sum_w"], ref["cache_sum_w"]) < 1e-6
    ok = same.reshape(H, W)
    check_planes(o, ref, ok, label)
    # the per-source blend weights (valid_w) behind every written slot
    alive = canon_valid(ref["valid_src_idx"]) >= 0
    vw = np.abs(ist["valid_w"] - ref["valid_src_w"])[alive & same[None]]
    assert vw.max() < 1e-5, vw.max()
    f64 = functools.lru_cache(None)(lambda: f64_truth(inp, grads)[1])
    check_grads_arbitered([(lk, leaves[lk].grad.cpu().numpy(), gb[rk].reshape(leaves[lk].grad.shape), (lambda rk=rk, lk=lk: np.asarray(f64()[rk]).reshape(leaves[lk].grad.shape)))
                           for lk, rk in GRAD_PAIRS if leaves.get(lk) is not None], label)
    return ref, o, ist


@pytest.mark.parametrize("n_src,L", [(4, 4), (5, 8), (5, 1), (3, 5), (2, 2)])
def test_surface_scene_small_frames(n_src, L, wave_shape):
    inp = surface_scene(P=20000, W=176, H=112, seed=30 + 2 * n_src + L, n_src=n_src, L=L)
    H, W = inp["H"], inp["W"]
    grads = {"color": rnd((3, H, W), 7), "normal_map": rnd((3, H, W), 8), "median_depth": rnd((1, H, W), 9), "warped_image": rnd((15, H, W), 10)}

    def regime(m_ref, h_ref):
        assert m_ref >= min(MIN_MEAN_VALID, 0.75 * n_src) and (n_src != 5 or h_ref[5] >= MIN_ALL_VALID_5)
    small_frame_geo_checks(inp, grads, "[surface %s n_src %d L %d]" % (wave_shape, n_src, L), regime)


# ---------------------------------------------------------------------------------------------------
# (b) full size: 1 M surface Gaussians at 1920 x 1080
@functools.lru_cache(maxsize=1)
def full_inputs(n_src, L):
    return surface_scene(P=10 ** 6, W=1920, H=1080, seed=100 + n_src, n_src=n_src, L=L, images="linear")


@pytest.mark.parametrize("n_src,L,wave_shape", [(4, 4, "tile"), (5, 8, "quadrant")], indirect=["wave_shape"])          # (each case once: both shapes, half the time)
def test_surface_scene_full_size(n_src, L, wave_shape):
    inp = full_inputs(n_src, L)

    def closed_forms(o, ist, say):
        return closed_form_errors(inp, o, ist["valid_idx"], ist["final_T"], rasterizer.TEX_QUANT, say=say)
    full_size_geo_parity("surface_n%d_L%d" % (n_src, L), inp, min_mean_valid=MIN_MEAN_VALID, min_all_valid=MIN_ALL_VALID_5 if n_src == 5 else None,
                         extra_checks=closed_forms)


# (d) the deterministic backward on the full-size scene: two runs, the same bits
@pytest.mark.parametrize("wave_shape", ["tile"], indirect=True)
def test_surface_scene_deterministic_backward_is_bit_identical(wave_shape):
    inp = full_inputs(5, 8)
    H, W = inp["H"], inp["W"]
    r_ = np.random.default_rng(11)
    g = {"color": r_.standard_normal((3, H, W)), "normal_map": r_.standard_normal((3, H, W)), "median_depth": r_.standard_normal((1, H, W)),
         "warped_image": r_.standard_normal((15, H, W))}
    old = rasterizer.DETERMINISTIC
    rasterizer.DETERMINISTIC = True
    try:
        res = []
        for _ in range(2):
            outs, lv, _ = hipref.run_forward(inp)
            sum((outs[k] * torch.as_tensor(v, device="cuda", dtype=torch.float32)).sum() for k, v in g.items()).backward()
            torch.cuda.synchronize()
            res.append({k: v.grad.cpu().numpy() for k, v in lv.items() if v is not None and v.grad is not None})
            del outs, lv
    finally:
        rasterizer.DETERMINISTIC = old
    assert set(res[0]) == set(res[1]) and "all_map" in res[0]
    for k in res[0]:
        assert np.abs(res[0][k]).max() > 0 or k in ("means2D", "means2D_abs", "colors_precomp", "cov3D_precomp"), k
        assert np.array_equal(res[0][k].view(np.uint32), res[1][k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------
# (c) the trainer's chain: depth cache from render_depth_batch, read as a table by render() with the fused plane map
def _chain_setup(P=20000, W=176, H=112, seed=41, n_views=36):
    dev = torch.device("cuda")
    g = surface_discs(P, seed, deg=2)
    g = {k: g[k] for k in ("means3D", "shs", "scales", "rotations", "opacities", "normal", "offset")}      # learnt normal = the surface normal, offset 0
    # The orbit cameras circle the z axis at one elevation, and a horizontal ground and a sphere on that axis look the same from every one of them:
    # the depth planes of all views would then be one image and a source reading another view's plane would go unnoticed (measured: 5 % of the covered
    # pixels change their valid sources).  Tilted by 20 degrees and moved off the axis, the scene makes every plane its own view's (96 %).
    a = np.radians(20.0)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    g["means3D"] = (g["means3D"] @ rot.T + np.array([0.4, -0.3, 0.0])).astype(np.float32)
    g["normal"] = (g["normal"] @ rot.T).astype(np.float32)
    g["rotations"] = quat_z_to(g["normal"]).astype(np.float32)
    cams = simple_scene.orbit_cameras(W, H, n_views=n_views, device=dev, nearest=3)        # 10 degrees apart: the nearest three within 20 (at 15 the mean falls to 2.4 valid of 3)
    imgs = torch.rand(n_views, 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    scene = simple_scene.SimpleScene(cams, images=imgs, device=dev)
    pipe, args = simple_scene.default_pipe(), simple_scene.default_args()
    bg = torch.tensor([0.1, 0.1, 0.2], device=dev)
    pc0 = simple_scene.SimpleGaussians(g, sh_degree=2, device=dev)
    with torch.no_grad():
        # (one batched pass holds at most MAX_VIEWS views: the cache is filled batch by batch, as a trainer refreshing it would)
        scene.rendered_depth_list = torch.cat([renderer.render_depth_batch(cams[i:i + MAX_VIEWS], pc0, scene, pipe, args, bg, True, 3, 4)
                                               for i in range(0, n_views, MAX_VIEWS)])
    return dev, g, cams, scene, pipe, args, bg


def _f64_chain(chain, g, dev, cams, scene, bg, planes):
    """the raw-parameter gradients of the oracle chain with the float64 build of the oracle (the glue stays in float32 torch)"""
    with oracle.variant("f64"):
        return chain(True, g, dev, cams, scene, bg, planes=planes)[1]


def test_surface_scene_trainer_chain():
    from tests.test_gpu_fused_planes import _oracle_chain as chain
    from ibgs_amd import synthetic as syn
    dev, g, cams, scene, pipe, args, bg = _chain_setup()
    cam = cams[0]
    H, W = cam.image_height, cam.image_width
    table = scene.rendered_depth_list
    assert torch.is_tensor(table) and table.is_cuda and table.is_contiguous() and renderer.DEPTH_TABLE and renderer.FUSED_PLANE_MAP
    # 1. the batched depth-only pass of every view this frame reads (and the frame's own) against the oracle's depth-only render of that camera
    for j in [0] + list(cam.nearest_id):
        cj = cams[j]
        camd = {"viewmatrix": cj.world_view_transform.cpu().numpy(), "campos": cj.camera_center.cpu().numpy()}
        inp = {k: g[k] for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        inp.update(all_map=syn.plane_all_map(g["means3D"], g["scales"], g["rotations"], camd, normal=g["normal"], offset=g["offset"]), W=W, H=H,
                   tanfovx=np.tan(cj.FoVx * 0.5), tanfovy=np.tan(cj.FoVy * 0.5), viewmatrix=camd["viewmatrix"], projmatrix=cj.full_proj_transform.cpu().numpy(),
                   campos=camd["campos"], bg=bg.cpu().numpy(), sh_degree=2, render_depth_only=True, buffer_length=4)
        ref_d = oracle.forward(inp)["median_depth"]
        d = np.abs(table[j].cpu().numpy() - ref_d)
        print("\n[chain] depth cache plane %d vs the oracle: mean rel %.2e, px off by > 1e-3 rel: %d" % (j, d.mean() / np.abs(ref_d).mean(), int((d > 1e-3 * (1 + np.abs(ref_d))).sum())))
        # (test_gpu_depth_batch's bars: a pixel whose median window flips on a rounded T costs its whole depth difference)
        assert d.mean() / (np.abs(ref_d).mean() + 1e-9) < 1e-4 and (d > 1e-3 * (1 + np.abs(ref_d))).mean() < 2e-3, j
    # 2. render() with the table and the fused planes, every output and every raw-parameter gradient against the oracle through the torch glue
    pc = simple_scene.SimpleGaussians(g, sh_degree=2, device=dev)
    out = renderer.render(cam, pc, scene, pipe, args, bg, learnt_normal=True, nb_src_frames=3, buffer_length=4, render_geo=True, return_depth_normal=False)
    ist = hipref.internal_state({"color": out["render"]}, {"means3D": g["means3D"], "W": W, "H": H})
    rec = ist["rec"]
    planes = {"all_map": np.concatenate([rec[:, 12:15], np.ones((rec.shape[0], 1), np.float32), rec[:, 7:8]], axis=1),
              "have": out["radii"].detach().cpu().numpy() > 0}          # the plane map the kernels built (test_gpu_fused_planes._run)
    gen = torch.Generator(device=dev).manual_seed(3)                    # _oracle_chain draws the same upstream gradients in this order
    up = [torch.randn(c, H, W, device=dev, generator=gen) for c in (3, 3, 1, 15)]
    loss = sum((out[k] * u).sum() for k, u in zip(("render", "rendered_normal", "median_intersected_depth", "warped_image"), up))
    loss.backward()
    torch.cuda.synchronize()
    names = ("_xyz", "_normal", "_offset", "_rotation", "_scaling", "_opacity", "_features_dc")
    g_hip = {n: getattr(pc, n).grad.detach().cpu().numpy() for n in names}
    ref, g_orc = chain(True, g, dev, cams, scene, bg, planes=planes)
    h_ref, m_ref = valid_source_histogram(ref["valid_src_idx"], ref["final_T"], 3)
    h_hip, m_hip = valid_source_histogram(ist["valid_idx"], ist["final_T"], 3)
    print("[chain] valid sources per covered pixel: oracle mean %.2f [%s], HIP mean %.2f [%s]" % (m_ref, " ".join("%.3f" % x for x in h_ref), m_hip,
                                                                                                 " ".join("%.3f" % x for x in h_hip)))
    assert m_ref >= MIN_MEAN_VALID and h_ref[3] > 0.5
    o = {"color": out["render"], "normal_map": out["rendered_normal"], "median_depth": out["median_intersected_depth"], "cam_feat": out["cam_feat"],
         "warped_image": out["warped_image"], "min_depth_diff": out["min_depth_diff"], "camera_ray": out["camera_ray"],
         "use_first_src_frame_mask": out["use_first_src_frame_mask"]}
    o = {k: v.detach().cpu().numpy() for k, v in o.items()}
    assert l1(o["color"], ref["color"]) < 1e-6 and np.array_equal(out["radii"].cpu().numpy(), ref["radii"])
    assert l1(ist["final_T"], ref["final_T"]) < 1e-6
    win = (ist["low_high"][:, 0] == ref["cache_low"]) & (ist["low_high"][:, 1] == ref["cache_high"])
    same = np.all(canon_valid(ist["valid_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    with oracle.variant("fma"):          # the oracle's fma twin on the same inputs, for the decision budgets
        tw, _ = chain(True, g, dev, cams, scene, bg, planes=planes)
    win_tw = (tw["cache_low"] == ref["cache_low"]) & (tw["cache_high"] == ref["cache_high"])
    same_tw = np.all(canon_valid(tw["valid_src_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    check_decisions(win, same, win_tw, same_tw, "[chain]")
    check_planes(o, ref, same.reshape(H, W), "[chain]")
    f64 = functools.lru_cache(None)(lambda: _f64_chain(chain, g, dev, cams, scene, bg, planes))
    check_grads_arbitered([(n, g_hip[n], g_orc[n], (lambda n=n: f64()[n])) for n in names], "[chain]")
    # 3. the comparison can see a wrong plane: the sources reading each other's depth planes lose most of their valid sources
    real = renderer.GaussianRasterizationSettings
    try:
        renderer.GaussianRasterizationSettings = lambda **kw: real(**dict(kw, src_depth_slots=tuple(kw["src_depth_slots"][1:] + kw["src_depth_slots"][:1])))
        oc = renderer.render(cam, simple_scene.SimpleGaussians(g, sh_degree=2, device=dev), scene, pipe, args, bg, learnt_normal=True, nb_src_frames=3,
                             buffer_length=4, render_geo=True, return_depth_normal=False)
        ist_c = hipref.internal_state({"color": oc["render"]}, {"means3D": g["means3D"], "W": W, "H": H})
    finally:
        renderer.GaussianRasterizationSettings = real
    cov = ist["final_T"] < 0.5
    moved = ~np.all(canon_valid(ist_c["valid_idx"]) == canon_valid(ist["valid_idx"]), axis=0)
    print("[chain] swapped depth planes change the valid-source sets on %.3f of the covered pixels" % moved[cov].mean())
    assert moved[cov].mean() > 0.5
