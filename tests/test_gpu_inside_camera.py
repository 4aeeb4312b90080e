"""The rasterizer from cameras INSIDE the scene and with fx != fy, through the product path (run on the MI355X box: pytest -m gpu).

Every other camera of the suite stands outside the cloud with fx == fy (synthetic.make_camera), where an fx in the place of an fy -- in the EWA Jacobian
and its backward, the pixel ray and the source reprojection of the geo kernels and their gradients -- changes nothing, and where no Gaussian is
near-culled, lies behind the camera or covers the frame many times over.  (Planted one at a time in the library: fx for fy in preprocess_bwd's dty, in
render_fwd's reprojection of the median point and in render_bwd's warp derivative each pass the colour, geo, ragged-frame, culling, depth-batch and
small-frame surface tests of the rest of the suite and fail this file.)  The
scenes, their regime and the proof that the references alone meet every bar used here are in tests/test_oracle_inside_camera.py (no GPU); the judges and
their bars are those of tests/test_gpu_parity.py, test_gpu_anisotropic.py, test_gpu_surface_geo.py and test_gpu_depth_batch.py, unchanged.  No number in this
file comes from the HIP path."""
import numpy as np
import pytest
import torch

import oracle
from ibgs_amd import rasterizer
from tests import hipref
from tests.metrics import l1
from tests.test_gpu_anisotropic import check_color_aniso, check_grads_aniso, f64_truth, fixed_summation_order, fma_twin
from tests.test_gpu_parity import (GEO_GRAD_TOL, GRAD_PAIRS, canon_valid, check_color, check_grads, check_stages, run,  # noqa: F401
                                   wave_shape)
from tests.test_gpu_surface_geo import check_decisions, small_frame_geo_checks
from tests.test_oracle_inside_camera import (FOCAL_RATIOS, cloud, depth_bars, depth_batch_gaussians, depth_batch_views, depth_only_input, low_surface, mdd_bar,
                                             plane_inside, upstream)
from tests.test_oracle_surface import MIN_MEAN_VALID, closed_form_errors

pytestmark = pytest.mark.gpu


def sh_colours_only_where_used(ist, ref):
    """SH -> RGB runs for the Gaussians that reach a tile list: colours and clamp flags bit-identical there, zero elsewhere (test_colour_path_forward_backward)"""
    cb = (ref["clamped"][:, 0] | (ref["clamped"][:, 1] << 1) | (ref["clamped"][:, 2] << 2)).astype(np.uint8)
    used = ref["tiles_touched"] > 0
    assert used.sum() > 100
    assert np.array_equal(ist["clamped"][used], cb[used]) and not ist["clamped"][~used].any()
    assert np.array_equal(ist["rec"][used, 8:11].view(np.uint32), ref["rgb"][used].view(np.uint32)) and not ist["rec"][~used, 8:11].any()


def culled_gaussians_get_nothing(ref, o, ist, leaves):
    """every Gaussian the oracle culls (radius 0: behind the camera, inside the near plane, or an empty footprint) has radius 0, no tile and an exactly zero
    row in every gradient"""
    gone = ref["radii"] == 0
    assert gone.sum() > 1500
    assert not o["radii"][gone].any() and not ist["tiles"][gone].any()
    for lk, _ in GRAD_PAIRS:
        if leaves.get(lk) is not None:
            g = leaves[lk].grad
            assert g is not None and not g.cpu().numpy()[gone].any(), lk


# (a) the colour path from inside, tile-aligned and ragged frame
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_colour_path_from_inside(name):
    inp = cloud(name)
    ref, o, ist, leaves, gb = run(inp, upstream(inp))
    check_stages(ist, o, ref); check_color(o, ist, ref)
    sh_colours_only_where_used(ist, ref)
    check_grads(leaves, gb)
    culled_gaussians_get_nothing(ref, o, ist, leaves)
    for k in ("normal_map", "median_depth", "cam_feat", "warped_image", "min_depth_diff", "camera_ray", "use_first_src_frame_mask"):
        assert o[k].shape == ref[k].shape and not o[k].any()


# (b) the three footprint classes of the tile cull and the tall-rectangle walk, populated from one inside scene
@pytest.mark.parametrize("name,cull", [("wide", True), ("wide", False), ("wide_big", True)])
def test_footprint_classes_from_inside(name, cull):
    inp = cloud(name)
    ref, o, ist, leaves, gb = run(inp, upstream(inp), cull=cull)
    check_stages(ist, o, ref); check_color(o, ist, ref); check_grads(leaves, gb)
    r = ref["rect4"].astype(np.int64)
    h = r[:, 3] - r[:, 1]
    area = (r[:, 2] - r[:, 0]) * h
    for label, m in (("at most 64 tiles", (area > 0) & (area <= 64)), ("65 .. 256 tiles", (area > 64) & (area <= 256)), ("more than 256 tiles", area > 256),
                     ("taller than 16 tile rows", h > 16)):
        assert m.sum() > 25, (label, m.sum())
        assert np.array_equal(ist["tiles"][m], ref["tiles_touched"][m]), label
    if not cull:          # the reference's bounding-box lists: every tile of every rectangle
        assert np.array_equal(ref["tiles_touched"], area.astype(np.uint32)) and ist["R"] == area.sum()


# (c) the geo path on the multi-view-consistent scene from a low camera, both focal ratios
@pytest.mark.parametrize("fovx,fovy", FOCAL_RATIOS)
def test_geo_path_from_a_low_camera(fovx, fovy, wave_shape):
    inp = low_surface(fovx, fovy)

    def regime(m_ref, h_ref):
        assert m_ref >= MIN_MEAN_VALID and h_ref[4] > 0.33

    label = "[low %s fov %g / %g]" % (wave_shape, fovx, fovy)
    ref, o, ist = small_frame_geo_checks(inp, upstream(inp), label, regime)
    # ... and against the closed forms of the ground plane (ray/plane depth, camera ray, ground normal, source ray cosines, linear source images), which an
    # fx / fy exchange fails by 0.15 .. 0.4 (tests/test_oracle_inside_camera.py); the min_depth_diff row at twice the float64 oracle's own figure
    fails = closed_form_errors(inp, o, ist["valid_idx"], ist["final_T"], rasterizer.TEX_QUANT, mdd_bar=mdd_bar(fovx, fovy))
    assert not fails, fails


# (d) plane-like Gaussians from inside: the arbiter
def test_geo_path_on_plane_like_gaussians_from_inside(wave_shape):
    inp = plane_inside()
    H, W = inp["H"], inp["W"]
    grads = upstream(inp)
    with fixed_summation_order(True):
        ref, o, ist, leaves, gb = run(inp, grads)
    twin, _ = fma_twin(inp, grads)
    r64, g64 = f64_truth(inp, grads)
    check_stages(ist, o, ref); check_color_aniso(o, ist, ref, twin, r64)
    assert (ref["valid_src_idx"][0] >= 0).mean() > 0.3, "scene does not exercise the warp path"
    win = (ist["low_high"][:, 0] == ref["cache_low"]) & (ist["low_high"][:, 1] == ref["cache_high"])
    win_tw = (twin["cache_low"] == ref["cache_low"]) & (twin["cache_high"] == ref["cache_high"])
    same = np.all(canon_valid(ist["valid_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    same_tw = np.all(canon_valid(twin["valid_src_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    check_decisions(win, same, win_tw, same_tw, "[plane inside %s]" % wave_shape)
    assert l1(o["normal_map"], ref["normal_map"]) < 1e-6
    ok = same.reshape(H, W)
    for k, tol in (("median_depth", 1e-4), ("cam_feat", 1e-5), ("warped_image", 1e-5), ("min_depth_diff", 1e-5), ("camera_ray", 1e-5)):          # test_geo_path_on_plane_like_gaussians' bars
        d = np.abs(o[k] - ref[k])[:, ok]
        assert d.mean() / (np.abs(ref[k][:, ok]).mean() + 1e-9) < tol, k
    assert np.array_equal(o["use_first_src_frame_mask"][0][ok], ref["use_first_src_frame_mask"][0][ok])
    check_grads_aniso(leaves, gb, g64, base_tol=GEO_GRAD_TOL)


# (e) one batched depth pass over views that differ in pose and in both fields of view
def test_depth_batch_with_views_that_differ():
    from ibgs_amd.rasterizer import rasterize_depth_batch
    dev = torch.device("cuda")
    cams = depth_batch_views()
    g = depth_batch_gaussians()
    W, H, P = cams[0]["W"], cams[0]["H"], g["means3D"].shape[0]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    m, op, sc, rot = t(g["means3D"]), t(g["opacities"]), t(g["scales"]), t(g["rotations"])

    def depth_pass(views):
        return rasterize_depth_batch(m, op, sc, rot, None, 1.0, torch.stack([t(c["viewmatrix"]) for c in views]), torch.stack([t(c["projmatrix"]) for c in views]),
                                     torch.stack([t(c["campos"]) for c in views]), [c["tanfovx"] for c in views], [c["tanfovy"] for c in views], H, W, 4, plane_mode=2)

    depths, radii = depth_pass(cams)
    assert depths.shape == (4, 1, H, W) and radii.shape == (4, P)
    for v, c in enumerate(cams):
        d1, r1 = depth_pass([c])
        assert torch.equal(depths[v], d1[0]) and torch.equal(radii[v], r1[0]), v          # bit-identical to the view's own pass
        ref = oracle.forward(depth_only_input(c))
        assert np.array_equal(radii[v].cpu().numpy(), ref["radii"]), v
        rel, off = depth_bars(depths[v].cpu().numpy(), ref["median_depth"])
        print("\n[depth batch view %d] mean rel %.2e, px off by > 1e-3 rel: %.2e" % (v, rel, off))
        assert rel < 1e-4 and off < 2e-3, v
    assert not torch.equal(depths[0], depths[3])          # (the same pose: only the fields of view tell these two apart)


# (f) mark_visible with most of the cloud behind the near plane
def test_mark_visible_from_inside():
    inp = cloud("small")
    st = hipref.settings_from(inp, "cuda")
    vis = rasterizer.GaussianRasterizer(st).markVisible(torch.as_tensor(inp["means3D"], device="cuda")).cpu().numpy()
    want = oracle.mark_visible(inp["means3D"], inp["viewmatrix"])
    assert want.sum() > 560 and (~want).sum() > 900
    assert vis.dtype == np.bool_ and np.array_equal(vis, want)
