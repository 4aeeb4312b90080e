"""The HIP kernels against the RECORDED OUTPUT OF THE REFERENCE'S OWN CODE (tests/golden/reference_<case>.npz, written by
tests/golden/make_reference_fixtures.py from the reference's CUDA sources compiled for the CPU).  Only the committed fixtures are read.

Each case regenerates its inputs (tests/reference_cases.FIXTURES), checks their checksum against the fixture's, runs the HIP forward and backward through
tests/hipref.py and holds the results to the bars the suite applies against the oracle:
* on the reference's AABB lists (rasterizer.TILE_CULL = False, as tests/test_gpu_parity.py's cull=False) radii, tiles touched, clamp flags, the sorted lists, the
  tile ranges and the preprocess record are exact; with the default culled lists the public outputs and gradients must meet the same bars;
* colour mean L1 <= 1e-4; the geo planes by test_gpu_parity's bars on the pixels whose decisions agree;
* decisions (n_contrib, the median contributors, the valid-source sets) may differ on at most as many pixels as the fixture records between the reference's
  plain and fma builds, plus one;
* gradients: relative L2 <= 1e-3 against the reference's; an array of the per-Gaussian chain that misses it is ill-conditioned if the reference itself is
  further than that from float64, and is then held to the arbiter's rule with the fixture's float64 column: |HIP - f64| <= F64_K x |reference - f64|."""
import os

import numpy as np
import pytest
import torch

from ibgs_amd import rasterizer
from tests import hipref
from tests import reference_cases as rc
from tests.metrics import l1, rel_l2

pytestmark = pytest.mark.gpu

F64_K = 2.0
GRAD_TOL = 1e-3
L1_TOL = 1e-4
GRAD_PAIRS = [("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("means2D_abs", "dL_dmeans2D_abs"), ("shs", "dL_dsh"), ("colors_precomp", "dL_dcolors"),
              ("opacities", "dL_dopacity"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"), ("cov3D_precomp", "dL_dcov3D"), ("all_map", "dL_dall_map")]


def _terminated(v):
    v = np.asarray(v).reshape(5, -1).copy()
    v[np.cumsum(v == -1, axis=0) > 0] = -1
    return v


@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("name", list(rc.FIXTURES))
def test_hip_against_the_references_recorded_output(name, cull):
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_%s.npz" % name))
    inp, g, q = rc.fixture_case(name)
    assert (int(fx["scene_seed"]), int(fx["upstream_seed"])) == (rc.FIXTURES[name]["scene_seed"], rc.FIXTURES[name]["upstream_seed"])
    assert rc.checksum(inp, g) == str(fx["checksum"]), "the regenerated inputs are not the ones the fixture was recorded on"
    assert bool(fx["tex_quant"]) == q
    geo = bool(inp.get("render_geo")); n = int(inp["n_src"]) if geo else 0
    H, W = int(inp["H"]), int(inp["W"]); HW = H * W
    for k, v in g.items():
        assert np.array_equal((v[:3 * n] if k == "warped_image" else v), fx["g_" + k].astype(np.float32)), k
    old = (rasterizer.TILE_CULL, rasterizer.TEX_QUANT)
    try:
        rasterizer.TILE_CULL, rasterizer.TEX_QUANT = cull, q
        outs, leaves, _ = hipref.run_forward(inp, debug=True)
        ist = hipref.internal_state(outs, inp)
        o = hipref.to_np(outs)
        loss = 0
        for k, v in g.items():
            loss = loss + (outs[k] * torch.as_tensor(v, device="cuda")).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        rasterizer.TILE_CULL, rasterizer.TEX_QUANT = old

    # ---- integer state and the preprocess record
    assert np.array_equal(o["radii"], fx["radii"])
    vis = fx["radii"] > 0
    for a, b in ((ist["depths"], fx["depths"]), (ist["rec"][:, 0:2], fx["means2D"]), (ist["rec"][:, 4:7], fx["conic_opacity"][:, :3]),
                 (ist["rec"][:, 2], fx["conic_opacity"][:, 3]), (ist["cov3D"], fx["cov3D"])):
        if name == "precomp" and a is ist["cov3D"]:
            continue          # cov3D is an input there; the reference leaves its own array unwritten
        assert np.array_equal(np.ascontiguousarray(a[vis]).view(np.uint32), np.ascontiguousarray(b[vis]).view(np.uint32)), "preprocess record not bit-identical"
    if inp.get("shs") is not None:
        c = fx["clamped"].astype(np.uint8)
        used = ist["tiles"] > 0          # a Gaussian whose every tile was culled gets no colour and no flags (tests/test_gpu_bwd_rows.py); none on the reference's lists
        assert cull or np.array_equal(used, vis)
        assert np.array_equal(ist["clamped"][used], (c[:, 0] | (c[:, 1] << 1) | (c[:, 2] << 2))[used]) and not ist["clamped"][~used].any()
    if not cull:          # the reference's own lists
        assert np.array_equal(ist["tiles"], fx["tiles_touched"])
        assert ist["R"] == int(fx["num_rendered"])
        assert np.array_equal(ist["ranges"], fx["ranges"])
        assert np.array_equal(ist["point_list"], fx["point_list"])
        assert np.array_equal(ist["sorted_tile_keys"], fx["tile_keys"])
    else:
        assert ist["R"] <= int(fx["num_rendered"])

    # ---- decisions: flips capped by the reference's own plain-versus-fma count, plus one
    same = np.ones(HW, bool)
    if not cull:          # (culled lists are shorter: contributor numbers are positions in another list)
        flips = ist["n_contrib"] != fx["n_contrib"]
        print("\n[%s cull=%s] n_contrib flips %d (reference plain vs fma: %d)" % (name, cull, int(flips.sum()), int(fx["flips_n_contrib"])))
        assert flips.sum() <= int(fx["flips_n_contrib"]) + 1
        same &= ~flips
        if geo:
            mflips = (ist["low_high"][:, 0] != fx["cache_low"]) | (ist["low_high"][:, 1] != fx["cache_high"])
            print("[%s] median-contributor flips %d (reference: %d)" % (name, int(mflips.sum()), int(fx["flips_median"])))
            assert mflips.sum() <= int(fx["flips_median"]) + 1
            same &= ~mflips
    if geo:
        vflips = (_terminated(ist["valid_idx"]) != fx["valid_src_idx"].astype(np.int32)).any(axis=0)
        print("[%s cull=%s] valid-source flips %d (reference plain vs fma: %d)" % (name, cull, int(vflips.sum()), int(fx["flips_valid"])))
        assert vflips.sum() <= int(fx["flips_valid"]) + 1
        same &= ~vflips
        assert (fx["valid_src_idx"][0] >= 0).mean() > 0.2, "the case does not exercise the warp path"

    # ---- public outputs
    d = l1(o["color"], fx["color"])
    print("[%s cull=%s] colour mean L1 %.3e" % (name, cull, d))
    assert d <= L1_TOL
    assert l1(ist["final_T"], fx["final_T"]) < 1e-6
    if geo:
        ok = same.reshape(H, W)
        assert l1(o["normal_map"], fx["normal_map"]) < 1e-6
        assert l1(ist["sum_w"][same], fx["cache_sum_w"][same]) < 1e-6
        live = {"cam_feat": 4 * n, "warped_image": 3 * n}
        for k, tol in (("median_depth", 1e-4), ("cam_feat", 1e-5), ("warped_image", 1e-5), ("min_depth_diff", 1e-5), ("camera_ray", 1e-5)):
            a = o[k][:live.get(k, o[k].shape[0])]
            e = np.abs(a - fx[k])[:, ok].mean() / (np.abs(fx[k][:, ok]).mean() + 1e-9)
            print("[%s cull=%s] %s mean rel err %.3e" % (name, cull, k, e))
            assert e < tol, (k, e)
            assert not o[k][live.get(k, o[k].shape[0]):].any(), k + ": a slot beyond the sources was written"
        assert np.array_equal(o["use_first_src_frame_mask"][0][ok], fx["use_first_src_frame_mask"][0][ok].astype(np.int32))

    # ---- the ten gradients
    if not same.all():          # a flipped pixel's upstream gradient reaches other Gaussians: the arrays are compared as they are, the bars absorb <= 2 pixels
        print("[%s cull=%s] %d pixels with flipped decisions stay in the gradient comparison" % (name, cull, int((~same).sum())))
    for lk, rk in GRAD_PAIRS:
        if leaves.get(lk) is None:
            continue
        a = leaves[lk].grad.cpu().numpy()
        if rk not in fx.files:          # all zero in the reference (not recorded)
            assert not np.abs(a).any(), lk
            continue
        b = fx[rk].reshape(a.shape)
        e = rel_l2(a, b)
        text = "[%s cull=%s] %-16s relL2 vs reference %.3e (d_order %.2e)" % (name, cull, rk, e, float(fx["d_order_" + rk]))
        if e > GRAD_TOL and ("f64_" + rk) in fx.files and float(fx["f64_dist_" + rk]) > GRAD_TOL:
            e64 = rel_l2(a, fx["f64_" + rk].reshape(a.shape).astype(np.float64))
            print(text + "  ill-conditioned: vs float64 %.3e, reference vs float64 %.3e" % (e64, float(fx["f64_dist_" + rk])))
            assert e64 <= F64_K * float(fx["f64_dist_" + rk]), (rk, e64)
            continue
        print(text)
        assert e <= GRAD_TOL, (rk, e)
