"""scale_modifier != 1 through the whole operator: the same checks and bars as tests/test_gpu_parity.py::test_colour_path_forward_backward (both wave shapes),
plus the proof that the setting arrived -- the radii differ from the modifier-1.0 run on most visible Gaussians."""
import numpy as np
import pytest

import oracle
from tests.scenes import scene
from tests.test_gpu_parity import check_color, check_grads, check_stages, rnd, run, wave_shape  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mod", [0.7, 1.6])
def test_colour_path_with_a_scale_modifier(mod):
    inp = scene(P=3000, deg=1, seed=43, opacity="trained")
    unit = oracle.forward(inp, cull=True)
    inp["scale_modifier"] = mod
    ref, o, ist, leaves, gb = run(inp, {"color": rnd((3, inp["H"], inp["W"]), 1)})
    vis = (ref["radii"] > 0) | (unit["radii"] > 0)
    assert vis.sum() > 1000 and (ref["radii"][vis] != unit["radii"][vis]).sum() > 0.5 * vis.sum(), "the modifier did not reach the forward"
    check_stages(ist, o, ref)
    check_color(o, ist, ref)
    cb = (ref["clamped"][:, 0] | (ref["clamped"][:, 1] << 1) | (ref["clamped"][:, 2] << 2)).astype(np.uint8)
    used = ref["tiles_touched"] > 0
    assert used.sum() > 100
    assert np.array_equal(ist["clamped"][used], cb[used]) and not ist["clamped"][~used].any()
    assert np.array_equal(ist["rec"][used, 8:11].view(np.uint32), ref["rgb"][used].view(np.uint32)) and not ist["rec"][~used, 8:11].any()
    check_grads(leaves, gb)
    for k in ("normal_map", "median_depth", "cam_feat", "warped_image", "min_depth_diff", "camera_ray", "use_first_src_frame_mask"):
        assert o[k].shape == ref[k].shape and not o[k].any()
