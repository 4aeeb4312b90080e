"""Generates tests/golden/consumer_resized.npz IN THE BUILD CONTAINER, where the reference is present (as make_consumer_fixture.py does): the `oracle_*`
tensors already in consumer.npz (48 x 32, 3 levels) are fed to the reference's own `fuse_color` (color_aggregation_network.py:156-250, imported read-only
through _ref_import's path) with `residual_resolution_scale` = 0.5, 0.75 and 1.5 and one seeded `ColorFusionResidualNet(height=int(H s), width=int(W s))`
on the CPU in float32 -- the parameters do not depend on the size, so every scale runs the same state dict.  Recorded:

  * s = 0.5, plain ("half_") and with exposure correction ("half_exposure_"): the three tensors `fuse_color` handed to the network (forward pre-hook:
    x_views (Hr Wr, levels, 7), ray_dir (Hr Wr, 3), c_3dgs (Hr Wr, 3)), `residual`, `image_pred` (3, H, W) and the level count;
  * s = 0.75 ("three_quarters_") and 1.5 ("three_halves_"), plain: `residual` and `image_pred`;
  * the seed and the state dict under the reference's keys ("sd/per_view_mlp.0.weight", "sd/conv_decoder.enc1.0.weight", ...).

The fixture is data only; nothing of the reference is copied.  Re-run:  python tests/golden/make_consumer_resized_fixture.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import as ri  # noqa: E402

sys.path.insert(0, ri.REF)
from color_aggregation_network import ColorFusionResidualNet, fuse_color  # noqa: E402

SEED = 4
src = np.load(os.path.join(HERE, "consumer.npz"))
H, W = int(src["H"]), int(src["W"])
pkg = {name: torch.tensor(src["oracle_" + key]) for name, key in (("render", "color"), ("cam_feat", "cam_feat"), ("warped_image", "warped_image"),
                                                                  ("min_depth_diff", "min_depth_diff"), ("camera_ray", "camera_ray"),
                                                                  ("use_first_src_frame_mask", "use_first_src_frame_mask"))}
torch.manual_seed(SEED)
net = ColorFusionResidualNet(height=H, width=W)
seen = {}
net.register_forward_pre_hook(lambda m, args: seen.update(x_views=args[0].detach().clone(), ray_dir=args[1].detach().clone(), c_3dgs=args[2].detach().clone()))
out = {"H": H, "W": W, "seed": np.int32(SEED), "scales": np.float64([0.5, 0.75, 1.5])}
for tag, s, expo, hooked in (("half", 0.5, False, True), ("half_exposure", 0.5, True, True), ("three_quarters", 0.75, False, False), ("three_halves", 1.5, False, False)):
    net.height, net.width = int(H * s), int(W * s)
    assert net.height % 4 == 0 and net.width % 4 == 0
    opts = types.SimpleNamespace(enable_exposure_correction=expo, nb_visible_src_frames=3, residual_resolution_scale=s)
    with torch.no_grad():
        r = fuse_color(pkg, net, None, None, None, 0, opts)
    assert r is not None and torch.isfinite(r["image_pred"]).all() and tuple(r["residual"].shape) == (3, H, W) and r["burned_in_gauss"] == 1.0
    assert tuple(seen["x_views"].shape) == (net.height * net.width, 3, 7)
    out[tag + "_residual"], out[tag + "_image_pred"] = r["residual"].numpy(), r["image_pred"].numpy()
    out[tag + "_size"] = np.int32([net.height, net.width])
    if hooked:
        out[tag + "_levels"] = np.int32(r["nb_valid_warp_level"])
        for k in ("x_views", "ray_dir", "c_3dgs"):
            out[tag + "_" + k] = seen[k].numpy()
for k, v in net.state_dict().items():
    out["sd/" + k] = v.numpy()
path = os.path.join(HERE, "consumer_resized.npz")
np.savez_compressed(path, **out)
print("consumer_resized.npz written:", len(out), "arrays,", os.path.getsize(path), "bytes; levels", int(out["half_levels"]), int(out["half_exposure_levels"]))
assert os.path.getsize(path) < 414000          # below the larger golden files already here (the state dict is 264 kB of it)
