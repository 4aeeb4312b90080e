"""Generates tests/golden/hourglass.npz IN THE BUILD CONTAINER, where the reference is present (as make_coloragg_fixture.py does): a seeded
`ColorFusionResidualNet(height=16, width=24)` of the reference (color_aggregation_network.py, imported read-only through _ref_import's path) runs on the CPU
through the reference's own `fuse_color` on the 16 x 24 window of consumer.npz that coloragg.npz holds.  Recorded:

  * the network's full state dict, under the reference's keys ("sd/per_view_mlp.0.weight", "sd/conv_decoder.enc1.0.weight", ...);
  * the (1, 38, 16, 24) tensor `conv_decoder` received (forward pre-hook) and the (B, 3) residual the network returned (B = 16 x 24, row-major pixels);
  * a second pair for `conv_decoder` alone at 13 x 19: a seeded input with non-negative features, unit rays and colours in [0, 1], and its (1, 3, 13, 19) output.

The fixture is data only; nothing of the reference is copied.  Re-run:  python tests/golden/make_hourglass_fixture.py
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

FH, FW = 16, 24
src = np.load(os.path.join(HERE, "coloragg.npz"))
assert tuple(src["window"][2:]) == (FH, FW)

torch.manual_seed(2)
net = ColorFusionResidualNet(height=FH, width=FW)
seen = {}
net.conv_decoder.register_forward_pre_hook(lambda m, args: seen.update(cnn_input=args[0]))
net.register_forward_hook(lambda m, args, out: seen.update(residual=out))
pkg = {name: torch.tensor(src["in_" + key]) for name, key in (("render", "color"), ("cam_feat", "cam_feat"), ("warped_image", "warped_image"),
                                                             ("min_depth_diff", "min_depth_diff"), ("camera_ray", "camera_ray"),
                                                             ("use_first_src_frame_mask", "use_first_src_frame_mask"))}
opts = types.SimpleNamespace(enable_exposure_correction=False, nb_visible_src_frames=3, residual_resolution_scale=1.0)
with torch.no_grad():
    r = fuse_color(pkg, net, None, None, None, 0, opts)
assert r is not None and r["nb_valid_warp_level"] == 3 and tuple(seen["cnn_input"].shape) == (1, 38, FH, FW) and tuple(seen["residual"].shape) == (FH * FW, 3)
assert torch.equal(r["residual"], seen["residual"].T.view(3, FH, FW)) and r["burned_in_gauss"] == 1.0

out = {"window": src["window"], "cnn_input": seen["cnn_input"].numpy(), "residual": seen["residual"].numpy(), "image_pred": r["image_pred"].numpy()}
for k, v in net.state_dict().items():
    out["sd/" + k] = v.numpy()

# conv_decoder alone on an odd frame
H2, W2 = 13, 19
g = np.random.default_rng(5)
feat = np.maximum(g.standard_normal((32, H2, W2)), 0) * 0.5
ray = g.standard_normal((3, H2, W2))
ray /= np.linalg.norm(ray, axis=0, keepdims=True)
x2 = np.concatenate([feat, ray, g.random((3, H2, W2))]).astype(np.float32)[None]
with torch.no_grad():
    y2 = net.conv_decoder(torch.tensor(x2))
assert tuple(y2.shape) == (1, 3, H2, W2)
out["odd_cnn_input"], out["odd_residual"] = x2, y2.numpy()

path = os.path.join(HERE, "hourglass.npz")
np.savez_compressed(path, **out)
print("hourglass.npz written:", len(out), "arrays,", os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1 << 20
