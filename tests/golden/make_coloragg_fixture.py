"""Generates tests/golden/coloragg.npz IN THE BUILD CONTAINER, where the reference is present (as make_consumer_fixture.py does): the oracle outputs stored
in consumer.npz, cropped to a 16 x 24 window in which all three slot levels carry pixels, go through the reference's own `fuse_color` and a seeded
`ColorFusionResidualNet(height=16, width=24)` on CPU (/root/reference/color_aggregation_network.py, imported read-only).  Recorded per aggregation mode:

  * the (1, 38, 16, 24) tensor `conv_decoder` received (captured with a forward pre-hook);
  * under a seeded upstream gradient of that shape: the gradients of the four `per_view_mlp` parameters, of `render` and of `warped_image`;
and once: the cropped inputs, the four parameters and the upstream gradient.

The fixture is data only; nothing of the reference is copied.  Re-run:  python tests/golden/make_coloragg_fixture.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

from color_aggregation_network import ColorFusionResidualNet, fuse_color  # noqa: E402

FH, FW = 16, 24
src = np.load(os.path.join(HERE, "consumer.npz"))
H, W = int(src["H"]), int(src["W"])


def carried(y, x):
    w = src["oracle_warped_image"][:, y:y + FH, x:x + FW].reshape(-1, 3, FH, FW)
    return [int((np.abs(w[k]).sum(0) > 0).sum()) for k in range(w.shape[0])]


# the first window (rows, then columns, in steps of 4) whose first three slot levels each carry at least a tenth of the pixels
y0, x0 = next((y, x) for y in range(0, H - FH + 1, 4) for x in range(0, W - FW + 1, 4) if min(carried(y, x)[:3]) >= FH * FW // 10)
crop = lambda k: np.ascontiguousarray(src["oracle_" + k][..., y0:y0 + FH, x0:x0 + FW])
inputs = {k: crop(k) for k in ("color", "cam_feat", "warped_image", "min_depth_diff", "camera_ray", "use_first_src_frame_mask")}
per_level = carried(y0, x0)
assert all(n > 0 for n in per_level[:3]), per_level

torch.manual_seed(0)
upstream = torch.randn(1, 38, FH, FW)
out = {"window": np.int32([y0, x0, FH, FW]), "upstream": upstream.numpy(), "pixels_per_level": np.int32(per_level)}
for k, v in inputs.items():
    out["in_" + k] = v
for mode in ("mean", "max"):
    torch.manual_seed(1)
    net = ColorFusionResidualNet(height=FH, width=FW, feat_aggregate_mode=mode)
    seen = {}
    net.conv_decoder.register_forward_pre_hook(lambda m, args: seen.update(cnn_input=args[0]))
    pkg = {name: torch.tensor(inputs[key]) for name, key in (("render", "color"), ("cam_feat", "cam_feat"), ("warped_image", "warped_image"),
                                                            ("min_depth_diff", "min_depth_diff"), ("camera_ray", "camera_ray"),
                                                            ("use_first_src_frame_mask", "use_first_src_frame_mask"))}
    pkg["render"].requires_grad_(True)
    pkg["warped_image"].requires_grad_(True)
    opts = types.SimpleNamespace(enable_exposure_correction=False, nb_visible_src_frames=3, residual_resolution_scale=1.0)
    r = fuse_color(pkg, net, None, None, None, 0, opts)
    assert r is not None and r["nb_valid_warp_level"] == 3 and tuple(seen["cnn_input"].shape) == (1, 38, FH, FW)
    params = [net.per_view_mlp[0].weight, net.per_view_mlp[0].bias, net.per_view_mlp[2].weight, net.per_view_mlp[2].bias]
    grads = torch.autograd.grad(seen["cnn_input"], params + [pkg["render"], pkg["warped_image"]], grad_outputs=upstream)
    if mode == "mean":
        for name, p in zip(("w1", "b1", "w2", "b2"), params):
            out[name] = p.detach().numpy().copy()
    else:
        assert all(np.array_equal(out[name], p.detach().numpy()) for name, p in zip(("w1", "b1", "w2", "b2"), params))
    out[mode + "_cnn_input"] = seen["cnn_input"].detach().numpy()
    out[mode + "_valid_warp_mask"] = r["valid_warp_mask"].detach().numpy()
    for name, g in zip(("w1", "b1", "w2", "b2", "render", "warped_image"), grads):
        out[mode + "_grad_" + name] = g.numpy()
path = os.path.join(HERE, "coloragg.npz")
np.savez_compressed(path, **out)
print("coloragg.npz written: window", (y0, x0), "pixels per level", per_level, "bytes", os.path.getsize(path))
assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "consumer.npz"))
