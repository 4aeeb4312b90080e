"""Generates tests/golden/consumer_resized_train.npz IN THE BUILD CONTAINER, where the reference is present (as make_consumer_resized_fixture.py does): the
`oracle_*` tensors of consumer.npz (48 x 32, 3 levels) and the state dict of consumer_resized.npz (seed 4) are fed to the reference's own `fuse_color`
(color_aggregation_network.py:156-250, imported read-only through _ref_import's path) with `residual_resolution_scale` = 0.5, plain ("half_") and with exposure
correction ("half_exposure_"), on the CPU, once in float64 and once in float32, with render, warped_image and all 22 parameters requiring grad and
`loss = (image_pred * g).sum()` for a seeded g.  Recorded:

  * "g": the upstream gradient (3, H, W) float32, and its seed;
  * of the float64 run, per tag: the gradients of render ("half_grad/render"), warped_image ("../warped_image") and the 22 parameters under the reference's
    keys ("../per_view_mlp.0.weight", "../conv_decoder.enc1.0.weight", ...), each as 40-bit fixed point of its own maximum (tests/resample_train_ref.pack_fixed:
    "/hi" int32, "/lo" uint8, "/max" float64 -- at most 2^-39 max off; whole float64 arrays of both runs would pass the size limit of a committed file);
  * of the float32 run, per tag: ONLY each tensor's max-abs distance from the float64 run ("half_d32/<key>"), and image_pred's.

The fixture is data only; nothing of the reference is copied.  Re-run:  python tests/golden/make_consumer_resized_train_fixture.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_import as ri  # noqa: E402

sys.path.insert(0, ri.REF)
from color_aggregation_network import ColorFusionResidualNet, fuse_color  # noqa: E402

from tests.resample_train_ref import pack_fixed  # noqa: E402

G_SEED = 11
src, made = np.load(os.path.join(HERE, "consumer.npz")), np.load(os.path.join(HERE, "consumer_resized.npz"))
H, W = int(src["H"]), int(src["W"])
planes = {name: torch.tensor(src["oracle_" + key]) for name, key in (("render", "color"), ("cam_feat", "cam_feat"), ("warped_image", "warped_image"),
                                                                     ("min_depth_diff", "min_depth_diff"), ("camera_ray", "camera_ray"),
                                                                     ("use_first_src_frame_mask", "use_first_src_frame_mask"))}
sd = {k[3:]: torch.tensor(made[k]) for k in made.files if k.startswith("sd/")}
g = torch.randn(3, H, W, generator=torch.Generator().manual_seed(G_SEED))
s = 0.5


def run(dtype, expo):
    net = ColorFusionResidualNet(height=int(H * s), width=int(W * s))
    net.load_state_dict(sd)
    net = net.to(dtype)
    pkg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in planes.items()}
    for k in ("render", "warped_image"):
        pkg[k] = pkg[k].clone().requires_grad_(True)
    opts = types.SimpleNamespace(enable_exposure_correction=expo, nb_visible_src_frames=3, residual_resolution_scale=s)
    r = fuse_color(pkg, net, None, None, None, 0, opts)
    assert r is not None and r["burned_in_gauss"] == 1.0 and r["nb_valid_warp_level"] == 3 and r["image_pred"].dtype == dtype
    (r["image_pred"] * g.to(dtype)).sum().backward()
    grads = {"render": pkg["render"].grad, "warped_image": pkg["warped_image"].grad}
    grads.update({k: p.grad for k, p in net.named_parameters()})
    assert len(grads) == 24 and all(v is not None and torch.isfinite(v).all() for v in grads.values())
    return {k: v.double().numpy() for k, v in grads.items()}, r["image_pred"].detach().double().numpy()


out = {"H": H, "W": W, "g": g.numpy(), "g_seed": np.int32(G_SEED), "scale": np.float64(s), "fixed_bits": np.int32(38)}
for tag, expo in (("half", False), ("half_exposure", True)):
    g64, pred64 = run(torch.float64, expo)
    g32, pred32 = run(torch.float32, expo)
    for k, v in g64.items():
        for part, a in pack_fixed(v).items():
            out["%s_grad/%s/%s" % (tag, k, part)] = a
        out["%s_d32/%s" % (tag, k)] = np.float64(np.abs(g32[k] - v).max())
    out[tag + "_d32/image_pred"] = np.float64(np.abs(pred32 - pred64).max())
    out[tag + "_image_pred_max"] = np.float64(np.abs(pred64).max())
path = os.path.join(HERE, "consumer_resized_train.npz")
np.savez_compressed(path, **out)
print("consumer_resized_train.npz written:", len(out), "arrays,", os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1 << 20
