"""Restatement of the two geometry loss terms of the reference's steady-state iteration that autograd can differentiate, on any device and in any float
type: the train.py expressions themselves (lines 310-315 and 320-338) over tests/ssim_ref.ssim_map_ref, which stands for `compute_photometric_ssim(...,
size_average=False)`.  At float64 with the "shift2d" window this is the ARBITER of the fused kernels (ibgs_amd/csrc/geoloss.hip); at float32 in the
"conv2d" and "separable" forms it is their yardstick (tests/test_gpu_geoloss.py).

The reference decides `valid` with torch.sum, whose order is its own; the kernels sum ((f0 + f1) + f2) + f3 in float32.  Test inputs therefore keep every
feature sum away from zero: `assert_decided` is the condition, asserted on the CPU when an input is made."""
import torch

from tests import ssim_ref

DECIDED = 2.0 ** -20


def assert_decided(cam_feat):
    """|sum f| > 2^-20 sum |f| at every pixel and source: no summation order, at float32 or float64, can change the sign of the sum.  (An all-zero slot, as the
    rasterizer writes an invalid one, is decided too: every order gives 0.)"""
    f = cam_feat.detach().cpu().double().reshape((-1, 4) + tuple(cam_feat.shape[-2:]))
    total, mag = f.sum(1), f.abs().sum(1)
    assert bool(((total.abs() > DECIDED * mag) | (mag == 0)).all()), "a feature sum is too close to zero for `valid` to be the same in every summation order"


def valid_mask(cam_feat, nb):
    """train.py:322-324 -> (S, 1, H, W) bool."""
    feat = cam_feat.reshape((-1, 4) + tuple(cam_feat.shape[-2:]))[:nb]
    return torch.sum(feat, dim=1, keepdim=True) > 0


def masked_image(gt_image, warped_image, cam_feat, nb, dtype):
    """train.py:320-327 -> (ref_image (1, 3, H, W), masked (S, 3, H, W), valid (S, 1, H, W) bool); unread sources are sliced away before anything reads them."""
    h, w = gt_image.shape[-2:]
    warped = warped_image.reshape(-1, 3, h, w)[:nb].to(dtype)
    valid = valid_mask(cam_feat, nb)
    ref_image = gt_image.to(dtype).unsqueeze(0)
    mask = valid.to(dtype)
    return ref_image, mask * warped + (1 - mask) * ref_image, valid


def photometric_ref(gt_image, warped_image, cam_feat, nb_visible_src_frames=3, photo_weight=0.3, photo_ssim_weight=1.0, dtype=torch.float64, form="shift2d"):
    """train.py:320-338 in `dtype`; a 0-d tensor, differentiable in warped_image."""
    ref_image, masked, valid = masked_image(gt_image, warped_image, cam_feat, nb_visible_src_frames, dtype)
    if not bool(torch.sum(valid) > 0):
        return (masked * 0).sum()
    mask = valid[:, 0].to(dtype)
    ssim_loss = 1 - torch.stack([ssim_ref.ssim_map_ref(ref_image[0], masked[i], dtype, form).mean(0) for i in range(len(masked))])
    ssim_loss = torch.sum(ssim_loss * mask) / torch.sum(mask)
    l1 = torch.abs(ref_image - masked).mean(1)
    l1 = torch.sum(l1 * mask) / torch.sum(mask)
    return (((1 - photo_ssim_weight) * l1 + photo_ssim_weight * ssim_loss) * photo_weight).mean()


def mean_map_ref(gt_image, warped_image, cam_feat, nb, dtype=torch.float64, form="shift2d"):
    """The channel-mean map of (gt, masked) per source, (S, H, W): what the value's bar is taken from."""
    ref_image, masked, _ = masked_image(gt_image, warped_image, cam_feat, nb, dtype)
    return torch.stack([ssim_ref.ssim_map_ref(ref_image[0], masked[i], dtype, form).mean(0) for i in range(len(masked))])


def normal_ref(rendered_normal, depth_normal, weight=0.03, dtype=torch.float64):
    """train.py:310-315 in `dtype`."""
    normal, depth_normal = rendered_normal.to(dtype), depth_normal.to(dtype)
    normal_loss1 = weight * (((depth_normal - normal)).abs().sum(0)).mean()
    normal_loss2 = weight * (1 - ((depth_normal * normal).sum(0))).mean()
    return 0.4 * normal_loss1 + 0.6 * normal_loss2
