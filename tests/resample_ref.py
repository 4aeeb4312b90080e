"""Restatements of the reduced-resolution colour tail (ibgs_amd/resample.py, csrc/resample.hip), written from its contract (include/ibgs_resample.h; DESIGN.md
section 19) with explicit taps and weights -- not from F.interpolate:

  * `taps(n_in, n_out)`: y0, y1 and t of every output index, the taps in integers, t = rem / (n_out - 1) in float64;
  * `resample_ref(planes, size)`: float64 bilinear gather of (C, H, W) planes;
  * `features_ref`: the ARBITER of `resized_features`: per slot the masked 7 features at full resolution (tests/coloragg_ref.assemble_ref: the mask is the
    float32 sum, part of the definition), resampled, the two Linear + ReLU, the mean or maximum, the normalised ray, the colour;
  * `upsample_ref`: the arbiter of `upsample_residual`;
  * `images_first_ref`: the WRONG order on purpose -- interpolate the images and the feature planes, then mask and subtract -- which the host tests must tell
    from the right one;
  * `chain_f32`: `features_ref` in sequential float32 (the kernel's blend order, then k-ordered multiply-add chains from the bias): one of the two yardsticks;
  * `torch_composition`: the reference's own three F.interpolate calls around the assembly, in torch ops at any float type: the other yardstick at float32,
    and at float64 the check of this file against torch."""
import numpy as np
import torch

from tests import coloragg_ref

WIDTH = 32


def scaled_size(h, w, s):
    return int(h * s), int(w * s)


def taps(n_in, n_out):
    """-> (i0, i1, t): int64, int64, float64 arrays of n_out entries.  y = i (n_in - 1) / (n_out - 1), or 0 when n_out == 1."""
    i = np.arange(n_out, dtype=np.int64)
    if n_out == 1:
        num, den = np.zeros(1, dtype=np.int64), 1
    else:
        num, den = i * (n_in - 1), n_out - 1
    i0 = num // den
    return i0, np.minimum(i0 + 1, n_in - 1), (num - i0 * den) / float(den)


def resample_ref(planes, size, dtype=np.float64):
    """planes (..., H, W) -> (..., size[0], size[1]) in `dtype`: (1 - ty) ((1 - tx) a + tx b) + ty ((1 - tx) c + tx d)."""
    p = np.asarray(planes).astype(dtype)
    y0, y1, ty = taps(p.shape[-2], size[0])
    x0, x1, tx = taps(p.shape[-1], size[1])
    ty, tx = ty.astype(dtype)[:, None], tx.astype(dtype)[None, :]
    a, b = p[..., y0[:, None], x0[None, :]], p[..., y0[:, None], x1[None, :]]
    c, d = p[..., y1[:, None], x0[None, :]], p[..., y1[:, None], x1[None, :]]
    one = dtype(1)
    top = (tx * b + ((one - tx) * a).astype(dtype)).astype(dtype)
    bottom = (tx * d + ((one - tx) * c).astype(dtype)).astype(dtype)
    return (ty * bottom + ((one - ty) * top).astype(dtype)).astype(dtype)


def full_features(render, warped, cam_feat, levels, dtype=np.float64):
    """-> (levels, 7, H, W): the slot definition at full resolution, each pixel under its own mask (the float32 sum in index order)."""
    r = coloragg_ref._np(render).astype(dtype)
    h, w = r.shape[-2:]
    wl = coloragg_ref._np(warped).astype(dtype).reshape(-1, 3, h, w)[:levels]
    ft = coloragg_ref._np(cam_feat).astype(dtype).reshape(-1, 4, h, w)[:levels]
    v = coloragg_ref.valid_ref(cam_feat)[:levels].astype(dtype)
    return np.concatenate([((wl - r[None]).astype(dtype) * v[:, None]).astype(dtype), ft], axis=1)


def _levels(warped, nb, levels, s):
    counted = coloragg_ref.levels_ref(warped, nb)
    return counted if levels is None else max(0, min(int(levels), s))


def _tail(x, ray_r, colour_r, params, levels, mode, size):
    """x (levels, 7, Hr, Wr) -> (1, 38, Hr, Wr) in float64."""
    hr, wr = size
    p1, q1, p2, q2 = (coloragg_ref._np(t).astype(np.float64) for t in params)
    rows = x.astype(np.float64).transpose(2, 3, 0, 1).reshape(hr * wr, levels, 7)
    h1 = np.maximum(rows @ p1.T + q1, 0.0)
    h2 = np.maximum(h1 @ p2.T + q2, 0.0)
    if levels == 0:
        agg = np.zeros((hr * wr, WIDTH))
    elif mode == "mean":
        agg = h2.sum(1) / levels
    else:
        agg = h2.max(1)
    return np.concatenate([agg.T.reshape(WIDTH, hr, wr), ray_r, colour_r], axis=0).reshape(1, WIDTH + 6, hr, wr)


def _ray(ray, size, dtype=np.float64):
    r = resample_ref(coloragg_ref._np(ray), size, dtype)
    n = np.sqrt(((r[0] * r[0] + r[1] * r[1]).astype(dtype) + r[2] * r[2]).astype(dtype)).astype(dtype)
    return (r / (n + dtype(1e-10)).astype(dtype)).astype(dtype)


def features_ref(render, warped, cam_feat, camera_ray, w1, b1, w2, b2, size, nb_visible_src_frames=3, mode="mean", levels=None):
    """-> ((1, 38, Hr, Wr) float64, the level count used).  levels=None: counted at full resolution and capped by nb_visible_src_frames; an int: kept
    within 0 .. S as the kernel keeps a device word."""
    h, w = coloragg_ref._np(render).shape[-2:]
    s = coloragg_ref._np(warped).reshape(-1, 3, h, w).shape[0]
    levels = _levels(warped, nb_visible_src_frames, levels, s)
    x = resample_ref(full_features(render, warped, cam_feat, levels), size)
    return _tail(x, _ray(camera_ray, size), resample_ref(coloragg_ref._np(render), size), (w1, b1, w2, b2), levels, mode, size), levels


def x_views_ref(render, warped, cam_feat, camera_ray, size, levels):
    """The three tensors the reference's fuse_color hands to its network, in its layout: x_views (Hr Wr, levels, 7), ray_dir (Hr Wr, 3), c_3dgs (Hr Wr, 3)."""
    hr, wr = size
    x = resample_ref(full_features(render, warped, cam_feat, levels), size)
    return (x.transpose(2, 3, 0, 1).reshape(hr * wr, levels, 7), _ray(camera_ray, size).reshape(3, -1).T, resample_ref(coloragg_ref._np(render), size).reshape(3, -1).T)


def images_first_ref(render, warped, cam_feat, size, levels):
    """Interpolate-then-mask: x_views (Hr Wr, levels, 7) assembled from interpolated images and feature planes.  NOT the contract."""
    hr, wr = size
    h, w = coloragg_ref._np(render).shape[-2:]
    r = resample_ref(coloragg_ref._np(render), size)
    wl = resample_ref(coloragg_ref._np(warped).reshape(-1, 3, h, w)[:levels], size)
    ft = resample_ref(coloragg_ref._np(cam_feat).reshape(-1, 4, h, w)[:levels], size)
    v = (ft.sum(1, keepdims=True) > 0).astype(np.float64)
    return np.concatenate([(wl - r[None]) * v, ft], axis=1).transpose(2, 3, 0, 1).reshape(hr * wr, levels, 7)


def upsample_ref(residual, render, render_scale=1.0, dtype=np.float64):
    """-> (residual_up, image_pred) (3, H, W) in `dtype`."""
    r = coloragg_ref._np(render).astype(dtype)
    up = resample_ref(coloragg_ref._np(residual), r.shape[-2:], dtype)
    return up, ((dtype(render_scale) * r).astype(dtype) + up).astype(dtype)


def _chain_layer(x, wt, bias, order):
    """x (N, K) float32 -> (N, 32): per output a multiply-add chain from the bias over the inputs in `order`, each step rounded once (a product of two floats
    is exact in float64, and the float64 sum of it and a float rounds to float32 as the fused operation does, but for rare double roundings)."""
    acc = np.broadcast_to(bias.astype(np.float32), (x.shape[0], wt.shape[0])).copy()
    for k in order:
        acc = (acc.astype(np.float64) + x[:, k:k + 1].astype(np.float64) * wt[None, :, k].astype(np.float64)).astype(np.float32)
    return acc


# the order in which the matrix-core instruction takes the 32 channels of the second layer: k-step kk takes ch(kk, 0) then ch(kk, 1)
MFMA_ORDER = [(kk & 3) + 8 * (kk >> 2) + 4 * h for kk in range(16) for h in range(2)]


def chain_f32(render, warped, cam_feat, camera_ray, w1, b1, w2, b2, size, nb_visible_src_frames=3, mode="mean", levels=None):
    """`features_ref` as a sequential float32 program: the blends in the kernel's order, the layers as chains, the mean as ((h0 + h1) + ..) / levels."""
    f32 = np.float32
    hr, wr = size
    h, w = coloragg_ref._np(render).shape[-2:]
    s = coloragg_ref._np(warped).reshape(-1, 3, h, w).shape[0]
    levels = _levels(warped, nb_visible_src_frames, levels, s)
    x = resample_ref(full_features(render, warped, cam_feat, levels, f32), size, f32)
    p1, q1, p2, q2 = (coloragg_ref._np(t).astype(f32) for t in (w1, b1, w2, b2))
    rows = x.transpose(2, 3, 0, 1).reshape(hr * wr * levels, 7)
    h1 = np.maximum(_chain_layer(rows, p1, q1, range(7)), 0)
    h2 = np.maximum(_chain_layer(h1, p2, q2, MFMA_ORDER), 0).reshape(hr * wr, levels, WIDTH)
    if levels == 0:
        agg = np.zeros((hr * wr, WIDTH), dtype=f32)
    elif mode == "mean":
        agg = h2[:, 0]
        for k in range(1, levels):
            agg = (agg + h2[:, k]).astype(f32)
        agg = (agg / f32(levels)).astype(f32) if levels > 1 else agg
    else:
        agg = h2.max(1)
    return np.concatenate([agg.T.reshape(WIDTH, hr, wr), _ray(camera_ray, size, f32), resample_ref(coloragg_ref._np(render), size, f32)], axis=0).reshape(1, WIDTH + 6, hr, wr)


def torch_composition(render, warped, cam_feat, camera_ray, w1, b1, w2, b2, size, nb_visible_src_frames=3, mode="mean", dtype=torch.float32, levels=None):
    """The reference's order in torch ops at `dtype` on the CPU: assemble and mask at full resolution, F.interpolate (bilinear, align_corners=True) the
    features, the colour and the ray, normalise the ray, the MLP, the aggregation.  -> (1, 38, Hr, Wr)."""
    F = torch.nn.functional
    t = lambda a: torch.as_tensor(coloragg_ref._np(a))
    render, warped, cam_feat, camera_ray = t(render), t(warped), t(cam_feat), t(camera_ray)
    _, h, w = render.shape
    s = warped.reshape(-1, 3, h, w).shape[0]
    levels = _levels(warped, nb_visible_src_frames, levels, s)
    r = render.to(dtype)
    resize = lambda planes: F.interpolate(planes, size=tuple(size), mode="bilinear", align_corners=True)
    colour = resize(r[None])
    ray = resize(camera_ray.to(dtype)[None])
    ray = ray / (torch.norm(ray, dim=1, keepdim=True) + 1e-10)
    hr, wr = size
    if levels == 0:
        return torch.cat([torch.zeros((1, WIDTH, hr, wr), dtype=dtype), ray, colour], dim=1)
    wl = warped.reshape(-1, 3, h, w)[:levels].to(dtype)
    ft = cam_feat.reshape(-1, 4, h, w)[:levels]
    f32 = ft.float()
    valid = ((((f32[:, 0] + f32[:, 1]) + f32[:, 2]) + f32[:, 3]) > 0).to(dtype).unsqueeze(1)
    x = torch.cat([(wl - r[None]) * valid, ft.to(dtype)], dim=1)                       # (levels, 7, H, W)
    x = resize(x).permute(2, 3, 0, 1).reshape(hr * wr * levels, 7)
    lin = F.linear
    feats = torch.relu(lin(torch.relu(lin(x, t(w1).to(dtype), t(b1).to(dtype))), t(w2).to(dtype), t(b2).to(dtype))).view(hr * wr, levels, WIDTH)
    agg = feats.mean(dim=1) if mode == "mean" else feats.max(dim=1).values
    return torch.cat([agg.T.reshape(1, WIDTH, hr, wr), ray, colour], dim=1)


def torch_upsample(residual, render, render_scale=1.0, dtype=torch.float32):
    """-> (residual_up, image_pred) by F.interpolate(size=(H, W), bilinear, align_corners=True) on the CPU."""
    res = torch.as_tensor(coloragg_ref._np(residual)).to(dtype)
    r = torch.as_tensor(coloragg_ref._np(render)).to(dtype)
    up = torch.nn.functional.interpolate(res[None], size=tuple(r.shape[-2:]), mode="bilinear", align_corners=True)[0]
    return up, render_scale * r + up


def seeded_case(h, w, s=3, seed=0):
    """The inputs of the resample tests, on the CPU: ((render, warped (S, 3, H, W), cam_feat (S, 4, H, W), camera_ray), (w1, b1, w2, b2)).  Validity varies between neighbouring pixels in every slot, slot 1 is invalid everywhere."""
    g = torch.Generator().manual_seed(seed * 7919 + 131 * s + 17 * h + w)
    render = torch.rand(3, h, w, generator=g)
    warped = (render[None] + 0.15 * torch.randn(s, 3, h, w, generator=g)).clamp(0.01, 1)
    f = torch.randn(s, 4, h, w, generator=g) * 0.2 + 0.5
    f[:, 0][f.sum(1) < 0.3] += 1.0
    kind = torch.rand(s, 1, h, w, generator=g)
    feat = torch.where(kind < 0.6, f, torch.zeros(()))
    feat = torch.where(kind >= 0.85, -f, feat)
    if s > 1:
        feat[1] = 0
    ray = torch.nn.functional.normalize(torch.randn(3, h, w, generator=g), dim=0)
    params = tuple(((torch.rand(shape, generator=g) * 2 - 1) / fan ** 0.5) for shape, fan in (((32, 7), 7), ((32,), 7), ((32, 32), 32), ((32,), 32)))
    return tuple(t.float().contiguous() for t in (render, warped, feat, ray)), params
