"""The arbiter of training at a reduced residual resolution (ibgs_amd/resample_train.py, csrc/rsztrain.hip): tests/resample_ref's explicit taps and weights as a
DIFFERENTIABLE torch composition on the CPU, so that autograd's gradients of it are the float64 statement of include/ibgs_resample_train.h:

  * `gather(planes, size)`: the bilinear gather with `resample_ref.taps` (integer taps, t = rem / (n_out - 1)), at the dtype of `planes`;
  * `features(...)`: `resized_features` -- the masked slots (the mask is the float32 sum: part of the definition), gathered, the two Linear + ReLU, the mean or
    maximum, the normalised ray, the colour.  `dtype=torch.float64` is the ARBITER; `dtype=torch.float32` its float32 TWIN (one yardstick);
    `interpolate=True` puts F.interpolate(bilinear, align_corners=True) in the gather's place: torch's own composition, the reference's order (at float32 the
    other yardstick, at float64 the check of this file against torch);
  * `feature_grads`, `upsample_grads`: autograd of `(out * upstream).sum()`;
  * `tail_grads`: the whole training tail of `fuse_color_train_scaled` -- the exposure correction (its affine map a constant), `features`, the hourglass, the
    upsampling, image_pred -- chained through tests/hourglass_bwd_ref (float64: `backward_ref` on `forward_ref`'s stages; float32: the chains), or with the CNN in
    torch ops where `interpolate=True`;
  * `margin`, `decided_seed`, `SEEDS`: a gradient is discontinuous where a pre-activation or a max-mode gap is 0, so every frame of the device tests uses the
    smallest seed of `resample_ref.seeded_case` whose float64 pre-activations and non-zero max gaps are all >= MARGIN;
  * `raised_biases`: for a frame too large for a seed to give that margin, both biases raised until every pre-activation is >= 0.5."""
import functools

import numpy as np
import torch

from tests import coloragg_ref, exposure_ref
from tests import hourglass_bwd_ref as bref
from tests import hourglass_ref
from tests import resample_ref as ref

F = torch.nn.functional
WIDTH = 32
MARGIN = 2e-6
# (H, W, s) -> the seed of resample_ref.seeded_case (tests/test_resample_train_host.py asserts that each is the smallest with the margin)
SEEDS = {(8, 8, 0.5): 0, (9, 11, 0.5): 0, (9, 13, 0.56): 1, (33, 65, 0.5): 0, (32, 48, 0.75): 4, (35, 37, 0.5): 2}
FRAMES = list(SEEDS)
BIG = (516, 512, 0.5)          # 258 x 256 reduced pixels = 516 chunks of 128: beyond one pass of the reduced-resolution kernel's 512 workgroups
NAMES = ("render", "warped", "w1", "b1", "w2", "b2")


def _t(a, dtype):
    return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dtype)


def gather(planes, size):
    """planes (..., H, W) torch -> (..., size[0], size[1]) at its dtype: top = tx b + (1 - tx) a; bottom = tx d + (1 - tx) c; ty bottom + (1 - ty) top."""
    dtype = planes.dtype
    y0, y1, ty = ref.taps(planes.shape[-2], size[0])
    x0, x1, tx = ref.taps(planes.shape[-1], size[1])
    y0, y1, x0, x1 = (torch.as_tensor(v) for v in (y0, y1, x0, x1))
    ty, tx = torch.as_tensor(ty).to(dtype)[:, None], torch.as_tensor(tx).to(dtype)[None, :]
    a, b = planes[..., y0[:, None], x0[None, :]], planes[..., y0[:, None], x1[None, :]]
    c, d = planes[..., y1[:, None], x0[None, :]], planes[..., y1[:, None], x1[None, :]]
    top, bottom = tx * b + (1 - tx) * a, tx * d + (1 - tx) * c
    return ty * bottom + (1 - ty) * top


def _interpolate(planes, size):
    lead = planes.shape[:-2]
    return F.interpolate(planes.reshape((1, -1) + tuple(planes.shape[-2:])), size=tuple(size), mode="bilinear", align_corners=True).reshape(tuple(lead) + tuple(size))


def features(render, warped, cam_feat, camera_ray, w1, b1, w2, b2, size, levels, mode="mean", dtype=torch.float64, interpolate=False, return_preacts=False):
    """-> (1, 38, Hr, Wr) at `dtype`, differentiable in whatever of render, warped and the parameters requires grad.  levels: an int, kept within 0 .. S."""
    resize = _interpolate if interpolate else gather
    r = _t(render, dtype)
    h, w = r.shape[-2:]
    hr, wr = size
    wl = _t(warped, dtype).reshape(-1, 3, h, w)
    levels = max(0, min(int(levels), wl.shape[0]))
    colour = resize(r, size)
    ray = resize(_t(camera_ray, dtype).reshape(3, h, w), size)
    ray = ray / (torch.sqrt((ray * ray).sum(0, keepdim=True)) + 1e-10)
    pre = None
    if levels == 0:
        agg = torch.zeros((WIDTH, hr, wr), dtype=dtype)
    else:
        valid = torch.as_tensor(coloragg_ref.valid_ref(cam_feat)[:levels]).to(dtype).unsqueeze(1)
        ft = _t(cam_feat, dtype).reshape(-1, 4, h, w)[:levels]
        x = torch.cat([(wl[:levels] - r[None]) * valid, ft], dim=1)          # masked at full resolution, then resampled
        x = resize(x, size).permute(2, 3, 0, 1).reshape(hr * wr * levels, 7)
        z1 = F.linear(x, _t(w1, dtype), _t(b1, dtype))
        z2 = F.linear(torch.relu(z1), _t(w2, dtype), _t(b2, dtype))
        feats = torch.relu(z2).view(hr * wr, levels, WIDTH)
        agg = feats.mean(dim=1) if mode == "mean" else feats.max(dim=1).values
        agg = agg.T.reshape(WIDTH, hr, wr)
        pre = (z1.detach(), z2.detach().view(hr * wr, levels, WIDTH))
    out = torch.cat([agg, ray, colour], dim=0)[None]
    return (out, pre) if return_preacts else out


def feature_grads(case, params, size, levels, mode, grad_out, dtype=torch.float64, interpolate=False):
    """case = (render, warped, cam_feat, camera_ray), params = (w1, b1, w2, b2), grad_out (1, 38, Hr, Wr).  -> ({name: float64 numpy gradient of
    (out * grad_out).sum()} for NAMES, out as float64 numpy).  With levels == 0 the graph does not reach warped or the parameters: their gradients are zeros."""
    render, warped = (_t(case[k], dtype).clone().requires_grad_(True) for k in (0, 1))
    p = [_t(v, dtype).clone().requires_grad_(True) for v in params]
    out = features(render, warped, case[2], case[3], *p, size, levels, mode, dtype, interpolate)
    leaves = [render, warped] + p
    got = torch.autograd.grad((out * _t(grad_out, dtype)).sum(), leaves, allow_unused=True)
    grads = {k: (torch.zeros_like(t) if g is None else g).detach().double().numpy() for k, t, g in zip(NAMES, leaves, got)}
    return grads, out.detach().double().numpy()


def upsample(residual, render, render_scale, interpolate=False):
    """-> (residual_up, image_pred) (3, H, W) torch at residual's dtype."""
    up = (_interpolate if interpolate else gather)(residual, tuple(render.shape[-2:]))
    return up, render_scale * render + up


def upsample_grads(residual, render, render_scale, g_up, g_pred, dtype=torch.float64, interpolate=False):
    """-> {"residual", "render"}: float64 numpy gradients of (up g_up).sum() + (pred g_pred).sum(); either upstream may be None."""
    res, r = _t(residual, dtype).clone().requires_grad_(True), _t(render, dtype).clone().requires_grad_(True)
    up, pred = upsample(res, r, render_scale, interpolate)
    loss = 0
    if g_up is not None:
        loss = loss + (up * _t(g_up, dtype)).sum()
    if g_pred is not None:
        loss = loss + (pred * _t(g_pred, dtype)).sum()
    got = torch.autograd.grad(loss, [res, r], allow_unused=True)
    return {k: (torch.zeros_like(t) if g is None else g).detach().double().numpy() for k, t, g in zip(("residual", "render"), (res, r), got)}


# ---- decided cases -------------------------------------------------------------------------------------------------------------------------------------------
def margin(case, params, size, levels=3):
    """-> (the smallest |pre-activation| of both layers, the smallest non-zero gap between a channel's maximum over the slots and its runner-up) in float64."""
    with torch.no_grad():
        _, (z1, z2) = features(*case, *params, size, levels, "max", torch.float64, return_preacts=True)
    h2 = torch.relu(z2).sort(dim=1).values
    gap = h2[:, -1] - h2[:, -2] if h2.shape[1] > 1 else torch.ones(1, dtype=torch.float64)
    gap = gap[gap > 0]
    return min(float(z1.abs().min()), float(z2.abs().min())), (float(gap.min()) if gap.numel() else float("inf"))


@functools.lru_cache(maxsize=None)
def decided_seed(h, w, s, limit=64):
    """The smallest seed of resample_ref.seeded_case(h, w) with margin >= MARGIN at levels 3 (levels 1 reads a subset of its pre-activations and has no gap)."""
    size = ref.scaled_size(h, w, s)
    for seed in range(limit):
        case, params = ref.seeded_case(h, w, seed=seed)
        if min(margin(case, params, size)) >= MARGIN:
            return seed
    raise AssertionError("no seed below %d decides %dx%d at %g" % (limit, h, w, s))


def raised_biases(case, params, size, levels=3, least=0.5):
    """-> (w1, b1 + c1, w2, b2 + c2) float32 with every float64 pre-activation of both layers >= `least` (the caller asserts it): c1 from the first layer's
    minimum, then c2 from the second's under the raised b1.  Steps of 1/4, so the raised biases are as exact in float32 as the biases were."""
    w1, b1, w2, b2 = (t.clone() for t in params)
    step = lambda low: float(np.ceil((least + 0.25 - low) * 4) / 4) if low < least + 0.25 else 0.0
    with torch.no_grad():
        _, (z1, _) = features(*case, w1, b1, w2, b2, size, levels, "mean", torch.float64, return_preacts=True)
        b1 = (b1 + step(float(z1.min()))).float()
        _, (_, z2) = features(*case, w1, b1, w2, b2, size, levels, "mean", torch.float64, return_preacts=True)
        b2 = (b2 + step(float(z2.min()))).float()
    return w1, b1, w2, b2


# ---- the whole training tail -------------------------------------------------------------------------------------------------------------------------------
def _cnn_torch(x, cp):
    conv = lambda v, name, pad: F.conv2d(v, cp[name + "_w"], cp[name + "_b"], padding=pad)
    e1 = F.relu(conv(x, "enc1", 1))
    e2 = F.relu(conv(F.max_pool2d(e1, 2), "enc2", 1))
    b = F.relu(conv(F.max_pool2d(e2, 2), "enc3", 1))
    u2 = F.relu(conv(F.interpolate(b, size=e2.shape[-2:], mode="nearest"), "up2_conv", 1))
    d2 = F.relu(conv(torch.cat([u2, e2], 1), "dec2", 1))
    u1 = F.relu(conv(F.interpolate(d2, size=e1.shape[-2:], mode="nearest"), "up1_conv", 1))
    d1 = F.relu(conv(torch.cat([u1, e1], 1), "dec1", 1))
    f = F.relu(conv(torch.cat([d1, x], 1), "fuse_input", 0))
    return conv(f, "final", 0)[0]


def tail_grads(planes, mlp, cnn, size, upstream, burned=1.0, expo=False, dtype=torch.float64, interpolate=False, images=True, levels=3):
    """planes: {"color", "warped_image", "cam_feat", "camera_ray", "use_first_src_frame_mask"} (numpy); mlp = (w1, b1, w2, b2); cnn: the eighteen tensors under
    tests/hourglass_ref's names; upstream: (3, H, W) on image_pred.  -> ({"render", "warped", "w1", .., "b2", "enc1_w", ..}: float64 numpy gradients of
    (image_pred upstream).sum(), image_pred as float64 numpy).  The exposure correction's affine map is a constant of the backward, as in the reference.
    `interpolate`: F.interpolate both ways and the CNN in torch ops (torch's own composition); otherwise the explicit taps, and the CNN through
    tests/hourglass_ref / hourglass_bwd_ref (float64: the arbiters; float32: the chains).  `images=False`: render and warped are constants (the burn-in)."""
    render = _t(planes["color"], dtype).clone().requires_grad_(images)
    warped = _t(planes["warped_image"], dtype).clone().requires_grad_(images)
    p = [_t(v, dtype).clone().requires_grad_(True) for v in mlp]
    g = _t(upstream, dtype)
    shown = render
    if expo:
        affine = _t(exposure_ref.fit_ref(planes["color"], planes["warped_image"], planes["use_first_src_frame_mask"])[0], dtype)
        shown = torch.einsum("ij,jhw->ihw", affine[:, :3], render) + affine[:, 3, None, None]
    x = features(shown, warped, planes["cam_feat"], planes["camera_ray"], *p, size, levels, "mean", dtype, interpolate)
    leaves = ([render, warped] if images else []) + p
    names = (["render", "warped"] if images else []) + ["w1", "b1", "w2", "b2"]
    if interpolate:
        cp = {k: _t(v, dtype).clone().requires_grad_(True) for k, v in cnn.items()}
        _, pred = upsample(_cnn_torch(x, cp), shown, burned, True)
        got = torch.autograd.grad((pred * g).sum(), leaves + list(cp.values()))
        out = {k: v.double().numpy() for k, v in zip(names + list(cp), got)}
        return out, pred.detach().double().numpy()
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    xin = x.detach().numpy()
    fwd = hourglass_ref.forward_ref(xin, cnn) if dtype == torch.float64 else hourglass_ref.chain_f32(xin, cnn)
    res_r = torch.as_tensor(np.asarray(fwd["residual"], dtype=np_dtype)).requires_grad_(True)
    _, pred = upsample(res_r, shown, burned)
    loss = (pred * g).sum()
    g_res = torch.autograd.grad(loss, res_r, retain_graph=True)[0].numpy()
    back = (bref.backward_ref if dtype == torch.float64 else bref.backward_chain_f32)(xin, cnn, fwd, g_res, None, 1.0)
    got = torch.autograd.grad(loss + (x * torch.as_tensor(np.asarray(back["x"], dtype=np_dtype)).reshape(x.shape)).sum(), leaves)
    out = {k: v.double().numpy() for k, v in zip(names, got)}
    out.update({k: np.asarray(v, dtype=np.float64) for k, v in back.items() if k != "x"})
    return out, pred.detach().double().numpy()


# ---- the recorded gradients of the reference (tests/golden/consumer_resized_train.npz) ------------------------------------------------------------------
FIXED_BITS = 38          # a recorded gradient is round(g / max|g| 2^38) split into an int32 (the high bits) and a uint8 (the low eight): 2^-39 max|g| at most off


def pack_fixed(g):
    g = np.asarray(g, dtype=np.float64)
    top = float(np.abs(g).max())
    q = np.rint(g / top * 2.0 ** FIXED_BITS).astype(np.int64) if top > 0 else np.zeros(g.shape, np.int64)
    return {"hi": (q >> 8).astype(np.int32), "lo": (q & 0xFF).astype(np.uint8), "max": np.float64(top)}


def unpack_fixed(z, key):
    q = (z[key + "/hi"].astype(np.int64) << 8) | z[key + "/lo"].astype(np.int64)
    return q.astype(np.float64) * (float(z[key + "/max"]) / 2.0 ** FIXED_BITS)
