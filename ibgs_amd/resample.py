"""The reduced-resolution colour tail of the reference's fuse_color (`residual_resolution_scale != 1`; color_aggregation_network.py:200-239, train.py:227-228) for
test-time rendering: the CNN runs at Hr x Wr = int(H s) x int(W s), on features that were assembled and masked at full resolution and THEN interpolated, and
its residual is interpolated back to H x W -- two kernels (C ABI include/ibgs_resample.h, csrc/resample.hip) around `hourglass.hourglass_forward`:

  resized_features    rasterizer planes (H x W) -> (1, 38, Hr, Wr): per source the masked 7 features at the four full-resolution taps, blended, the per-view MLP
                      on the matrix cores, the mean or maximum over the slot levels; the blended ray, normalised; the blended colour
  upsample_residual   residual (3, Hr, Wr) -> (3, H, W), and image_pred = render_scale * render + that in the same pass

Bilinear, align_corners=True, both ways, with the taps formed in integers (the header states the rule).  `hourglass.fuse_color(...,
residual_resolution_scale=s)` composes them.  FORWARD ONLY: training at a reduced resolution is ibgs_amd/resample_train.py (`resized_features_train`,
`upsample_residual_train`, `fuse_color_train_scaled`: these forwards with the adjoint kernels of csrc/rsztrain.hip behind them); `fuse_color_train` and
`coloragg.fuse_color_inputs` have no such keyword.  The contract is a tolerance against a float64 restatement (tests/resample_ref.py).

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import math

import torch

from . import _device, _lib
from .coloragg import _count, _f32, _front_end_arguments, _image3, count_levels          # noqa: F401  (count_levels is part of this module's surface)

MODES = {"mean": _lib.RSZ_MEAN, "max": _lib.RSZ_MAX}


def scaled_size(h, w, scale):
    """(int(h * scale), int(w * scale)): how the reference sizes its network (train.py) and how F.interpolate(scale_factor=scale) sizes its output."""
    name = "scaled_size"
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise TypeError("%s: scale must be a number, got %s" % (name, type(scale).__name__)) from None
    if isinstance(h, bool) or isinstance(w, bool) or int(h) != h or int(w) != w or h < 1 or w < 1:
        raise ValueError("%s: h and w must be integers >= 1, got %r x %r" % (name, h, w))
    if not math.isfinite(scale) or scale <= 0:
        raise ValueError("%s: scale must be a finite positive number, got %r" % (name, scale))
    return int(int(h) * scale), int(int(w) * scale)


def _size(name, size):
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError("%s: size must be (Hr, Wr), got %r" % (name, size))
    hr, wr = (_count(name, "size's " + what, n, 1) for what, n in zip(("Hr", "Wr"), size))
    if hr > _lib.RSZ_MAX_SIDE or wr > _lib.RSZ_MAX_SIDE:
        raise ValueError("%s: a reduced frame of %d x %d is too large (sides <= %d)" % (name, hr, wr, _lib.RSZ_MAX_SIDE))
    return hr, wr


def _forward_only(name, tensors):
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError("%s is forward only: call it under torch.no_grad() (an input or parameter requires grad and grad mode is on); training at a reduced "
                           "residual resolution is ibgs_amd.resample_train" % name)


def resized_features(render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2, size, levels, mode="mean"):
    """render (3, H, W) (or the exposure-corrected image made of it); warped_image (3 S, H, W) or (S, 3, H, W); cam_feat (4 S, H, W) or (S, 4, H, W);
    camera_ray (3, H, W); the four parameters of `per_view_mlp` in nn.Linear layout; 1 <= S <= 5; size = (Hr, Wr), e.g. `scaled_size(H, W, s)`;
    levels: the 0-d int32 DEVICE tensor `coloragg.per_view_features` returns -- counted at FULL resolution, as the reference counts it -- or an int, which is
    capped at S.  -> cnn_input (1, 38, Hr, Wr) float32: [32 aggregated features, the interpolated ray normalised, the interpolated colour].

    With levels == 0 the 32 aggregated channels are exactly zero; the ray and the colour are still written.  Inputs of another float type or with other
    strides are converted; no argument is written; the same arguments give the same bits on every call and stream; nothing waits for the host.
    Forward only: with grad mode on and an argument that requires grad this raises."""
    name = "resized_features"
    s, h, w, (hr, wr), levels, tensors = _front_end_arguments("resample", name, render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2, MODES, mode, levels,
                                                              lambda: _size(name, size), lambda ts: _forward_only(name, ts))
    dev = render.device
    with torch.cuda.device(dev):
        if not torch.is_tensor(levels):
            levels = torch.full((), min(levels, s), dtype=torch.int32, device=dev)
        out = torch.empty((1, _lib.RSZ_FEATURES + 6, hr, wr), dtype=torch.float32, device=dev)
    r, x, feat, ray, p1, q1, p2, q2 = (_f32(t) for t in tensors)
    _device.call(dev, "ibgs_rsz_features_forward", s, h, w, hr, wr, MODES[mode], r.data_ptr(), x.data_ptr(), feat.data_ptr(), ray.data_ptr(), p1.data_ptr(), q1.data_ptr(),
                 p2.data_ptr(), q2.data_ptr(), levels.data_ptr(), out.data_ptr())
    return out


def upsample_residual(residual, render, render_scale=1.0):
    """residual (3, Hr, Wr) -- the hourglass's output at the reduced resolution; render (3, H, W) (or the exposure-corrected image); render_scale: the
    reference's burned_in_gauss.  -> (residual_up (3, H, W), image_pred (3, H, W)) float32, with image_pred = render_scale * render + residual_up bit for
    bit what torch gives for that expression on the returned residual_up.  Any two sizes go together (Hr = 1 or Wr = 1 included).
    No argument is written; the same arguments give the same bits on every call and stream; nothing waits for the host.  Forward only."""
    name = "upsample_residual"
    hr, wr = _image3(name, "residual", residual)
    h, w = _image3(name, "render", render)
    try:
        render_scale = float(render_scale)
    except (TypeError, ValueError):
        raise TypeError("%s: render_scale must be a number, got %s" % (name, type(render_scale).__name__)) from None
    named = [("residual", residual), ("render", render)]
    _forward_only(name, [t for _, t in named])
    for what, t in named:
        _device.refuse_cpu("resample", "%s's %s" % (name, what), t)
    dev = residual.device
    if render.device != dev:
        raise ValueError("%s: residual is on %s, render on %s" % (name, dev, render.device))
    with torch.cuda.device(dev):
        up = torch.empty((3, h, w), dtype=torch.float32, device=dev)
        image_pred = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    res, r = _f32(residual), _f32(render)
    _device.call(dev, "ibgs_rsz_residual_upsample", h, w, hr, wr, res.data_ptr(), r.data_ptr(), render_scale, up.data_ptr(), image_pred.data_ptr())
    return up, image_pred
