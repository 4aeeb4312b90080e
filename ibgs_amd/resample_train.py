"""TRAINING the colour network at a reduced residual resolution (the reference's fuse_color under `residual_resolution_scale != 1`;
color_aggregation_network.py:200-239, train.py:227-228): the two resampling steps of ibgs_amd/resample.py as autograd functions, and the training tail made of
them.  The forwards call resample.py's own entry points (C ABI include/ibgs_resample.h), so their outputs are that module's bit for bit; the backwards are the
adjoint kernels of csrc/rsztrain.hip (C ABI include/ibgs_resample_train.h):

  resized_features_train    `resample.resized_features`, differentiable in render, warped_image and the four parameters of the per-view MLP
  upsample_residual_train   `resample.upsample_residual`, differentiable in residual and render
  fuse_color_train_scaled   `hourglass.fuse_color_train` with the CNN at Hr x Wr = int(H s) x int(W s): the burn-in schedule, the exposure correction if asked
                            for, the level count at FULL resolution, resized_features_train, `hourglass.hourglass_train` there, upsample_residual_train

cam_feat and camera_ray get no gradient (they are data, as in coloragg.py).  Only the groups autograd needs are computed: with render and warped_image
detached the full-resolution gather kernel does not run.  Double backward raises.  The contract is a tolerance against a float64 restatement (DESIGN.md
section 19; tests/resample_train_ref.py); the same arguments give the same bits on every call and stream; nothing waits for the host.

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import torch

from . import _device, _lib
from .coloragg import _f32, _front_end_arguments, _image3, count_levels
from .exposure import correct_package
from .hourglass import _checked_package, _fused, _ray_planes, fuse_color_train, hourglass_train
from .resample import MODES, _size, scaled_size

_ptr = lambda t: None if t is None else t.data_ptr()


def _not_upscaled(name, h, w, hr, wr):
    if hr > h or wr > w:
        raise ValueError("%s: a reduced frame of %d x %d is larger than the frame of %d x %d: training an upscaled network is not supported" % (name, hr, wr, h, w))


class _ResizedFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, warped_image, w1, b1, w2, b2, cam_feat, camera_ray, levels, dims, mode):
        s, h, w, hr, wr = dims
        dev = render.device
        saved = [_f32(t) for t in (render, warped_image, cam_feat, w1, b1, w2, b2)]
        ray = _f32(camera_ray)
        with torch.cuda.device(dev):
            out = torch.empty((1, _lib.RSZ_FEATURES + 6, hr, wr), dtype=torch.float32, device=dev)
        r, x, feat, p1, q1, p2, q2 = saved
        _device.call(dev, "ibgs_rsz_features_forward", s, h, w, hr, wr, mode, r.data_ptr(), x.data_ptr(), feat.data_ptr(), ray.data_ptr(), p1.data_ptr(), q1.data_ptr(),
                     p2.data_ptr(), q2.data_ptr(), levels.data_ptr(), out.data_ptr())
        ctx.dims, ctx.mode = dims, mode
        ctx.shapes = (render.shape, warped_image.shape)
        ctx.save_for_backward(*saved, levels)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad[:6]
        if not any(need):
            return (None,) * 11
        r, x, feat, p1, q1, p2, q2, levels = ctx.saved_tensors
        s, h, w, hr, wr = ctx.dims
        dev = r.device
        go = _f32(grad_out.to(dev))
        with torch.cuda.device(dev):
            # (with render and warped_image detached -- the reference's burn-in -- no image gradient is allocated and the gather kernel does not run)
            grads = [torch.empty_like(t) if k else None for t, k in zip((r, x, p1, q1, p2, q2), need)]
        sc = _device.scratch(dev, _lib.load().ibgs_rzt_required_scratch(s, h, w, hr, wr))
        _device.call(dev, "ibgs_rzt_features_backward", s, h, w, hr, wr, ctx.mode, r.data_ptr(), x.data_ptr(), feat.data_ptr(), p1.data_ptr(), q1.data_ptr(), p2.data_ptr(),
                     q2.data_ptr(), levels.data_ptr(), go.data_ptr(), *[_ptr(g) for g in grads], sc.data_ptr(), sc.numel())
        if grads[0] is not None:
            grads[0] = grads[0].view(ctx.shapes[0])
        if grads[1] is not None:
            grads[1] = grads[1].view(ctx.shapes[1])
        return tuple(grads) + (None,) * 5


def resized_features_train(render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2, size, levels, mode="mean"):
    """`resample.resized_features` for training: the same arguments, the same checks and -- bit for bit -- the same cnn_input (1, 38, Hr, Wr), differentiable in
    render, warped_image (full shape; zero in the slots from `levels` on) and the four parameters.  cam_feat and camera_ray get NO gradient.  size = (Hr, Wr)
    must not exceed the frame's own (H, W): training an upscaled network is refused.  With levels == 0 the parameter gradients and warped_image's are exactly
    zero and render's is the gathered colour gradient alone.  Only the groups autograd needs are computed.  Double backward raises."""
    name = "resized_features_train"
    def reduced():          # (runs after render's shape has been checked, before any tensor's device is)
        hr, wr = _size(name, size)
        _not_upscaled(name, int(render.shape[1]), int(render.shape[2]), hr, wr)
        return hr, wr
    s, h, w, (hr, wr), levels, _ = _front_end_arguments("resample_train", name, render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2, MODES, mode, levels, reduced)
    if not torch.is_tensor(levels):
        with torch.cuda.device(render.device):
            levels = torch.full((), min(levels, s), dtype=torch.int32, device=render.device)
    return _ResizedFeatures.apply(render, warped_image, w1, b1, w2, b2, cam_feat.detach(), camera_ray.detach(), levels, (s, h, w, hr, wr), MODES[mode])


class _UpsampleResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, residual, render, dims, render_scale):
        h, w, hr, wr = dims
        dev = residual.device
        with torch.cuda.device(dev):
            up = torch.empty((3, h, w), dtype=torch.float32, device=dev)
            image_pred = torch.empty((3, h, w), dtype=torch.float32, device=dev)
        res, r = _f32(residual), _f32(render)
        _device.call(dev, "ibgs_rsz_residual_upsample", h, w, hr, wr, res.data_ptr(), r.data_ptr(), render_scale, up.data_ptr(), image_pred.data_ptr())
        ctx.dims, ctx.render_scale = dims, render_scale
        ctx.meta = (residual.shape, residual.dtype, render.dtype, dev)
        ctx.set_materialize_grads(False)          # an output nobody used arrives as None, not as a plane of zeros
        return up, image_pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_up, g_pred):
        if g_up is None and g_pred is None:
            return None, None, None, None
        h, w, hr, wr = ctx.dims
        res_shape, res_dtype, render_dtype, dev = ctx.meta
        g_up = None if g_up is None else _f32(g_up.to(dev))
        g_pred = None if g_pred is None else _f32(g_pred.to(dev))
        g_res = g_render = None
        if ctx.needs_input_grad[0]:
            with torch.cuda.device(dev):
                g_res = torch.empty((3, hr, wr), dtype=torch.float32, device=dev)
            _device.call(dev, "ibgs_rzt_upsample_backward", h, w, hr, wr, _ptr(g_up), _ptr(g_pred), g_res.data_ptr())
            g_res = g_res.view(res_shape).to(res_dtype)
        if ctx.needs_input_grad[1] and g_pred is not None:
            g_render = (ctx.render_scale * g_pred).to(render_dtype)
        return g_res, g_render, None, None


def upsample_residual_train(residual, render, render_scale=1.0):
    """`resample.upsample_residual` for training: -> (residual_up, image_pred), both (3, H, W) float32 and bit for bit that function's, differentiable in
    residual (the adjoint kernel: any two sizes go together) and in render (render_scale times image_pred's gradient).  Double backward raises."""
    name = "upsample_residual_train"
    hr, wr = _image3(name, "residual", residual)
    h, w = _image3(name, "render", render)
    try:
        render_scale = float(render_scale)
    except (TypeError, ValueError):
        raise TypeError("%s: render_scale must be a number, got %s" % (name, type(render_scale).__name__)) from None
    for what, t in (("residual", residual), ("render", render)):
        _device.refuse_cpu("resample_train", "%s's %s" % (name, what), t)
    if render.device != residual.device:
        raise ValueError("%s: residual is on %s, render on %s" % (name, residual.device, render.device))
    return _UpsampleResidual.apply(residual, render, (h, w, hr, wr), render_scale)


def fuse_color_train_scaled(render_pkg, net, residual_resolution_scale, nb_visible_src_frames=3, iter_count=None, burn_start=None, burn_end=None, none_if_no_level=False,
                            enable_exposure_correction=False):
    """The reference's TRAINING fuse_color under `residual_resolution_scale` with a `ColorAggregationNet`, differentiable end to end: in its order the burn-in
    schedule and detaching of `hourglass.fuse_color_train`, the exposure correction if asked for, `count_levels` at FULL resolution,
    `resized_features_train`, `hourglass_train` at Hr x Wr = int(H s) x int(W s), `upsample_residual_train` (which forms image_pred = burned_in_gauss * render
    (or the corrected image) + residual at H x W).  -> the dictionary of `hourglass.fuse_color`: residual is the upsampled (3, H, W) one.
    A scale whose sizes lie outside the hourglass's range, or above the frame's own, raises ValueError before any GPU work.  A scale == 1 returns
    `fuse_color_train(...)` itself: every bit and every key.  Nothing waits for the host unless `none_if_no_level`.
    Inside `with hourglass.train_precision("float16"):` the hourglass is trained in half precision (`hourglass.hourglass_train`); the resized features, the
    exposure correction and the upsampling adjoint stay float32.  Outside such a block every bit is what it was."""
    name = "fuse_color_train_scaled"
    if residual_resolution_scale == 1:
        return fuse_color_train(render_pkg, net, nb_visible_src_frames, iter_count, burn_start, burn_end, none_if_no_level, enable_exposure_correction)
    render, h, w = _checked_package(name, render_pkg, net)
    reduced = scaled_size(h, w, residual_resolution_scale)
    if min(reduced) < _lib.HG_MIN_SIDE or max(reduced) > _lib.HG_MAX_SIDE:
        raise ValueError("%s: residual_resolution_scale %r turns the frame of %d x %d into %d x %d, which is out of the hourglass's range (sides %d .. %d)"
                         % (name, residual_resolution_scale, h, w, reduced[0], reduced[1], _lib.HG_MIN_SIDE, _lib.HG_MAX_SIDE))
    if reduced[0] > h or reduced[1] > w:
        raise ValueError("%s: residual_resolution_scale %r turns the frame of %d x %d into %d x %d: training an upscaled network is not supported"
                         % (name, residual_resolution_scale, h, w, reduced[0], reduced[1]))
    if iter_count is None or burn_start is None or burn_end is None:
        burned = 1.0
    else:
        burned = (max(0.0, min(1.0, (iter_count - burn_start) / (burn_end - burn_start))) + 1) / 2
    warped, cam_feat, camera_ray, min_depth_diff = render_pkg["warped_image"], render_pkg["cam_feat"], render_pkg["camera_ray"], render_pkg["min_depth_diff"]
    if burned < 1.0:          # the gradients to the Gaussians are blocked while the residual is not fully used
        render, warped, cam_feat, camera_ray, min_depth_diff = (t.detach() for t in (render, warped, cam_feat, camera_ray, min_depth_diff))
    camera_ray = _ray_planes(camera_ray, h, w)
    exposure = {}
    if enable_exposure_correction:
        render, exposure["exposure_affine"], exposure["exposure_fit_ok"] = correct_package(name, render_pkg, render, warped)
    levels = count_levels(warped, nb_visible_src_frames)
    front = net.front_end
    cnn_input = resized_features_train(render, warped, cam_feat, camera_ray, front.w1, front.b1, front.w2, front.b2, reduced, levels, front.mode)
    if none_if_no_level and int(levels) == 0:          # (the count is read back: ONE synchronisation, only with this keyword)
        return None
    residual, image_pred = upsample_residual_train(hourglass_train(cnn_input, net.cnn), render, burned)
    return _fused(image_pred, residual, min_depth_diff, burned, levels, warped, nb_visible_src_frames, exposure)
