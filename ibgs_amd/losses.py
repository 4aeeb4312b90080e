"""The photometric L1 term of the reference's training step (`l1_loss`, utils/loss_utils.py:23-24; train.py:302) as one pass over the
image: value and gradient together (C ABI `ibgs_l1_loss`, csrc/loss.hip).  Same number as `torch.abs(a - b).mean()`, same gradient
`sign(a - b) / N`; torch needs six small kernels for the pair, ~70 us on a 1080p image.

`ssim` and `ssim_map` are the reference's `ssim` (loss_utils.py:34-64; train.py:302, 355) and `compute_photometric_ssim(..., size_average=False)`
(loss_utils.py:66-91; train.py:330): one kernel forward and one backward (C ABI include/ibgs_ssim.h, csrc/ssim.hip) where torch runs five grouped
11 x 11 convolutions and about twenty element-wise kernels each way.  The contract is a tolerance against a float64 restatement ("Fused SSIM").

`photometric_loss` and `normal_consistency` are the multi-view photometric term and the normal-consistency term of the reference's steady-state iteration
(train.py:317-338 and 308-315): one kernel forward and one backward for the first, one pass over the six planes for the second (C ABI
include/ibgs_geo_loss.h, csrc/geoloss.hip).  Neither waits for the device: the count of valid pixels the reference branches on stays there.  The contract is
a tolerance against a float64 restatement.

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import ctypes

import torch

from . import _device, _lib

_scratch = {}


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, store_grad):
        if not image.is_cuda:
            raise RuntimeError("ibgs_amd.losses.l1_loss runs on the MI355X only (no CPU path)")
        if image.shape != target.shape:
            raise ValueError("l1_loss: shapes differ: %s vs %s" % (tuple(image.shape), tuple(target.shape)))
        lib = _lib.load()
        x = image.detach().float().contiguous()
        y = target.detach().to(x.device).float().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device).cuda_stream
            key = (x.device.index, stream)
            sc = _scratch.get(key)
            if sc is None:
                if len(_scratch) > 8:
                    _scratch.clear()
                sc = _scratch[key] = torch.empty(lib.ibgs_required_l1(), dtype=torch.uint8, device=x.device)
            # value AND gradient sign(x - y) / N in the one pass over x and y (when a gradient will be asked for): the backward then only has to
            # scale it by the incoming gradient -- and not even that when the term enters the total with weight one
            # (`store_grad` is the caller's grad mode: needs_input_grad ignores no_grad(), and inside forward() grad mode is always off)
            grad = torch.empty_like(x) if (ctx.needs_input_grad[0] and store_grad) else None
            rc = lib.ibgs_l1_loss(stream, x.numel(), x.data_ptr(), y.data_ptr(), None if grad is None else grad.data_ptr(), loss.data_ptr(), sc.data_ptr(), sc.numel())
        if rc < 0:
            raise RuntimeError("ibgs_l1_loss failed (%d): %s" % (rc, _lib.last_error()))
        ctx.save_for_backward(x, y)
        ctx.unit_grad = grad          # consumed (scaled in place) by the first backward
        ctx.shape = image.shape
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        x, y = ctx.saved_tensors
        lib = _lib.load()
        go = grad_out.detach().to(x.device).float().contiguous()
        grad, ctx.unit_grad = ctx.unit_grad, None
        if grad is not None:
            with torch.cuda.device(x.device):
                rc = lib.ibgs_l1_rescale(torch.cuda.current_stream(x.device).cuda_stream, grad.numel(), grad.data_ptr(), go.data_ptr())
            if rc < 0:
                raise RuntimeError("ibgs_l1_rescale failed (%d): %s" % (rc, _lib.last_error()))
            return grad.view(ctx.shape), None, None
        grad = torch.empty_like(x)          # a second backward through the same node (retain_graph): from x and y again
        with torch.cuda.device(x.device):
            # sign(x - y) * grad_out / N in ONE pass: the incoming gradient is read on the device (no host sync, no separate multiply)
            rc = lib.ibgs_l1_grad(torch.cuda.current_stream(x.device).cuda_stream, x.numel(), x.data_ptr(), y.data_ptr(), go.data_ptr(), grad.data_ptr())
        if rc < 0:
            raise RuntimeError("ibgs_l1_grad failed (%d): %s" % (rc, _lib.last_error()))
        return grad.view(ctx.shape), None, None      # (the target's gradient is never asked for by the trainer)


def l1_loss(network_output, gt):
    """Drop-in for the reference's `l1_loss(network_output, gt)`: mean absolute difference, differentiable in `network_output`."""
    if network_output.numel() == 0:
        return torch.abs(network_output - gt).mean()
    return _L1.apply(network_output, gt, torch.is_grad_enabled())


# ---- SSIM ----------------------------------------------------------------------------------------------------------------------------------------
def ssim_tile():
    """(TILE_H, TILE_W): the tile of one workgroup of the SSIM kernels."""
    th, tw = ctypes.c_int32(), ctypes.c_int32()
    _lib.load().ibgs_ssim_tile(ctypes.byref(th), ctypes.byref(tw))
    return th.value, tw.value


def _ssim_check(name, img1, img2, window_size, dims):
    """Every argument check of the SSIM entry points, before any GPU work.  -> (N, C, H, W) of the call."""
    if window_size != 11:
        raise ValueError("%s: window_size must be 11 (the only size the kernels have), got %r" % (name, window_size))
    if not (torch.is_tensor(img1) and torch.is_tensor(img2)):
        raise TypeError("%s: the images must be tensors" % name)
    if img1.shape != img2.shape:
        raise ValueError("%s: shapes differ: %s vs %s" % (name, tuple(img1.shape), tuple(img2.shape)))
    if img1.dim() not in dims:
        raise ValueError("%s: %s input expected, got %s" % (name, " or ".join("%d-D" % d for d in dims), tuple(img1.shape)))
    n, c, h, w = ((1,) + tuple(img1.shape))[-4:]
    if n * c * h * w == 0:
        raise ValueError("%s: empty image %s" % (name, tuple(img1.shape)))
    if h > _lib.SSIM_MAX_SIDE or w > _lib.SSIM_MAX_SIDE:
        raise ValueError("%s: image %s too large (sides <= %d)" % (name, tuple(img1.shape), _lib.SSIM_MAX_SIDE))
    _device.refuse_cpu("losses", name + "'s img1", img1)
    _device.refuse_cpu("losses", name + "'s img2", img2)
    if img1.device != img2.device:
        raise ValueError("%s: img1 is on %s, img2 on %s" % (name, img1.device, img2.device))
    return n, c, h, w


def _ssim_forward(dims, x, y, map_out=None, dmaps=None, mean=None, per_image=None, mse=None, l1=None, l1_per_image=None):
    """One ibgs_ssim_forward on x's device and torch's current stream there."""
    ptr = lambda t: None if t is None else t.data_ptr()
    sc = None
    if any(t is not None for t in (mean, per_image, mse, l1, l1_per_image)):
        sc = _device.scratch(x.device, _lib.load().ibgs_ssim_required_scratch(dims[0] * dims[1], dims[2], dims[3]))
    _device.call(x.device, "ibgs_ssim_forward", *dims, x.data_ptr(), y.data_ptr(), ptr(map_out), ptr(dmaps), ptr(mean), ptr(per_image), ptr(mse), ptr(l1), ptr(l1_per_image),
                 ptr(sc), 0 if sc is None else sc.numel())


def _ssim_dmaps(dims, a, b, map_out=None, **sums):
    """The derivative planes of m(a, b) with respect to a's statistics (and whatever else the same launch is asked for)."""
    with torch.cuda.device(a.device):
        d = torch.empty((3,) + tuple(a.shape), dtype=torch.float32, device=a.device)
    _ssim_forward(dims, a, b, map_out=map_out, dmaps=d, **sums)
    return d


def _ssim_backward(dims, a, b, dmaps, plane_scale, grad_map):
    with torch.cuda.device(a.device):
        g = torch.empty_like(a)
    _device.call(a.device, "ibgs_ssim_backward", *dims, a.data_ptr(), b.data_ptr(), dmaps.data_ptr(), None if plane_scale is None else plane_scale.data_ptr(),
                 None if grad_map is None else grad_map.data_ptr(), g.data_ptr())
    return g


def _ssim_setup(ctx, dims, img1, img2, store_grad, map_out, **sums):
    """The forward launches of both Functions: one, or two when both images will be asked for a gradient (m is bit-symmetric in its arguments, so the
    second launch only adds the derivative planes of the other side)."""
    x = img1.detach().float().contiguous()
    y = img2.detach().float().contiguous()
    # (`store_grad` is the caller's grad mode: needs_input_grad ignores no_grad(), and inside forward() grad mode is always off)
    need1, need2 = store_grad and ctx.needs_input_grad[0], store_grad and ctx.needs_input_grad[1]
    d1 = d2 = None
    if need1:
        d1 = _ssim_dmaps(dims, x, y, map_out=map_out, **sums)
    if need2:
        d2 = _ssim_dmaps(dims, y, x) if need1 else _ssim_dmaps(dims, y, x, map_out=map_out, **sums)
    if not (need1 or need2):
        _ssim_forward(dims, x, y, map_out=map_out, **sums)
    ctx.dims, ctx.shape = dims, img1.shape
    ctx.has = (d1 is not None, d2 is not None)
    ctx.save_for_backward(x, y, *[d for d in (d1, d2) if d is not None])


def _ssim_grads(ctx, plane_scale, grad_map):
    x, y = ctx.saved_tensors[:2]
    rest = list(ctx.saved_tensors[2:])
    d1 = rest.pop(0) if ctx.has[0] else None
    d2 = rest.pop(0) if ctx.has[1] else None
    g1 = g2 = None
    if ctx.needs_input_grad[0]:
        if d1 is None:
            raise RuntimeError("ssim: the gradient of img1 was not prepared (the forward ran under no_grad or img1 did not require grad)")
        g1 = _ssim_backward(ctx.dims, x, y, d1, plane_scale, grad_map).view(ctx.shape)
    if ctx.needs_input_grad[1]:
        if d2 is None:
            raise RuntimeError("ssim: the gradient of img2 was not prepared (the forward ran under no_grad or img2 did not require grad)")
        g2 = _ssim_backward(ctx.dims, y, x, d2, plane_scale, grad_map).view(ctx.shape)
    return g1, g2


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, dims, per_image, store_grad):
        dev = img1.device
        with torch.cuda.device(dev):
            mean = torch.empty((), dtype=torch.float32, device=dev)
            per = torch.empty(dims[0], dtype=torch.float32, device=dev) if per_image else None
        _ssim_setup(ctx, dims, img1, img2, store_grad, None, mean=mean, per_image=per)
        ctx.per_image = per_image
        return per if per_image else mean

    @staticmethod
    def backward(ctx, grad_out):
        n, c, h, w = ctx.dims
        go = grad_out.detach().to(ctx.saved_tensors[0].device).float()
        # G is constant over a plane: the incoming gradient over the pixels it was averaged over, formed on the device (no host sync)
        if ctx.per_image:
            scale = (go / float(c * h * w)).repeat_interleave(c).contiguous()
        else:
            scale = (go / float(n * c * h * w)).reshape(1).expand(n * c).contiguous()
        return _ssim_grads(ctx, scale, None) + (None, None, None)


class _SSIMMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, dims, store_grad):
        with torch.cuda.device(img1.device):
            out = torch.empty(tuple(img1.shape), dtype=torch.float32, device=img1.device)
        _ssim_setup(ctx, dims, img1, img2, store_grad, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        go = grad_out.detach().to(ctx.saved_tensors[0].device).float().contiguous()
        return _ssim_grads(ctx, None, go) + (None, None)


def ssim(img1, img2, window_size=11, size_average=True):
    """Drop-in for the reference's `ssim(img1, img2, window_size=11, size_average=True)`: (C, H, W) or (N, C, H, W) images; the mean of the SSIM map over
    everything, or with size_average=False (4-D input only) the (N,) means per image.  Differentiable in either or both images."""
    dims = _ssim_check("ssim", img1, img2, window_size, (3, 4) if size_average else (4,))
    return _SSIM.apply(img1, img2, dims, not size_average, torch.is_grad_enabled())


def ssim_map(img1, img2, window_size=11):
    """Drop-in for the reference's `compute_photometric_ssim(img1, img2, size_average=False)`: the SSIM map in the input's shape ((C, H, W) or (N, C, H, W)),
    differentiable in either or both images under any upstream gradient."""
    dims = _ssim_check("ssim_map", img1, img2, window_size, (3, 4))
    return _SSIMMap.apply(img1, img2, dims, torch.is_grad_enabled())


# ---- the geometry loss terms -----------------------------------------------------------------------------------------------------------------------
def geoloss_tile():
    """(TILE_H, TILE_W): the tile of one workgroup of the photometric kernels."""
    th, tw = ctypes.c_int32(), ctypes.c_int32()
    _lib.load().ibgs_geoloss_tile(ctypes.byref(th), ctypes.byref(tw))
    return th.value, tw.value


def _planes_check(name, what, t, per_source, h, w):
    """t: (per_source * S_total, H, W) or (S_total, per_source, H, W) -> S_total."""
    if t.dim() == 3 and t.shape[0] % per_source == 0:
        total = t.shape[0] // per_source
    elif t.dim() == 4 and t.shape[1] == per_source:
        total = t.shape[0]
    else:
        raise ValueError("%s: %s must be (%d S, H, W) or (S, %d, H, W), got %s" % (name, what, per_source, per_source, tuple(t.shape)))
    if not 1 <= total <= _lib.GEOLOSS_MAX_SRC:
        raise ValueError("%s: %s holds %d sources (1 .. %d)" % (name, what, total, _lib.GEOLOSS_MAX_SRC))
    if tuple(t.shape[-2:]) != (h, w):
        raise ValueError("%s: %s is %d x %d, gt_image %d x %d" % (name, what, t.shape[-2], t.shape[-1], h, w))
    return total


def _image3_check(name, what, t):
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor" % (name, what))
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError("%s: %s must be (3, H, W), got %s" % (name, what, tuple(t.shape)))
    h, w = int(t.shape[1]), int(t.shape[2])
    if h * w == 0:
        raise ValueError("%s: empty image %s" % (name, tuple(t.shape)))
    if h > _lib.GEOLOSS_MAX_SIDE or w > _lib.GEOLOSS_MAX_SIDE:
        raise ValueError("%s: image %s too large (sides <= %d)" % (name, tuple(t.shape), _lib.GEOLOSS_MAX_SIDE))
    return h, w


def _one_device(name, *named):
    for what, t in named:
        _device.refuse_cpu("losses", "%s's %s" % (name, what), t)
    for what, t in named[1:]:
        if t.device != named[0][1].device:
            raise ValueError("%s: %s is on %s, %s on %s" % (name, named[0][0], named[0][1].device, what, t.device))


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, warped_image, gt_image, cam_feat, dims, weights, store_grad):
        s, s_total, h, w = dims
        dev = warped_image.device
        x = warped_image.detach().float().contiguous()
        gt = gt_image.detach().float().contiguous()
        feat = cam_feat.detach().float().contiguous()
        # (`store_grad` is the caller's grad mode: needs_input_grad ignores no_grad(), and inside forward() grad mode is always off)
        need = store_grad and ctx.needs_input_grad[0]
        with torch.cuda.device(dev):
            loss = torch.empty((), dtype=torch.float32, device=dev)
            nv = torch.empty((), dtype=torch.float64, device=dev)
            d = torch.empty((3, s, 3, h, w), dtype=torch.float32, device=dev) if need else None
        sc = _device.scratch(dev, _lib.load().ibgs_geoloss_required_scratch(s, h, w))
        _device.call(dev, "ibgs_geoloss_photo_forward", s, h, w, gt.data_ptr(), x.data_ptr(), feat.data_ptr(), weights[0], weights[1],
                     None if d is None else d.data_ptr(), loss.data_ptr(), nv.data_ptr(), sc.data_ptr(), sc.numel())
        ctx.dims, ctx.weights, ctx.shape = dims, weights, warped_image.shape
        ctx.prepared = need
        if need:
            ctx.save_for_backward(x, gt, feat, d, nv)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        if not ctx.prepared:
            raise RuntimeError("photometric_loss: the gradient of warped_image was not prepared (the forward ran under no_grad)")
        x, gt, feat, d, nv = ctx.saved_tensors
        s, s_total, h, w = ctx.dims
        go = grad_out.detach().to(x.device).float().contiguous()          # a device scalar: read there, no host sync
        with torch.cuda.device(x.device):
            g = torch.empty_like(x)
        _device.call(x.device, "ibgs_geoloss_photo_backward", s, s_total, h, w, gt.data_ptr(), x.data_ptr(), feat.data_ptr(), d.data_ptr(), nv.data_ptr(), go.data_ptr(),
                     ctx.weights[0], ctx.weights[1], g.data_ptr())
        return g.view(ctx.shape), None, None, None, None, None


def photometric_loss(gt_image, warped_image, cam_feat, nb_visible_src_frames=3, photo_weight=0.3, photo_ssim_weight=1.0):
    """The multi-view photometric term of train.py:319-338 on the rasterizer's outputs taken whole: gt_image (3, H, W); warped_image (3 S_total, H, W) or
    (S_total, 3, H, W); cam_feat (4 S_total, H, W) or (S_total, 4, H, W).  The first min(nb_visible_src_frames, S_total) sources are read.  -> a 0-d float32
    tensor, exactly 0 when no pixel is valid (decided on the device).  Differentiable in warped_image only; the gradient has its full shape."""
    name = "photometric_loss"
    h, w = _image3_check(name, "gt_image", gt_image)
    for what, t in (("warped_image", warped_image), ("cam_feat", cam_feat)):
        if not torch.is_tensor(t):
            raise TypeError("%s: %s must be a tensor" % (name, what))
    s_total = _planes_check(name, "warped_image", warped_image, 3, h, w)
    if _planes_check(name, "cam_feat", cam_feat, 4, h, w) != s_total:
        raise ValueError("%s: warped_image holds %d sources, cam_feat %d" % (name, s_total, _planes_check(name, "cam_feat", cam_feat, 4, h, w)))
    if int(nb_visible_src_frames) != nb_visible_src_frames or nb_visible_src_frames < 1:
        raise ValueError("%s: nb_visible_src_frames must be a positive integer, got %r" % (name, nb_visible_src_frames))
    weights = (float(photo_weight), float(photo_ssim_weight))
    if not all(abs(x) < 1e30 for x in weights):          # (NaN fails too)
        raise ValueError("%s: the weights must be finite, got %r" % (name, weights))
    if gt_image.requires_grad:
        raise ValueError("%s: gt_image requires grad; the term is differentiable in warped_image only" % name)
    _one_device(name, ("warped_image", warped_image), ("gt_image", gt_image), ("cam_feat", cam_feat))
    dims = (min(int(nb_visible_src_frames), s_total), s_total, h, w)
    return _Photometric.apply(warped_image, gt_image, cam_feat.detach(), dims, weights, torch.is_grad_enabled())


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def _launch(n, dn, weight, want):
        """-> (loss, unit gradient of n or None, of dn or None) from one pass."""
        dev = n.device
        h, w = n.shape[1:]
        with torch.cuda.device(dev):
            loss = torch.empty((), dtype=torch.float32, device=dev)
            g = [torch.empty_like(n) if k else None for k in want]
        sc = _device.scratch(dev, _lib.load().ibgs_geoloss_required_scratch(1, h, w))
        _device.call(dev, "ibgs_geoloss_normal_forward", h, w, n.data_ptr(), dn.data_ptr(), weight, None if g[0] is None else g[0].data_ptr(),
                     None if g[1] is None else g[1].data_ptr(), loss.data_ptr(), sc.data_ptr(), sc.numel())
        return loss, g[0], g[1]

    @staticmethod
    def forward(ctx, rendered_normal, depth_normal, weight, store_grad):
        n = rendered_normal.detach().float().contiguous()
        dn = depth_normal.detach().float().contiguous()
        # value AND both unit gradients in the one pass (when a gradient will be asked for), as l1_loss does
        want = tuple(bool(store_grad and k) for k in ctx.needs_input_grad[:2])
        loss, g_n, g_dn = _NormalConsistency._launch(n, dn, weight, want)
        ctx.save_for_backward(n, dn)
        ctx.unit = (g_n, g_dn)          # consumed (scaled in place) by the first backward
        ctx.weight, ctx.shapes = weight, (rendered_normal.shape, depth_normal.shape)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        n, dn = ctx.saved_tensors
        want = tuple(bool(k) for k in ctx.needs_input_grad[:2])
        unit, ctx.unit = ctx.unit, (None, None)
        if any(k and u is None for k, u in zip(want, unit)):          # a second backward through the same node (retain_graph): from n and dn again
            unit = _NormalConsistency._launch(n, dn, ctx.weight, want)[1:]
        go = grad_out.detach().to(n.device).float().contiguous()
        out = []
        for k, u, shape in zip(want, unit, ctx.shapes):
            if not k:
                out.append(None)
                continue
            _device.call(n.device, "ibgs_geoloss_rescale", u.numel(), u.data_ptr(), go.data_ptr())
            out.append(u.view(shape))
        return out[0], out[1], None, None


def normal_consistency(rendered_normal, depth_normal, weight=0.03):
    """The single-view normal term of train.py:310-315: weight (0.4 mean_p sum_c |dn - n| + 0.6 mean_p (1 - sum_c dn n)) for two (3, H, W) images.
    -> a 0-d float32 tensor, differentiable in both."""
    name = "normal_consistency"
    h, w = _image3_check(name, "rendered_normal", rendered_normal)
    if (h, w) != _image3_check(name, "depth_normal", depth_normal):
        raise ValueError("%s: shapes differ: %s vs %s" % (name, tuple(rendered_normal.shape), tuple(depth_normal.shape)))
    weight = float(weight)
    if not abs(weight) < 1e30:
        raise ValueError("%s: weight must be finite, got %r" % (name, weight))
    _one_device(name, ("rendered_normal", rendered_normal), ("depth_normal", depth_normal))
    return _NormalConsistency.apply(rendered_normal, depth_normal, weight, torch.is_grad_enabled())
