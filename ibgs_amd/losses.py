"""The photometric L1 term of the reference's training step (`l1_loss`, utils/loss_utils.py:23-24; train.py:302) as one pass over the
image: value and gradient together (C ABI `ibgs_l1_loss`, csrc/loss.hip).  Same number as `torch.abs(a - b).mean()`, same gradient
`sign(a - b) / N`; torch needs six small kernels for the pair, ~70 us on a 1080p image.

`ssim` and `ssim_map` are the reference's `ssim` (loss_utils.py:34-64; train.py:302, 355) and `compute_photometric_ssim(..., size_average=False)`
(loss_utils.py:66-91; train.py:330): one kernel forward and one backward (C ABI include/ibgs_ssim.h, csrc/ssim.hip) where torch runs five grouped
11 x 11 convolutions and about twenty element-wise kernels each way.  The contract is a tolerance against a float64 restatement ("Fused SSIM").

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
