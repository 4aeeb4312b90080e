"""The exposure correction of the reference's fuse_color (color_aggregation_network.py:136-153, 182-185; `--enable_exposure_correction`): a 3 x 4 affine colour
map fitted by least squares on the pixels where `use_first_src_frame_mask == 1`, taking the rendered image onto the first warped source image, and that map
applied to the whole rendered image -- four launches (moments, solve, apply; the apply again for the gradient) of C ABI include/ibgs_exposure.h,
csrc/exposure.hip.  The corrected image takes the place of `render` in everything fuse_color does afterwards (`coloragg.fuse_color_inputs`,
`hourglass.fuse_color`, `hourglass.fuse_color_train`: keyword `enable_exposure_correction`).

  A = argmin sum over {mask == 1} |A [r; 1] - s|^2          r = render, s = slot 0 of warped_image; sums and solve in float64 on the device
  corrected[i] = A[i,0] r0 + A[i,1] r1 + A[i,2] r2 + A[i,3]  at every pixel, float32
  d render[j]  = sum_i A[i,j] g[i]                           A is a constant (the reference fits it under torch.no_grad())

Where the reference's fit is not defined (`gels` on a rank-deficient system) this one is declared UNDETERMINED: fewer than 4 pixels take part, or their
colours do not span three dimensions.  Then A = [I | 0], fit_ok = 0 and corrected is render bit for bit.  The contract is a tolerance against a float64
restatement (tests/exposure_ref.py).

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import torch

from . import _device, _lib
from .coloragg import _f32, _image3, _planes


class _Correct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, first_warped, mask, dims):
        h, w = dims
        dev = render.device
        r, x, m = _f32(render), _f32(first_warped), mask.detach().contiguous()
        with torch.cuda.device(dev):
            corrected = torch.empty((3, h, w), dtype=torch.float32, device=dev)
            affine = torch.empty((3, 4), dtype=torch.float32, device=dev)
            fit_ok = torch.empty((), dtype=torch.int32, device=dev)
        sc = _device.scratch(dev, _lib.load().ibgs_expo_required_scratch(h, w))
        _device.call(dev, "ibgs_expo_fit", h, w, r.data_ptr(), x.data_ptr(), m.data_ptr(), affine.data_ptr(), fit_ok.data_ptr(), sc.data_ptr(), sc.numel(), _lib.EXPO_FIT)
        _device.call(dev, "ibgs_expo_apply", h, w, affine.data_ptr(), fit_ok.data_ptr(), r.data_ptr(), corrected.data_ptr())
        ctx.dims, ctx.shape, ctx.dtype = dims, render.shape, render.dtype
        ctx.save_for_backward(affine, fit_ok)
        ctx.mark_non_differentiable(affine, fit_ok)
        return corrected, affine, fit_ok

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_corrected, _grad_affine, _grad_ok):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        affine, fit_ok = ctx.saved_tensors
        h, w = ctx.dims
        dev = affine.device
        g = _f32(grad_corrected.to(dev))
        with torch.cuda.device(dev):
            grad = torch.empty_like(g)
        _device.call(dev, "ibgs_expo_apply_backward", h, w, affine.data_ptr(), fit_ok.data_ptr(), g.data_ptr(), grad.data_ptr())
        return grad.view(ctx.shape).to(ctx.dtype), None, None, None


def exposure_correct(render, warped_image, use_first_src_frame_mask):
    """render (3, H, W); warped_image (3 S, H, W) or (S, 3, H, W), 1 <= S <= 5, of which only slot 0 is read; use_first_src_frame_mask (1, H, W) or (H, W),
    int32 as the rasterizer writes it: a pixel takes part in the fit iff its word is 1.
    -> (corrected (3, H, W) float32, affine (3, 4) float32, fit_ok: a 0-d int32 DEVICE tensor, 1 or 0).

    With fit_ok == 0 (fewer than 4 pixels under the mask, or colours there that do not span three dimensions: a constant colour, a channel that copies
    another) affine is [I | 0] and corrected equals render bit for bit; the reference's `lstsq` returns something undefined there.  Values of render and
    warped_image outside the mask, NaN included, do not reach affine.

    Differentiable in render only, with affine as a constant (the reference fits it under torch.no_grad()): warped_image and the mask get no gradient.
    Inputs of another float type or with other strides are converted; no argument is written.  The same arguments give the same bits on every call and
    stream; nothing waits for the host."""
    name = "exposure_correct"
    h, w = _image3(name, "render", render)
    _planes(name, "warped_image", warped_image, 3, h, w)
    mask = use_first_src_frame_mask
    if not torch.is_tensor(mask):
        raise TypeError("%s: use_first_src_frame_mask must be a tensor" % name)
    if tuple(mask.shape) not in ((1, h, w), (h, w)):
        raise ValueError("%s: use_first_src_frame_mask must be (1, %d, %d) or (%d, %d), got %s" % (name, h, w, h, w, tuple(mask.shape)))
    if mask.dtype != torch.int32:
        raise ValueError("%s: use_first_src_frame_mask must be int32 (the rasterizer's plane), got %s" % (name, mask.dtype))
    named = [("render", render), ("warped_image", warped_image), ("use_first_src_frame_mask", mask)]
    for what, t in named:
        _device.refuse_cpu("exposure", "%s's %s" % (name, what), t)
    for what, t in named[1:]:
        if t.device != render.device:
            raise ValueError("%s: render is on %s, %s on %s" % (name, render.device, what, t.device))
    first = warped_image[:3] if warped_image.dim() == 3 else warped_image[0]
    return _Correct.apply(render, first.detach(), mask, (h, w))


def correct_package(name, render_pkg, render, warped_image):
    """The step inside the fuse_color entry points (`name`: the caller's, for the message): -> (corrected, affine, fit_ok) from render_pkg's mask."""
    if "use_first_src_frame_mask" not in render_pkg:
        raise KeyError("%s: render_pkg lacks 'use_first_src_frame_mask' (enable_exposure_correction needs the rasterizer's mask)" % name)
    return exposure_correct(render, warped_image, render_pkg["use_first_src_frame_mask"])
