"""The frame export: the second loop of the reference's render.py (render_set, lines 221-249) on the device.  A rendered frame becomes the 8-bit images a
user looks at -- render, ground truth, aggregated image, normalised residual, colourised depth, normal map -- without leaving the device as float planes:
C ABI include/ibgs_export.h, csrc/export.hip.  Every rule is the reference's float32 arithmetic operation by operation (that header states them;
tests/frame_export_ref.py restates them in numpy), and the contract is equality of every byte:

  to_u8            torchvision's save_image rounding (x * 255, + 0.5, clamp, truncate), or the cv2 branch (clamp to [0, 1], * 255, truncate), RGB or BGR
  normal_to_u8     ((n + 1) / 2 * 255).clip(0, 255), truncated
  residual_vis_u8  |r| / max |r|, then save_image's rounding
  percentile       np.percentile's default rule as numpy 2.x evaluates it for a float32 array, from exact order statistics (a radix select, no sort)
  colorize         the reference's colorize: percentiles 2 and 85 of the valid depths, matplotlib's table lookup, grey where the depth is invalid
  export_frame     all of a view's images into one contiguous uint8 buffer, in one writer launch behind the select chain
  to_host          that buffer's ONE device-to-host copy -- the only place in this module where a value leaves the device
  quantize         save_image's rounding followed by / 255: what reading the PNG back gives (metrics.py:24-34; `image_eval.image_metrics(quantize=True)`)

Stated deviations from the reference: a NaN depth counts as invalid (the reference's percentiles become NaN and the image background); an all-zero residual
gives a zero image and status bit 0 (the reference divides by 0 and casts NaN); no valid depth at all gives percentiles 0 and status bit 1 (np.percentile of
nothing raises); a NaN that reaches a clamp becomes 0.

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import ctypes

import numpy as np
import torch

from . import _device, _lib

MODULE = "frame_export"
ZERO_RESIDUAL, NO_VALID = _lib.FEXP_ZERO_RESIDUAL, _lib.FEXP_NO_VALID
_RULES = {"round": _lib.FEXP_ROUND, "truncate": _lib.FEXP_TRUNCATE}
_LUTS = {}


# ---- argument checks (all of them run before any GPU work) -------------------------------------------------------------------------------------------
def _image(name, what, t, channels):
    """-> (C, H, W) of a float tensor with C in `channels`."""
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor, got %s" % (name, what, type(t).__name__))
    if t.dim() != 3 or t.shape[0] not in channels or not t.is_floating_point():
        raise ValueError("%s: %s must be (%s, H, W) float32, got %s %s" % (name, what, " or ".join(map(str, channels)), tuple(t.shape), t.dtype))
    c, h, w = (int(s) for s in t.shape)
    if h < 1 or w < 1 or h > _lib.FEXP_MAX_SIDE or w > _lib.FEXP_MAX_SIDE or h * w > _lib.FEXP_MAX_PIXELS:
        raise ValueError("%s: %s of %d x %d is empty or out of range (sides 1 .. %d, %d pixels)" % (name, what, h, w, _lib.FEXP_MAX_SIDE, _lib.FEXP_MAX_PIXELS))
    return c, h, w


def _plane(name, what, t):
    """-> (H, W) of a (1, H, W) or (H, W) float tensor."""
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor, got %s" % (name, what, type(t).__name__))
    if t.dim() == 2:
        t = t[None]
    return _image(name, what, t, (1,))[1:]


def _mask(name, mask, shape_numel, shape_text):
    if mask is None:
        return None
    if not torch.is_tensor(mask):
        raise TypeError("%s: invalid_mask must be a tensor, got %s" % (name, type(mask).__name__))
    if mask.numel() != shape_numel or mask.is_floating_point() or mask.is_complex():
        raise ValueError("%s: invalid_mask must hold %s bool or integer values, got %s %s" % (name, shape_text, tuple(mask.shape), mask.dtype))
    return mask


def _mask_bytes(mask):
    if mask is None:
        return None
    m = mask.detach()
    m = m.contiguous().view(torch.uint8) if m.dtype in (torch.bool, torch.uint8) else (m != 0).view(torch.uint8)
    return m.contiguous()


def _number(name, what, x):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise TypeError("%s: %s must be a number, got %s" % (name, what, type(x).__name__)) from None
    return x


def _same_device(name, named):
    for what, t in named:
        _device.refuse_cpu(MODULE, "%s's %s" % (name, what), t)
    for what, t in named[1:]:
        if t.device != named[0][1].device:
            raise ValueError("%s: %s is on %s, %s on %s" % (name, named[0][0], named[0][1].device, what, t.device))


def _f32(t):
    return t.detach().float().contiguous()


def _q32(name, qs):
    try:
        qs = [float(q) for q in qs]
    except TypeError:
        raise TypeError("%s: qs must be a sequence of numbers" % name) from None
    if not 1 <= len(qs) <= _lib.FEXP_MAX_Q:
        raise ValueError("%s: %d percentiles asked for (1 .. %d)" % (name, len(qs), _lib.FEXP_MAX_Q))
    if not all(0.0 <= q <= 100.0 for q in qs):
        raise ValueError("%s: percentiles must lie in [0, 100], got %r" % (name, qs))
    return [np.float32(q) / np.float32(100) for q in qs]          # numpy's own first step, in float32


# ---- one launch chain for any set of images of one size ----------------------------------------------------------------------------------------------
def _run(dev, h, w, images, status, colorize=None):
    """images: [(src float32 contiguous, dst uint8 view, mode, bgr)]; colorize: dict(lut, mask, invalid_val, vmin, vmax, background) for the COLORIZE image."""
    lib = _lib.load()
    f = _lib.FexpFrame()
    f.H, f.W, f.n_images = h, w, len(images)
    for i, (src, dst, mode, bgr) in enumerate(images):
        im = f.images[i]
        im.src, im.dst, im.mode, im.bgr = src.data_ptr(), dst.data_ptr(), mode, int(bgr)
        im.channels = 1 if mode == _lib.FEXP_COLORIZE else src.numel() // (h * w)
    need_arena = any(mode == _lib.FEXP_RESIDUAL for _, _, mode, _ in images)
    keep = None
    if colorize is not None:
        keep = (colorize["lut"], _mask_bytes(colorize["mask"]))
        f.lut = keep[0].data_ptr()
        f.invalid_mask = keep[1].data_ptr() if keep[1] is not None else None
        f.use_invalid_val = colorize["invalid_val"] is not None
        f.invalid_val = colorize["invalid_val"] if colorize["invalid_val"] is not None else 0.0
        f.have_vmin, f.have_vmax = colorize["vmin"] is not None, colorize["vmax"] is not None
        f.vmin = colorize["vmin"] if colorize["vmin"] is not None else 0.0
        f.vmax = colorize["vmax"] if colorize["vmax"] is not None else 0.0
        f.q32[0], f.q32[1] = np.float32(2) / np.float32(100), np.float32(85) / np.float32(100)
        for k in range(3):
            f.background[k] = colorize["background"][k]
        need_arena = need_arena or not (f.have_vmin and f.have_vmax)
    f.status = status.data_ptr()
    arena = None
    if need_arena:
        arena = _device.scratch(dev, lib.ibgs_required_export(h, w))
        f.scratch, f.scratch_bytes = arena.data_ptr(), arena.numel()
    _device.call(dev, "ibgs_fexp_frame_u8", ctypes.byref(f))
    return keep, arena


def _empty(dev, shape, dtype):
    with torch.cuda.device(dev):
        return torch.empty(shape, dtype=dtype, device=dev)


def _single(name, src, h, w, channels, mode, bgr=False, colorize=None):
    dev = src.device
    out = _empty(dev, (h, w, channels), torch.uint8)
    status = _empty(dev, (1,), torch.int32)
    _run(dev, h, w, [(src, out, mode, bgr)], status, colorize)
    return out, status[0]


# ---- the rules ------------------------------------------------------------------------------------------------------------------------------------------
def to_u8(image, rule="round", order="rgb"):
    """image (3, H, W) or (1, H, W) -> (H, W, C) uint8 on the device.  rule "round": torchvision's save_image (t = x * 255; t = t + 0.5; clamp to
    [0, 255]; truncate -- two float32 operations, never one fma); "truncate": the cv2 branch (clamp(x, 0, 1) * 255, truncated).  order "bgr" swaps channels
    0 and 2."""
    name = "to_u8"
    c, h, w = _image(name, "image", image, (1, 3))
    if rule not in _RULES:
        raise ValueError("%s: rule must be 'round' or 'truncate', got %r" % (name, rule))
    if order not in ("rgb", "bgr") or (order == "bgr" and c != 3):
        raise ValueError("%s: order must be 'rgb' or 'bgr' (3 channels), got %r for %d channel(s)" % (name, order, c))
    _same_device(name, [("image", image)])
    return _single(name, _f32(image), h, w, c, _RULES[rule], order == "bgr")[0]


def normal_to_u8(normal):
    """normal (3, H, W) -> (H, W, 3) uint8: ((n + 1) / 2 * 255).clip(0, 255), truncated (render.py:234-237)."""
    name = "normal_to_u8"
    _, h, w = _image(name, "normal", normal, (3,))
    _same_device(name, [("normal", normal)])
    return _single(name, _f32(normal), h, w, 3, _lib.FEXP_NORMAL)[0]


def residual_vis_u8(residual):
    """residual (3, H, W) or (1, H, W) -> ((H, W, C) uint8, status: a 0-d int32 DEVICE tensor).  |r| / max |r| (a correctly rounded float32 division), then
    save_image's rounding.  An all-zero residual gives a zero image and status bit 0 (ZERO_RESIDUAL)."""
    name = "residual_vis_u8"
    c, h, w = _image(name, "residual", residual, (1, 3))
    _same_device(name, [("residual", residual)])
    return _single(name, _f32(residual), h, w, c, _lib.FEXP_RESIDUAL)


def percentile(values, qs, invalid_val=None, invalid_mask=None, return_status=False):
    """values: a float tensor of at most 2^24 elements (any shape); qs: 1 .. 4 numbers in [0, 100].  -> (len(qs),) float32 on the device: np.percentile's
    default (linear) rule as numpy 2.x evaluates it for a float32 array, over the valid values: those that are not NaN, not == invalid_val (when given) and
    whose invalid_mask element (when given) is 0.  No valid value: 0, and status bit 1 (NO_VALID).  return_status: -> (result, status: 0-d int32 device tensor)."""
    name = "percentile"
    if not torch.is_tensor(values):
        raise TypeError("%s: values must be a tensor, got %s" % (name, type(values).__name__))
    if not values.is_floating_point():
        raise ValueError("%s: values must be float32, got %s" % (name, values.dtype))
    n = values.numel()
    if n > _lib.FEXP_MAX_SELECT:
        raise ValueError("%s: %d values (limit: 2^24, so that n - 1 is exact in float32)" % (name, n))
    q32 = _q32(name, qs)
    inv = None if invalid_val is None else _number(name, "invalid_val", invalid_val)
    _mask(name, invalid_mask, n, "%d" % n)
    _same_device(name, [("values", values)] + ([("invalid_mask", invalid_mask)] if invalid_mask is not None else []))
    dev = values.device
    v, m = _f32(values), _mask_bytes(invalid_mask)
    out = _empty(dev, (len(q32),), torch.float32)
    status = _empty(dev, (1,), torch.int32)
    arena = _device.scratch(dev, _lib.load().ibgs_required_export(1, 1))          # (the select's tables: their size does not depend on n)
    _device.call(dev, "ibgs_fexp_percentile", n, v.data_ptr(), m.data_ptr() if m is not None else None, inv is not None, inv if inv is not None else 0.0,
                 len(q32), (ctypes.c_float * len(q32))(*q32), out.data_ptr(), status.data_ptr(), arena.data_ptr(), arena.numel())
    return (out, status[0]) if return_status else out


def colormap_lut(name, device):
    """The (256, 3) uint8 table of a matplotlib colour map on `device`: (matplotlib.colormaps[name](arange(256))[:, :3] * 255).astype(uint8), built once on the
    host per (name, device).  matplotlib is imported here and nowhere else; no table ships with the library."""
    key = (str(name), str(torch.device(device)))
    if key not in _LUTS:
        try:
            import matplotlib
        except ImportError:
            raise ImportError("frame_export.colormap_lut needs matplotlib for the colour table %r; without it pass a (256, 3) uint8 `lut` of your own" % (name,)) from None
        table = (matplotlib.colormaps[str(name)](np.arange(256))[:, :3] * 255).astype(np.uint8)
        _LUTS[key] = torch.from_numpy(np.ascontiguousarray(table)).to(device)
    return _LUTS[key]


def _colorize_args(name, value, lut, vmin, vmax, invalid_val, invalid_mask, background):
    h, w = _plane(name, "value", value)
    if not torch.is_tensor(lut) or tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8:
        raise ValueError("%s: lut must be a (256, 3) uint8 tensor (colormap_lut builds one)" % name)
    try:
        bg = tuple(int(b) for b in background)[:3]
    except (TypeError, ValueError):
        raise TypeError("%s: background must be three integers" % name) from None
    if len(bg) != 3 or not all(0 <= b <= 255 for b in bg):
        raise ValueError("%s: background must be three integers in 0 .. 255, got %r" % (name, background))
    lo = None if vmin is None else float(np.float32(_number(name, "vmin", vmin)))
    hi = None if vmax is None else float(np.float32(_number(name, "vmax", vmax)))
    inv = None if invalid_val is None else _number(name, "invalid_val", invalid_val)
    _mask(name, invalid_mask, h * w, "%d x %d" % (h, w))
    if (lo is None or hi is None) and h * w > _lib.FEXP_MAX_SELECT:
        raise ValueError("%s: percentiles of %d x %d values (limit: 2^24, so that n - 1 is exact in float32)" % (name, h, w))
    return h, w, dict(lut=lut, mask=invalid_mask, invalid_val=inv, vmin=lo, vmax=hi, background=bg)


def colorize(value, lut, vmin=None, vmax=None, invalid_val=-99.0, invalid_mask=None, background=(128, 128, 128), return_status=False):
    """The reference's colorize (utils/general_utils.py:153-184).  value (1, H, W) or (H, W); lut (256, 3) uint8 on the device (`colormap_lut`).
    -> (H, W, 3) uint8.  vmin, vmax: numbers (rounded to float32), or the percentiles 2 and 85 of the valid pixels (`percentile`; H W <= 2^24).
    x = (v - vmin) / (vmax - vmin) where vmin != vmax, else v * 0; matplotlib's lookup of x; `background` where the pixel is invalid.  A given
    invalid_mask REPLACES the test against invalid_val, as in the reference (`percentile` applies both when it is given both)."""
    name = "colorize"
    if invalid_mask is not None:
        invalid_val = None          # general_utils.py:160-161: the comparison is made only without a mask
    h, w, args = _colorize_args(name, value, lut, vmin, vmax, invalid_val, invalid_mask, background)
    _same_device(name, [("value", value), ("lut", lut)] + ([("invalid_mask", invalid_mask)] if invalid_mask is not None else []))
    out, status = _single(name, _f32(value), h, w, 3, _lib.FEXP_COLORIZE, colorize=args)
    return (out, status) if return_status else out


# ---- a whole view -----------------------------------------------------------------------------------------------------------------------------------------
def export_frame(render_pkg, fusion_out=None, gt=None, lut=None, split="test"):
    """render.py:221-249 for one view.  render_pkg: "render" (3, H, W), "median_intersected_depth" (1, H, W), "rendered_normal" (3, H, W); fusion_out: the
    dictionary of fuse_color ("image_pred", "residual") or None; gt (3, H, W) or None; lut: `colormap_lut("magma_r", device)` when None.
    -> a dictionary of (H, W, 3) uint8 DEVICE tensors, all views into ONE contiguous uint8 buffer "packed":
         "render"     save_image's rounding for split "test"; the cv2 branch (truncated, BGR) for "train"
         "gt"         (if given) save_image's rounding
         "aggregate", "residual"   (with fusion_out) image_pred rounded; |residual| / max |residual| rounded
         "depth"      colorize(median_intersected_depth, invalid_val=-99)
         "normal"     normal_to_u8(rendered_normal)
       and "status": a 0-d int32 device view into "packed" (bit 0: the residual is all zero, bit 1: no valid depth), "layout": {name: (offset, shape)}.
    One writer launch behind the select chain; nothing waits for the host."""
    name = "export_frame"
    if split not in ("test", "train"):
        raise ValueError("%s: split must be 'test' or 'train', got %r" % (name, split))
    for key in ("render", "median_intersected_depth", "rendered_normal"):
        if key not in render_pkg:
            raise KeyError("%s: render_pkg lacks %r" % (name, key))
    _, h, w = _image(name, "render_pkg['render']", render_pkg["render"], (3,))
    todo = [("render", render_pkg["render"], _lib.FEXP_ROUND if split == "test" else _lib.FEXP_TRUNCATE, split == "train")]
    if gt is not None:
        todo.append(("gt", gt, _lib.FEXP_ROUND, False))
    if fusion_out is not None:
        for key in ("image_pred", "residual"):
            if key not in fusion_out:
                raise KeyError("%s: fusion_out lacks %r" % (name, key))
        todo += [("aggregate", fusion_out["image_pred"], _lib.FEXP_ROUND, False), ("residual", fusion_out["residual"], _lib.FEXP_RESIDUAL, False)]
    todo.append(("normal", render_pkg["rendered_normal"], _lib.FEXP_NORMAL, False))
    for key, t, _, _ in todo:
        if t is not None and torch.is_tensor(t) and t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if _image(name, key, t, (3,))[1:] != (h, w):
            raise ValueError("%s: %s is %s, render %d x %d" % (name, key, tuple(t.shape), h, w))
    depth = render_pkg["median_intersected_depth"]
    if _plane(name, "median_intersected_depth", depth) != (h, w):
        raise ValueError("%s: median_intersected_depth is %s, render %d x %d" % (name, tuple(depth.shape), h, w))
    if h * w > _lib.FEXP_MAX_SELECT:
        raise ValueError("%s: percentiles of %d x %d values (limit: 2^24, so that n - 1 is exact in float32)" % (name, h, w))
    named = [(key, t) for key, t, _, _ in todo] + [("median_intersected_depth", depth)]
    _same_device(name, named)
    dev = render_pkg["render"].device
    if lut is None:
        lut = colormap_lut("magma_r", dev)
    _, _, cargs = _colorize_args(name, depth, lut, None, None, -99.0, None, (128, 128, 128))
    _same_device(name, [("render", render_pkg["render"]), ("lut", lut)])
    todo.insert(len(todo) - 1, ("depth", depth, _lib.FEXP_COLORIZE, False))
    nbytes = h * w * 3
    step = (nbytes + 3) // 4 * 4          # every image starts on a dword: the writer's stores are dwords
    packed = _empty(dev, (step * len(todo) + 4,), torch.uint8)
    out, images, layout = {}, [], {}
    for i, (key, t, mode, bgr) in enumerate(todo):
        view = packed[i * step:i * step + nbytes].view(h, w, 3)
        if step != nbytes:
            packed[i * step + nbytes:(i + 1) * step].zero_()          # (the bytes between two images: so that the buffer is a function of the frame)
        src = _f32(t[0] if t.dim() == 4 else t)
        images.append((src, view, mode, bgr))
        out[key] = view
        layout[key] = (i * step, (h, w, 3))
    status = packed[step * len(todo):].view(torch.int32)
    _run(dev, h, w, images, status, cargs)
    layout["status"] = (step * len(todo), ())
    out.update(packed=packed, status=status[0], layout=layout)
    return out


def to_host(frame, pinned=None):
    """The ONE device-to-host copy of an `export_frame` result: "packed" into `pinned` (a pinned CPU uint8 tensor of at least that many bytes; allocated when
    None), then a wait for the stream.  -> {name: numpy (H, W, 3) uint8 view into that buffer, "status": int}."""
    name = "to_host"
    packed, layout = frame["packed"], frame["layout"]
    n = packed.numel()
    if pinned is None:
        pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    if not torch.is_tensor(pinned) or pinned.is_cuda or pinned.dtype != torch.uint8 or pinned.dim() != 1 or pinned.numel() < n or not pinned.is_contiguous():
        raise ValueError("%s: pinned must be a contiguous CPU uint8 tensor of at least %d bytes" % (name, n))
    pinned[:n].copy_(packed, non_blocking=True)
    torch.cuda.current_stream(packed.device).synchronize()
    host = pinned.numpy()
    out = {}
    for key, (offset, shape) in layout.items():
        if key == "status":
            out[key] = int(host[offset:offset + 4].view(np.int32)[0])
        else:
            out[key] = host[offset:offset + int(np.prod(shape))].reshape(shape)
    return out


def quantize(image):
    """A float tensor of any shape -> float32, same shape: save_image's rounding to a byte, then / 255 (torchvision's to_tensor): the values metrics.py sees
    after it reads the PNG back."""
    name = "quantize"
    if not torch.is_tensor(image) or not image.is_floating_point():
        raise TypeError("%s: image must be a float tensor" % name)
    if image.numel() < 1:
        raise ValueError("%s: image is empty" % name)
    _device.refuse_cpu(MODULE, "%s's image" % name, image)
    x = _f32(image)
    out = _empty(x.device, tuple(x.shape), torch.float32)
    _device.call(x.device, "ibgs_fexp_quantize", x.numel(), x.data_ptr(), out.data_ptr())
    return out
