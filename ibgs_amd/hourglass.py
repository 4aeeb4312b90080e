"""The hourglass CNN of the reference's colour aggregation network for test-time rendering (color_aggregation_network.py:6-68, 229-250; render.py:137-147):
from the (1, 38, H, W) tensor of `coloragg.fuse_color_inputs` to `residual` and `image_pred`, as seven launches of one matrix-core kernel (C ABI
include/ibgs_hourglass.h, csrc/hourglass.hip).  With `ColorAggregationNet` and `fuse_color` the whole test-time tail -- rasterizer outputs in, image_pred
out -- runs on this library's kernels, and a `ColorFusionResidualNet` checkpoint loads unchanged.

  e1 = relu(conv3(x; enc1 38 -> 38));  e2 = relu(conv3(pool(e1); enc2 38 -> 19));  b = relu(conv3(pool(e2); enc3 19 -> 9))
  u2 = relu(conv3(up(b); up2_conv 9 -> 19));  d2 = relu(conv3([u2, e2]; dec2 38 -> 19));  u1 = relu(conv3(up(d2); up1_conv 19 -> 38))
  d1 = relu(conv3([u1, e1]; dec1 76 -> 38));  f = relu(conv1([d1, x]; fuse_input 76 -> 38));  residual = conv1(f; final 38 -> 3)
  image_pred = burned_in_gauss * render + residual          (render = channels 35 .. 37 of x)

FORWARD ONLY (inference, under torch.no_grad()), hidden_dim 38, float32 by default.  `precision="float16"` selects the half-precision forward (C ABI
include/ibgs_hg_half.h, csrc/hghalf.hip): the roundings of the reference's test-time run under torch.autocast(float16), on the f16 matrix-core instruction.
Training (`hourglass_train`, `fuse_color_train`) runs in float32 or, with `precision="float16"` / inside `train_precision("float16")`, in half precision on the same instruction (C ABI
include/ibgs_hg_half_train.h, csrc/hghtrain.hip).  The contract is a tolerance against a float64 restatement (tests/hourglass_ref.py).

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import contextlib
import threading

import torch
from torch import nn

from . import _device, _lib
from .coloragg import PerViewFrontEnd, _f32
from .exposure import correct_package
from .resample import count_levels, resized_features, scaled_size, upsample_residual

C = _lib.HG_CHANNELS
# the nine convolutions in the order of the C ABI: (name, Cout, Cin, kernel side)
LAYERS = (("enc1", C, C, 3), ("enc2", C // 2, C, 3), ("enc3", C // 4, C // 2, 3), ("up2_conv", C // 2, C // 4, 3), ("dec2", C // 2, 2 * (C // 2), 3),
          ("up1_conv", C, C // 2, 3), ("dec1", C, 2 * C, 3), ("fuse_input", C, 2 * C, 1), ("final", 3, C, 1))
# the reference's names of the eighteen parameters inside ConvDecoderAE -> this module's
REFERENCE_KEYS = {}
for _name, _, _, _ in LAYERS:
    _theirs = _name if _name == "final" else _name + ".0"
    REFERENCE_KEYS[_theirs + ".weight"] = _name + "_w"
    REFERENCE_KEYS[_theirs + ".bias"] = _name + "_b"
# the intermediates of the arena (include/ibgs_hourglass.h), in its order: (name, channels, resolution level)
STAGES = (("e1", C, 0), ("e2", C // 2, 1), ("b", C // 4, 2), ("u2", C // 2, 1), ("d2", C // 2, 1), ("u1", C, 0))


def _arena_views(arena, h, w, half=False):
    """The six stages inside the arena of a forward, (channels, h, w) views each: float32 planes (include/ibgs_hourglass.h), or with `half` pixel-major binary16
    with the channels padded to a multiple of 8, after h(x) (include/ibgs_hg_half.h).  Every entry starts at the next multiple of 128 bytes."""
    sides = ((h, w), (h // 2, w // 2), (h // 2 // 2, w // 2 // 2))
    dtype, size, pad = (torch.float16, 2, 8) if half else (torch.float32, 4, 1)
    out, at = {}, 0
    for name, ch, level in ((("xh", C, 0),) if half else ()) + STAGES:
        hh, ww = sides[level]
        at = (at + 127) // 128 * 128
        cp = (ch + pad - 1) // pad * pad
        n = cp * hh * ww * size
        flat = arena[at:at + n].view(dtype)
        out[name] = flat.view(hh, ww, cp).permute(2, 0, 1)[:ch] if half else flat.view(ch, hh, ww)
        at += n
    out.pop("xh", None)
    return out


PRECISIONS = ("float32", "float16")


def _check_precision(name, precision):
    if precision not in PRECISIONS:
        raise ValueError("%s: precision must be \"float32\" or \"float16\", got %r" % (name, precision))


_TRAINING = threading.local()          # .precision: what `train_precision` set on this thread


@contextlib.contextmanager
def train_precision(precision):
    """`with train_precision("float16"):` -- the training calls made inside the block on this thread (`hourglass_train`, `fuse_color_train`,
    `resample_train.fuse_color_train_scaled`) build their forward in that precision, as torch.autocast does for torch's ops; a graph built inside keeps its
    precision when its backward runs outside.  `hourglass_train(..., precision=...)` overrides it for one call.  The test-time calls have their own keyword
    and `hourglass_backward` its own option: neither looks here.  Outside a block, and by default, training is float32 and every call keeps its bits."""
    _check_precision("train_precision", precision)
    before = getattr(_TRAINING, "precision", "float32")
    _TRAINING.precision = precision
    try:
        yield
    finally:
        _TRAINING.precision = before


def _options(name, given, allowed):
    """The keyword-only options of a training call: anything else is the TypeError Python itself would raise.  -> `given`"""
    for key in given:
        if key not in allowed:
            raise TypeError("%s() got an unexpected keyword argument %r" % (name, key))
    return given


def hourglass_forward(cnn_input, params, render_scale=None, return_stages=False, precision="float32"):
    """cnn_input: (1, 38, H, W) or (38, H, W), any strides, 4 <= H, W <= 8192; params: a `HourglassCNN`.  -> residual (3, H, W) float32.

    With `render_scale=float` (the reference's burned_in_gauss) -> (residual, image_pred) with image_pred = render_scale * cnn_input[35:38] + residual,
    formed in the last kernel: bit for bit what torch gives for that expression on the returned residual.
    With `return_stages` a dict of the intermediates e1, e2, b, u2, d2, u1 is returned last: VIEWS into the call's arena, (channels, h, w) each, valid until
    the next call on that device (a caller who keeps one longer clones it).
    `precision`: "float32" (every call without the keyword keeps its bits) or "float16": x, the weights, the biases and the eight ReLU stages rounded to
    binary16, float32 accumulation on the f16 matrix-core instruction, the residual left in float32 and image_pred formed from the unrounded input -- the
    roundings of the reference's autocast run but for the last.  The outputs are float32 either way; the stages are then float16 views (any strides).

    Forward only: with grad mode enabled and an input or parameter that requires grad this raises -- call it under torch.no_grad(); training keeps
    torch's CNN behind coloragg.fuse_color_inputs.  Nothing waits for the host."""
    name = "hourglass_forward"
    _check_precision(name, precision)
    x, h, w, tensors = _checked(name, cnn_input, params)
    if render_scale is not None:
        render_scale = float(render_scale)
    if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for _, t in tensors)):
        raise RuntimeError("%s is forward only: call it under torch.no_grad() (an input or parameter requires grad and grad mode is on); training keeps "
                           "torch's CNN behind coloragg.fuse_color_inputs" % name)
    _on_one_device(name, x, tensors)
    half = precision == "float16"
    arena = _device.scratch(x.device, (_lib.load().ibgs_hgh_required_scratch if half else _lib.load().ibgs_hg_required_scratch)(h, w))
    residual, image_pred = _forward_call(x.device, h, w, _f32(x), [_f32(t) for _, t in tensors], render_scale, arena, half)
    out = (residual,) if image_pred is None else (residual, image_pred)
    if return_stages:
        out += (_arena_views(arena, h, w, half),)
    return out[0] if len(out) == 1 else out


def _checked(name, cnn_input, params):
    """The checks of types and shapes that every entry point makes first.  -> (x (38, H, W), h, w, [(name, parameter)] in the C ABI's order)"""
    if not isinstance(params, HourglassCNN):
        raise TypeError("%s: params must be a HourglassCNN, got %s" % (name, type(params).__name__))
    if not torch.is_tensor(cnn_input):
        raise TypeError("%s: cnn_input must be a tensor" % name)
    x = cnn_input
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 3:
        raise ValueError("%s: cnn_input must be (1, %d, H, W) or (%d, H, W), got %s" % (name, C, C, tuple(cnn_input.shape)))
    if x.shape[0] != C:
        raise ValueError("%s: cnn_input has %d channels, which implies hidden_dim = %d; the kernels have hidden_dim = %d only (32 per-view features + ray + colour)"
                         % (name, x.shape[0], x.shape[0], C))
    h, w = int(x.shape[1]), int(x.shape[2])
    if min(h, w) < _lib.HG_MIN_SIDE or max(h, w) > _lib.HG_MAX_SIDE:
        raise ValueError("%s: a frame of %d x %d is out of range (sides %d .. %d: the bottleneck is a quarter of the frame)" % (name, h, w, _lib.HG_MIN_SIDE, _lib.HG_MAX_SIDE))
    tensors = []
    for layer, cout, cin, k in LAYERS:
        wt, bt = getattr(params, layer + "_w"), getattr(params, layer + "_b")
        if tuple(wt.shape) != (cout, cin, k, k):
            raise ValueError("%s: %s_w must be %s, got %s" % (name, layer, (cout, cin, k, k), tuple(wt.shape)))
        if tuple(bt.shape) != (cout,):
            raise ValueError("%s: %s_b must be %s, got %s" % (name, layer, (cout,), tuple(bt.shape)))
        tensors += [(layer + "_w", wt), (layer + "_b", bt)]
    return x, h, w, tensors


def _on_one_device(name, x, tensors):
    """... and the checks that come last (after the forward-only refusal, where there is one): nothing on the CPU, everything on x's device."""
    _device.refuse_cpu("hourglass", "%s's cnn_input" % name, x)
    for what, t in tensors:
        _device.refuse_cpu("hourglass", "%s's %s" % (name, what), t)
    for what, t in tensors:
        if t.device != x.device:
            raise ValueError("%s: cnn_input is on %s, %s on %s" % (name, x.device, what, t.device))


def _forward_call(dev, h, w, x, flat, render_scale, arena, half=False):
    """x, flat: float32, contiguous, on dev; arena: that of the precision's C ABI, at least its required size.  -> (residual, image_pred or None)"""
    with torch.cuda.device(dev):
        residual = torch.empty((3, h, w), dtype=torch.float32, device=dev)
        image_pred = torch.empty((3, h, w), dtype=torch.float32, device=dev) if render_scale is not None else None
    _device.call(dev, "ibgs_hgh_forward" if half else "ibgs_hg_forward", h, w, x.data_ptr(), *[t.data_ptr() for t in flat], 1.0 if render_scale is None else render_scale,
                 residual.data_ptr(), None if image_pred is None else image_pred.data_ptr(), arena.data_ptr(), arena.numel())
    return residual, image_pred


class HourglassCNN(nn.Module):
    """The eighteen parameters of the reference's `ConvDecoderAE(38)` (nn.Conv2d's default initialisation), named <layer>_w / <layer>_b for the layers enc1,
    enc2, enc3, up2_conv, dec2, up1_conv, dec1, fuse_input, final.  `load_state_dict` takes this module's keys or the reference's (enc1.0.weight,
    up2_conv.0.bias, fuse_input.0.weight, final.weight, ...), so the `conv_decoder.` part of a ColorFusionResidualNet checkpoint loads unchanged."""

    def __init__(self):
        super().__init__()
        for layer, cout, cin, k in LAYERS:
            conv = nn.Conv2d(cin, cout, kernel_size=k)
            setattr(self, layer + "_w", nn.Parameter(conv.weight.detach().clone()))
            setattr(self, layer + "_b", nn.Parameter(conv.bias.detach().clone()))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for theirs, mine in REFERENCE_KEYS.items():
            if prefix + theirs in state_dict:
                if prefix + mine in state_dict:
                    raise ValueError("HourglassCNN.load_state_dict: both %r and %r are given" % (prefix + theirs, prefix + mine))
                state_dict[prefix + mine] = state_dict.pop(prefix + theirs)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, cnn_input, render_scale=None, return_stages=False, precision="float32"):
        """`hourglass_forward` with this module's parameters."""
        return hourglass_forward(cnn_input, self, render_scale, return_stages, precision)


class ColorAggregationNet(nn.Module):
    """The reference's `ColorFusionResidualNet` for test-time rendering: `front_end` (its per_view_mlp) and `cnn` (its conv_decoder).  `load_state_dict` takes
    a whole checkpoint of the reference unchanged (per_view_mlp.* and conv_decoder.*, as its training script saves `color_aggregation_network.state_dict()`),
    or this module's own keys (front_end.*, cnn.*)."""

    def __init__(self, mode="mean"):
        super().__init__()
        self.front_end = PerViewFrontEnd(mode)
        self.cnn = HourglassCNN()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for key in list(state_dict):
            for theirs, mine in (("per_view_mlp.", "front_end.per_view_mlp."), ("conv_decoder.", "cnn.")):
                if key.startswith(prefix + theirs):
                    state_dict[prefix + mine + key[len(prefix + theirs):]] = state_dict.pop(key)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, render_pkg, nb_visible_src_frames=3, burned_in_gauss=1.0, none_if_no_level=False, precision="float32", *, residual_resolution_scale=1.0,
                enable_exposure_correction=False):
        """`fuse_color` with this network."""
        return fuse_color(render_pkg, self, nb_visible_src_frames, burned_in_gauss, none_if_no_level, precision, residual_resolution_scale=residual_resolution_scale,
                          enable_exposure_correction=enable_exposure_correction)


def fuse_color(render_pkg, net, nb_visible_src_frames=3, burned_in_gauss=1.0, none_if_no_level=False, precision="float32", *, residual_resolution_scale=1.0,
               enable_exposure_correction=False):
    """The reference's test-time fuse_color on the `render()` dictionary (keys "render", "warped_image", "cam_feat",
    "camera_ray", "min_depth_diff") with a `ColorAggregationNet`: the per-view front end, then the hourglass.  -> a dictionary with the reference's keys:
      image_pred, residual    (3, H, W)
      valid_warp_mask         (min_depth_diff < 0.999) as float
      burned_in_gauss         the float that was passed
      nb_valid_warp_level     a 0-d int32 DEVICE tensor (the reference's Python int is `int(...)` of it: one synchronisation, the caller's choice)
      warped_image_list       the first min(nb_visible_src_frames, S) slots as an (H, W, k, 3) view of warped_image; NOT trimmed to nb_valid_warp_level, which
                              the host does not know -- slots from that level on are all zero or unused
    The reference returns None when no slot level carries a colour.  With `none_if_no_level` the count is read back (ONE synchronisation, the only one) and
    None is returned then; without it nothing waits, the aggregated features are exactly zero and image_pred is the network's output on them.
    `precision="float16"` runs the hourglass in half precision (`hourglass_forward`), as the reference renders by default (autocast).  The per-view front
    end still runs its float32 kernels: its 32 features reach the hourglass unrounded by a half-precision MLP, which is closer to float64 than the
    reference's autocast run (that one runs the two Linear layers in half too).  Without the keyword every bit is what it was.
    `enable_exposure_correction` (the reference's option of that name): render_pkg must also hold "use_first_src_frame_mask"; `exposure.exposure_correct`
    fits the affine colour map on the device, and the corrected image takes the place of "render" in the residual features, in the CNN's colour channels
    and in image_pred = burned_in_gauss * corrected + residual.  The correction is float32 whatever `precision`.  The dictionary then also holds
      exposure_affine         (3, 4) float32
      exposure_fit_ok         a 0-d int32 DEVICE tensor: 0 when the fit was undetermined and the image went through unchanged
    Without the keyword every bit and every key is what it was.
    `residual_resolution_scale` (the reference's option of that name; keyword only, like `enable_exposure_correction` beside it): with a value other than 1 the
    CNN runs at Hr x Wr = int(H s) x int(W s) (`resample.scaled_size`; both must lie in the hourglass's range, else ValueError): the exposure correction
    if asked for, the level count at FULL resolution, `resample.resized_features` (the masked features interpolated, align_corners=True, not the images),
    `hourglass_forward` there in the given `precision`, and `resample.upsample_residual`, which also forms image_pred = burned_in_gauss * render (or the
    corrected image) + residual at H x W.  The dictionary is the same: residual is the upsampled (3, H, W) one, valid_warp_mask and warped_image_list stay
    at full resolution.  With a value == 1 the code above runs and every bit and every key is what it was.  Training at a reduced resolution is
    `resample_train.fuse_color_train_scaled`: `fuse_color_train` and `coloragg.fuse_color_inputs` have no such keyword.
    Forward only: call it under torch.no_grad()."""
    name = "fuse_color"
    _check_precision(name, precision)
    render, h, w = _checked_package(name, render_pkg, net)
    reduced = None
    if residual_resolution_scale != 1:
        reduced = scaled_size(h, w, residual_resolution_scale)
        if min(reduced) < _lib.HG_MIN_SIDE or max(reduced) > _lib.HG_MAX_SIDE:
            raise ValueError("%s: residual_resolution_scale %r turns the frame of %d x %d into %d x %d, which is out of the hourglass's range (sides %d .. %d)"
                             % (name, residual_resolution_scale, h, w, reduced[0], reduced[1], _lib.HG_MIN_SIDE, _lib.HG_MAX_SIDE))
    if torch.is_grad_enabled() and (any(torch.is_tensor(v) and v.requires_grad for v in render_pkg.values()) or any(p.requires_grad for p in net.parameters())):
        raise RuntimeError("%s is forward only: call it under torch.no_grad() (an input or parameter requires grad and grad mode is on); training keeps "
                           "torch's CNN behind coloragg.fuse_color_inputs" % name)
    camera_ray = _ray_planes(render_pkg["camera_ray"], h, w)
    warped = render_pkg["warped_image"]
    exposure = {}
    if enable_exposure_correction:
        render, exposure["exposure_affine"], exposure["exposure_fit_ok"] = correct_package(name, render_pkg, render, warped)
    if reduced is None:
        cnn_input, levels = net.front_end(render, warped, render_pkg["cam_feat"], camera_ray, nb_visible_src_frames)
    else:
        levels = count_levels(warped, nb_visible_src_frames)
        front = net.front_end
        cnn_input = resized_features(render, warped, render_pkg["cam_feat"], camera_ray, front.w1, front.b1, front.w2, front.b2, reduced, levels, front.mode)
    if none_if_no_level and int(levels.item()) == 0:
        return None
    if reduced is None:
        residual, image_pred = hourglass_forward(cnn_input, net.cnn, render_scale=float(burned_in_gauss), precision=precision)
    else:
        residual, image_pred = upsample_residual(hourglass_forward(cnn_input, net.cnn, precision=precision), render, float(burned_in_gauss))
    return _fused(image_pred, residual, render_pkg["min_depth_diff"], float(burned_in_gauss), levels, warped, nb_visible_src_frames, exposure)


def _checked_package(name, render_pkg, net):
    """The checks `fuse_color` and `fuse_color_train` make first.  -> (render, H, W)"""
    if not isinstance(net, ColorAggregationNet):
        raise TypeError("%s: net must be a ColorAggregationNet, got %s" % (name, type(net).__name__))
    for key in ("render", "warped_image", "cam_feat", "camera_ray", "min_depth_diff"):
        if key not in render_pkg:
            raise KeyError("%s: render_pkg lacks %r" % (name, key))
    render = render_pkg["render"]
    if not torch.is_tensor(render) or render.dim() != 3 or render.shape[0] != 3:
        raise ValueError("%s: render_pkg['render'] must be a (3, H, W) tensor" % name)
    h, w = int(render.shape[1]), int(render.shape[2])
    if min(h, w) < _lib.HG_MIN_SIDE or max(h, w) > _lib.HG_MAX_SIDE:
        raise ValueError("%s: a frame of %d x %d is out of range (sides %d .. %d)" % (name, h, w, _lib.HG_MIN_SIDE, _lib.HG_MAX_SIDE))
    return render, h, w


def _ray_planes(camera_ray, h, w):
    """render()'s (3, H W) rays as planes; anything else is left to the front end"""
    if torch.is_tensor(camera_ray) and camera_ray.numel() == 3 * h * w:
        return camera_ray.view(3, h, w)
    return camera_ray


def _fused(image_pred, residual, min_depth_diff, burned, levels, warped, nb_visible_src_frames, exposure):
    """The dictionary `fuse_color` and `fuse_color_train` return"""
    h, w = residual.shape[1:]
    slots = warped.reshape(-1, 3, h, w)
    slots = slots[:min(int(nb_visible_src_frames), slots.shape[0])]
    return {"image_pred": image_pred, "residual": residual, "valid_warp_mask": (min_depth_diff < 0.999).float(), "burned_in_gauss": burned,
            "nb_valid_warp_level": levels, "warped_image_list": slots.permute(2, 3, 0, 1), **exposure}


# ---- training: the backward (C ABI include/ibgs_hg_train.h, csrc/hgtrain.hip) --------------------------------------------------------------------------------
def _backward_call(dev, h, w, x, flat, burned, arena, g_res, g_ip, need_x, need_params):
    """x, flat, g_res, g_ip: float32, contiguous, on dev; arena: the owned stages arena.  -> (grad_x (38, h, w) or None, [18 gradients] or None)"""
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        grad_x = torch.empty((C, h, w), dtype=torch.float32, device=dev) if need_x else None
        grads = [torch.empty_like(t) for t in flat] if need_params else None
    sc = _device.scratch(dev, _lib.load().ibgs_hgb_required_scratch(h, w))
    _device.call(dev, "ibgs_hgb_backward", h, w, x.data_ptr(), *[t.data_ptr() for t in flat], float(burned), arena.data_ptr(), ptr(g_res), ptr(g_ip), ptr(grad_x),
                 *([g.data_ptr() for g in grads] if need_params else [None] * 18), sc.data_ptr(), sc.numel())
    return grad_x, grads


def _check_scale(name, precision, grad_scale_log2, status, return_decisions=False):
    """The checks of the half-precision training keywords, before any GPU work.  -> the scale as an int or None"""
    if precision != "float16":
        if grad_scale_log2 is not None or status is not None or return_decisions:
            raise ValueError("%s: grad_scale_log2, status and return_decisions belong to precision=\"float16\"" % name)
        return None
    if grad_scale_log2 is not None:
        if isinstance(grad_scale_log2, bool) or not isinstance(grad_scale_log2, int):
            raise TypeError("%s: grad_scale_log2 must be None (automatic) or an int, got %r" % (name, grad_scale_log2))
        if abs(grad_scale_log2) > 300:
            raise ValueError("%s: grad_scale_log2 %d is out of range (-300 .. 300)" % (name, grad_scale_log2))
    if status is not None:
        if not torch.is_tensor(status) or status.dtype != torch.int32 or status.numel() != 2 or not status.is_contiguous():
            raise ValueError("%s: status must be a contiguous int32 tensor of two words (the scale's k, the count of non-finite binary16 gradient values)" % name)
    return grad_scale_log2


def _status_on(name, status, dev):
    if status is not None:
        _device.refuse_cpu("hourglass", "%s's status" % name, status)
        if status.device != dev:
            raise ValueError("%s: cnn_input is on %s, status on %s" % (name, dev, status.device))


def _backward_call_half(dev, h, w, x, flat, burned, arena, g_res, g_ip, need_x, need_params, grad_scale_log2, status):
    """`_backward_call` for the half-precision unit (C ABI include/ibgs_hg_half_train.h); arena: that of ibgs_hgh_forward.  -> (grad_x, grads, the backward's arena)"""
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        grad_x = torch.empty((C, h, w), dtype=torch.float32, device=dev) if need_x else None
        grads = [torch.empty_like(t) for t in flat] if need_params else None
    sc = _device.scratch(dev, _lib.load().ibgs_hgh_train_required_scratch(h, w))
    fixed = grad_scale_log2 is not None
    _device.call(dev, "ibgs_hgh_train_backward", h, w, x.data_ptr(), *[t.data_ptr() for t in flat], float(burned), arena.data_ptr(), ptr(g_res), ptr(g_ip),
                 _lib.HGHT_SCALE_FIXED if fixed else _lib.HGHT_SCALE_AUTO, grad_scale_log2 if fixed else 0, ptr(status), ptr(grad_x),
                 *([g.data_ptr() for g in grads] if need_params else [None] * 18), sc.data_ptr(), sc.numel())
    return grad_x, grads, sc


def _head_stages(sc, h, w):
    """d1 and f as the backward that filled the arena `sc` recomputed them (include/ibgs_hg_half_train.h: they follow the control words): (38, h, w) float16 views"""
    n = 80 * h * w
    at = 128 + (n + 127) // 128 * 128
    return tuple(sc[o:o + n].view(torch.float16).view(h, w, 40).permute(2, 0, 1)[:C] for o in (128, at))


def _decisions(sc, h, w):
    """The planes d1 > 0 and f > 0 the backward used, (38, h, w) bool each"""
    return tuple(v > 0 for v in _head_stages(sc, h, w))


def _upstream(name, what, g, h, w, dev):
    if g is None:
        return None
    if not torch.is_tensor(g) or g.numel() != 3 * h * w or tuple(g.shape[-2:]) != (h, w):
        raise ValueError("%s: %s must be (3, %d, %d)" % (name, what, h, w))
    _device.refuse_cpu("hourglass", "%s's %s" % (name, what), g)
    if g.device != dev:
        raise ValueError("%s: cnn_input is on %s, %s on %s" % (name, dev, what, g.device))
    return _f32(g).view(3, h, w)


def hourglass_backward(cnn_input, params, stages, grad_residual=None, grad_image_pred=None, render_scale=1.0, need_input_grad=True, need_param_grads=True, **half):
    """The raw backward of the hourglass: cnn_input and params as for `hourglass_forward`; `stages` the six intermediates of the forward on them -- either the
    arena of ibgs_hg_forward as a uint8 tensor (what `hourglass_train` keeps) or a dict of the tensors e1, e2, b, u2, d2, u1 (packed into one here);
    grad_residual and / or grad_image_pred (3, H, W): the upstream gradients (either may be None, not both); render_scale: the burned_in_gauss image_pred was
    formed with.  -> (grad_x (38, H, W) or None, {"enc1_w": ..., ...} or None): a group that is not needed is not computed (no weight-gradient kernel runs
    without need_param_grads; enc1's input gradient does not without need_input_grad).  d1 and f are recomputed.  Float32; the same arguments give the same
    bits; nothing waits for the host and no argument is written.  It refuses what `hourglass_forward` refuses.
    `**half` are four keyword-only options: precision="float32", grad_scale_log2=None, status=None, return_decisions=False.
    `precision="float16"` (without the keyword every bit is what it was) runs the half-precision backward (C ABI include/ibgs_hg_half_train.h,
    csrc/hghtrain.hip): `stages` is then the arena of ibgs_hgh_forward (what the half `hourglass_train` keeps) or a dict of the six binary16 stages of
    `hourglass_forward(..., return_stages=True, precision="float16")`; products have binary16 operands and float32 accumulation, each pre-activation gradient
    is rounded to binary16 once, and the gradients returned are float32, unrounded.  The upstream is scaled by an exact 2^k inside and the results by 2^-k:
    `grad_scale_log2=None` chooses k on the device from max |upstream| (no synchronisation), an int fixes it; the caller needs no loss scaling.  `status`:
    an optional int32 device tensor of two words, written with the k that was used and the number of non-finite binary16 gradient values that were stored
    (overflow is not hidden: it reaches the outputs).  `return_decisions=True` appends the boolean planes (d1 > 0, f > 0), (38, H, W) each, that the
    backward used."""
    name = "hourglass_backward"
    _options(name, half, ("precision", "grad_scale_log2", "status", "return_decisions"))
    precision, grad_scale_log2, status = half.get("precision", "float32"), half.get("grad_scale_log2"), half.get("status")
    return_decisions = half.get("return_decisions", False)
    _check_precision(name, precision)
    x, h, w, tensors = _checked(name, cnn_input, params)
    grad_scale_log2 = _check_scale(name, precision, grad_scale_log2, status, return_decisions)
    _on_one_device(name, x, tensors)
    dev = x.device
    is_half = precision == "float16"
    if grad_residual is None and grad_image_pred is None:
        raise ValueError("%s: grad_residual and grad_image_pred are both None" % name)
    if not (need_input_grad or need_param_grads):
        raise ValueError("%s: neither the input gradient nor the parameter gradients are asked for" % name)
    g_res = _upstream(name, "grad_residual", grad_residual, h, w, dev)
    g_ip = _upstream(name, "grad_image_pred", grad_image_pred, h, w, dev)
    _status_on(name, status, dev)
    need = (_lib.load().ibgs_hgh_required_scratch if is_half else _lib.load().ibgs_hg_required_scratch)(h, w)
    if isinstance(stages, dict):
        sides = ((h, w), (h // 2, w // 2), (h // 2 // 2, w // 2 // 2))
        arena = _device.scratch(dev, need)
        if is_half:          # the padding channels of a binary16 stage are zeros, and h(x) leads the arena
            arena.zero_()
            arena[:80 * h * w].view(torch.float16).view(h, w, 40)[:, :, :C].copy_(_f32(x).view(C, h, w).permute(1, 2, 0))
        views = _arena_views(arena, h, w, is_half)
        for stage, ch, level in STAGES:
            if stage not in stages or not torch.is_tensor(stages[stage]) or tuple(stages[stage].shape[-3:]) != (ch,) + sides[level] or stages[stage].numel() != views[stage].numel():
                raise ValueError("%s: stages[%r] must be a (%d, %d, %d) tensor" % (name, stage, ch, sides[level][0], sides[level][1]))
            _device.refuse_cpu("hourglass", "%s's stage %s" % (name, stage), stages[stage])
            views[stage].copy_(stages[stage].detach().reshape(views[stage].shape))
    else:
        if not torch.is_tensor(stages) or stages.dtype != torch.uint8 or stages.dim() != 1 or stages.numel() < need or not stages.is_contiguous():
            raise ValueError("%s: stages must be the arena of the forward (a contiguous uint8 tensor of %d bytes) or a dict of the six stages" % (name, need))
        _device.refuse_cpu("hourglass", "%s's stages" % name, stages)
        if stages.device != dev:
            raise ValueError("%s: cnn_input is on %s, stages on %s" % (name, dev, stages.device))
        arena = stages
    flat = [_f32(t) for _, t in tensors]
    if is_half:
        grad_x, grads, sc = _backward_call_half(dev, h, w, _f32(x), flat, float(render_scale), arena, g_res, g_ip, bool(need_input_grad), bool(need_param_grads),
                                                grad_scale_log2, status)
        out = (grad_x, (None if grads is None else {what: g for (what, _), g in zip(tensors, grads)}))
        return out + (_decisions(sc, h, w),) if return_decisions else out
    grad_x, grads = _backward_call(dev, h, w, _f32(x), flat, float(render_scale), arena, g_res, g_ip, bool(need_input_grad), bool(need_param_grads))
    return grad_x, (None if grads is None else {what: g for (what, _), g in zip(tensors, grads)})


class _HourglassTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dims, burned, *params):
        h, w = dims
        dev = x.device
        x32 = _f32(x).view(C, h, w)
        flat = [_f32(t) for t in params]
        arena = torch.empty(_lib.load().ibgs_hg_required_scratch(h, w), dtype=torch.uint8, device=dev)          # owned: the backward reads it
        residual, image_pred = _forward_call(dev, h, w, x32, flat, burned, arena)
        ctx.dims, ctx.burned, ctx.x_shape, ctx.x_dtype = dims, burned, x.shape, x.dtype
        ctx.set_materialize_grads(False)          # an output nobody used arrives as None, not as a plane of zeros
        ctx.save_for_backward(x32, arena, *flat)
        if image_pred is None:
            return residual
        return residual, image_pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_res, g_ip=None):
        need_x, need_params = ctx.needs_input_grad[0], any(ctx.needs_input_grad[3:])
        if not (need_x or need_params) or (g_res is None and g_ip is None):
            return (None,) * (3 + 18)
        x32, arena = ctx.saved_tensors[:2]
        flat = list(ctx.saved_tensors[2:])
        h, w = ctx.dims
        dev = x32.device
        g_res = None if g_res is None else _f32(g_res.to(dev))
        g_ip = None if g_ip is None else _f32(g_ip.to(dev))
        grad_x, grads = _backward_call(dev, h, w, x32, flat, 1.0 if ctx.burned is None else ctx.burned, arena, g_res, g_ip, need_x, need_params)
        if grad_x is not None:
            grad_x = grad_x.view(ctx.x_shape).to(ctx.x_dtype)
        if grads is None:
            grads = [None] * 18
        else:
            grads = [g if k else None for g, k in zip(grads, ctx.needs_input_grad[3:])]
        return (grad_x, None, None) + tuple(grads)


class _HourglassTrainHalf(torch.autograd.Function):
    """`_HourglassTrain` in half precision: the forward is ibgs_hgh_forward on an arena this node owns (its six binary16 stages are the kept activations),
    the backward ibgs_hgh_train_backward."""

    @staticmethod
    def forward(ctx, x, dims, burned, grad_scale_log2, status, *params):
        h, w = dims
        dev = x.device
        x32 = _f32(x).view(C, h, w)
        flat = [_f32(t) for t in params]
        arena = torch.empty(_lib.load().ibgs_hgh_required_scratch(h, w), dtype=torch.uint8, device=dev)          # owned: the backward reads it
        residual, image_pred = _forward_call(dev, h, w, x32, flat, burned, arena, True)
        ctx.dims, ctx.burned, ctx.x_shape, ctx.x_dtype, ctx.grad_scale_log2, ctx.status = dims, burned, x.shape, x.dtype, grad_scale_log2, status
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x32, arena, *flat)
        if image_pred is None:
            return residual
        return residual, image_pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_res, g_ip=None):
        need_x, need_params = ctx.needs_input_grad[0], any(ctx.needs_input_grad[5:])
        if not (need_x or need_params) or (g_res is None and g_ip is None):
            return (None,) * (5 + 18)
        x32, arena = ctx.saved_tensors[:2]
        flat = list(ctx.saved_tensors[2:])
        h, w = ctx.dims
        dev = x32.device
        g_res = None if g_res is None else _f32(g_res.to(dev))
        g_ip = None if g_ip is None else _f32(g_ip.to(dev))
        grad_x, grads, _ = _backward_call_half(dev, h, w, x32, flat, 1.0 if ctx.burned is None else ctx.burned, arena, g_res, g_ip, need_x, need_params,
                                               ctx.grad_scale_log2, ctx.status)
        if grad_x is not None:
            grad_x = grad_x.view(ctx.x_shape).to(ctx.x_dtype)
        if grads is None:
            grads = [None] * 18
        else:
            grads = [g if k else None for g, k in zip(grads, ctx.needs_input_grad[5:])]
        return (grad_x, None, None, None, None) + tuple(grads)


def hourglass_train(cnn_input, params, render_scale=None, **half):
    """`hourglass_forward` for training: differentiable in cnn_input and the eighteen parameters.  -> residual, or (residual, image_pred) with
    `render_scale=float`; both bit for bit what `hourglass_forward` returns.  The forward runs ibgs_hg_forward on an arena this node owns (the six stages are
    the kept activations; d1 and f are recomputed by the backward); the backward is `hourglass_backward` and computes only the groups autograd needs (a frozen
    CNN: no weight gradient runs; a detached input: no enc1 input gradient).  Double backward raises.  Nothing waits for the host.
    `**half` are three keyword-only options: precision (default: what `train_precision` set on this thread, else "float32"), grad_scale_log2=None, status=None.
    `precision="float16"` is mixed-precision training: the forward is `hourglass_forward(..., precision="float16")` bit for bit (the network is trained
    against the roundings it is rendered with), the kept activations are its binary16 stages, and the backward is `hourglass_backward(...,
    precision="float16")` with its `grad_scale_log2` and `status`.  The gradients are float32 and true to scale: no torch.amp.GradScaler is needed.  Without
    the keyword every bit is what it was."""
    name = "hourglass_train"
    _options(name, half, ("precision", "grad_scale_log2", "status"))
    precision, grad_scale_log2, status = half.get("precision", getattr(_TRAINING, "precision", "float32")), half.get("grad_scale_log2"), half.get("status")
    _check_precision(name, precision)
    x, h, w, tensors = _checked(name, cnn_input, params)
    grad_scale_log2 = _check_scale(name, precision, grad_scale_log2, status)
    _on_one_device(name, x, tensors)
    _status_on(name, status, x.device)
    if render_scale is not None:
        render_scale = float(render_scale)
    if precision == "float16":
        return _HourglassTrainHalf.apply(cnn_input, (h, w), render_scale, grad_scale_log2, status, *[t for _, t in tensors])
    return _HourglassTrain.apply(cnn_input, (h, w), render_scale, *[t for _, t in tensors])


def fuse_color_train(render_pkg, net, nb_visible_src_frames=3, iter_count=None, burn_start=None, burn_end=None, none_if_no_level=False, enable_exposure_correction=False):
    """The reference's TRAINING fuse_color (color_aggregation_network.py:156-250; residual_resolution_scale 1 -- `resample_train.fuse_color_train_scaled` for another) with a
    `ColorAggregationNet`, differentiable end to end: the per-view front end (`PerViewFrontEnd`, forward and backward kernels), then `hourglass_train`.
    burned_in_gauss = (clamp((iter_count - burn_start) / (burn_end - burn_start), 0, 1) + 1) / 2, or 1.0 when one of the three is None; while it is below 1
    the five tensors of render_pkg are detached (no gradient reaches the rasterizer; the networks' parameters still train).  -> the dictionary of
    `fuse_color`.  Nothing waits for the host unless `none_if_no_level` (which reads the level count back and returns None when it is 0).
    `enable_exposure_correction`: as in `fuse_color`, after the detaching, in the reference's order; "render" receives its gradient through the correction
    (the affine map is a constant of the backward), "warped_image" only the front end's.  Without the keyword every bit and every key is what it was.
    Inside `with train_precision("float16"):` the hourglass is trained in half precision (`hourglass_train`, automatic scale); the per-view front end and the exposure correction
    stay float32, as at test time, and the forward's image_pred is `fuse_color(..., precision="float16")`'s bit for bit."""
    name = "fuse_color_train"
    render, h, w = _checked_package(name, render_pkg, net)
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
    cnn_input, levels = net.front_end(render, warped, cam_feat, camera_ray, nb_visible_src_frames)
    if none_if_no_level and int(levels.item()) == 0:
        return None
    residual, image_pred = hourglass_train(cnn_input, net.cnn, render_scale=burned)
    return _fused(image_pred, residual, min_depth_diff, burned, levels, warped, nb_visible_src_frames, exposure)
