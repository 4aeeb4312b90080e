"""The per-view front end of the reference's colour aggregation network (color_aggregation_network.py:102-133, 156-198, 229-233; train.py:347-357,
render.py:137-147): from the rasterizer's planes to the (1, 38, H, W) tensor `ColorFusionResidualNet.forward` hands to its `conv_decoder`, as one kernel
forward and one backward (C ABI include/ibgs_color_agg.h, csrc/coloragg.hip).  In training the hourglass CNN behind it stays with torch; at test time
ibgs_amd/hourglass.py runs it.

  levels  = min(slots of warped_image whose colours are not all zero, nb_visible_src_frames, S), formed and read ON THE DEVICE: nothing waits for the host
  slot k  : v = (cam_feat[4k] + .. + cam_feat[4k + 3] > 0);  x = [(warped[3k + c] - render[c]) v, cam_feat[4k .. 4k + 3]];  h2 = relu(W2 relu(W1 x + b1) + b2)
  output  = [mean (or max) of h2 over k < levels (32), camera_ray (3), render (3)]

The contract is a tolerance against a float64 restatement (tests/coloragg_ref.py).

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import torch
from torch import nn

from . import _device, _lib

MODES = {"mean": _lib.CAGG_MEAN, "max": _lib.CAGG_MAX}
# the reference's names of the four parameters inside ColorFusionResidualNet -> this module's
REFERENCE_KEYS = {"per_view_mlp.0.weight": "w1", "per_view_mlp.0.bias": "b1", "per_view_mlp.2.weight": "w2", "per_view_mlp.2.bias": "b2"}


def _f32(t):
    return t.detach().float().contiguous()


class _PerView(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, warped_image, w1, b1, w2, b2, cam_feat, camera_ray, levels, dims, mode):
        s, h, w = dims
        dev = render.device
        saved = [_f32(t) for t in (render, warped_image, cam_feat, w1, b1, w2, b2)]
        ray = _f32(camera_ray)
        with torch.cuda.device(dev):
            out = torch.empty((1, _lib.CAGG_FEATURES + 6, h, w), dtype=torch.float32, device=dev)
        r, x, feat, p1, q1, p2, q2 = saved
        _device.call(dev, "ibgs_cagg_forward", s, h, w, mode, r.data_ptr(), x.data_ptr(), feat.data_ptr(), ray.data_ptr(), p1.data_ptr(), q1.data_ptr(), p2.data_ptr(),
                     q2.data_ptr(), levels.data_ptr(), out.data_ptr())
        ctx.dims, ctx.mode = dims, mode
        ctx.shapes = (render.shape, warped_image.shape)
        ctx.save_for_backward(*saved, levels)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad[:6]
        if not any(need):
            return (None,) * 11
        r, x, feat, p1, q1, p2, q2, levels = ctx.saved_tensors
        s, h, w = ctx.dims
        dev = r.device
        go = _f32(grad_out.to(dev))
        with torch.cuda.device(dev):
            # (with render and warped_image detached -- the reference's burn-in -- no image gradient is allocated and the kernel does not run that arithmetic)
            grads = [torch.empty_like(t) if k else None for t, k in zip((r, x, p1, q1, p2, q2), need)]
        ptr = lambda t: None if t is None else t.data_ptr()
        sc = _device.scratch(dev, _lib.load().ibgs_cagg_required_scratch(s, h, w)) if any(need[2:]) else None
        _device.call(dev, "ibgs_cagg_backward", s, h, w, ctx.mode, r.data_ptr(), x.data_ptr(), feat.data_ptr(), p1.data_ptr(), q1.data_ptr(), p2.data_ptr(), q2.data_ptr(),
                     levels.data_ptr(), go.data_ptr(), *[ptr(g) for g in grads], ptr(sc), 0 if sc is None else sc.numel())
        if grads[0] is not None:
            grads[0] = grads[0].view(ctx.shapes[0])
        if grads[1] is not None:
            grads[1] = grads[1].view(ctx.shapes[1])
        return tuple(grads) + (None,) * 5


def _planes(name, what, t, per_source, h, w):
    """t: (per_source * S, H, W) or (S, per_source, H, W) -> S."""
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor" % (name, what))
    if t.dim() == 3 and t.shape[0] % per_source == 0:
        total = t.shape[0] // per_source
    elif t.dim() == 4 and t.shape[1] == per_source:
        total = t.shape[0]
    else:
        raise ValueError("%s: %s must be (%d S, H, W) or (S, %d, H, W), got %s" % (name, what, per_source, per_source, tuple(t.shape)))
    if not 1 <= total <= _lib.CAGG_MAX_SRC:
        raise ValueError("%s: %s holds %d sources (1 .. %d)" % (name, what, total, _lib.CAGG_MAX_SRC))
    if tuple(t.shape[-2:]) != (h, w):
        raise ValueError("%s: %s is %d x %d, render %d x %d" % (name, what, t.shape[-2], t.shape[-1], h, w))
    return total


def _image3(name, what, t):
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor" % (name, what))
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError("%s: %s must be (3, H, W), got %s" % (name, what, tuple(t.shape)))
    h, w = int(t.shape[1]), int(t.shape[2])
    if h * w == 0:
        raise ValueError("%s: empty image %s" % (name, tuple(t.shape)))
    if h > _lib.CAGG_MAX_SIDE or w > _lib.CAGG_MAX_SIDE:
        raise ValueError("%s: image %s too large (sides <= %d)" % (name, tuple(t.shape), _lib.CAGG_MAX_SIDE))
    return h, w


def _parameters(name, w1, b1, w2, b2):
    for what, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if not torch.is_tensor(t):
            raise TypeError("%s: %s must be a tensor" % (name, what))
    if w1.dim() != 2 or w1.shape[1] != 7:
        raise ValueError("%s: w1 must be (32, 7), got %s" % (name, tuple(w1.shape)))
    width = int(w1.shape[0])
    if width != _lib.CAGG_FEATURES:
        raise ValueError("%s: a per-view feature width of %d is not supported (the kernels have %d only); w1 is %s" % (name, width, _lib.CAGG_FEATURES, tuple(w1.shape)))
    for what, t, shape in (("b1", b1, (width,)), ("w2", w2, (width, width)), ("b2", b2, (width,))):
        if tuple(t.shape) != shape:
            raise ValueError("%s: %s must be %s, got %s" % (name, what, shape, tuple(t.shape)))


def _count(name, what, n, least):
    if isinstance(n, bool) or int(n) != n or n < least:
        raise ValueError("%s: %s must be an integer >= %d, got %r" % (name, what, least, n))
    return int(n)


def _front_end_arguments(unit, name, render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2, modes, mode, levels, own, before_device=None, levels_optional=False):
    """The argument checks of the two front ends, `per_view_features` and `resample.resized_features`, in the order both make them: the shapes, the source
    counts, the parameters, `own()` (the caller's check of the argument only it has; its value is handed back), the mode, `levels` (an int >= 0 or a 0-d int32 tensor; None
    is left alone where `levels_optional`), `before_device(tensors)` if given, the refusal of CPU tensors under `unit`'s name, one device for all.
    -> (S, H, W, own's value, levels, [render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2])"""
    h, w = _image3(name, "render", render)
    if _image3(name, "camera_ray", camera_ray) != (h, w):
        raise ValueError("%s: camera_ray is %s, render %s" % (name, tuple(camera_ray.shape), tuple(render.shape)))
    s, s_feat = _planes(name, "warped_image", warped_image, 3, h, w), _planes(name, "cam_feat", cam_feat, 4, h, w)
    if s_feat != s:
        raise ValueError("%s: warped_image holds %d sources, cam_feat %d" % (name, s, s_feat))
    _parameters(name, w1, b1, w2, b2)
    mine = own()
    if mode not in modes:
        raise ValueError("%s: mode must be 'mean' or 'max', got %r" % (name, mode))
    named = [("render", render), ("warped_image", warped_image), ("cam_feat", cam_feat), ("camera_ray", camera_ray), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)]
    if torch.is_tensor(levels):
        if levels.dim() != 0 or levels.dtype != torch.int32:
            raise ValueError("%s: levels must be an int or a 0-d int32 tensor, got %s %s" % (name, tuple(levels.shape), levels.dtype))
        named.append(("levels", levels))
    elif levels is not None or not levels_optional:
        levels = _count(name, "levels", levels, 0)
    if before_device is not None:
        before_device([t for _, t in named])
    for what, t in named:
        _device.refuse_cpu(unit, "%s's %s" % (name, what), t)
    dev = render.device
    for what, t in named[1:]:
        if t.device != dev:
            raise ValueError("%s: render is on %s, %s on %s" % (name, dev, what, t.device))
    return s, h, w, mine, levels, [t for _, t in named[:8]]


def _levels_of(warped_image, s, h, w, nb):
    """min(slots of warped_image whose colours are not all zero, nb, s) as a 0-d int32 DEVICE tensor (ibgs_cagg_levels); the arguments are checked already."""
    dev = warped_image.device
    x = _f32(warped_image)
    with torch.cuda.device(dev):
        levels = torch.empty((), dtype=torch.int32, device=dev)
    sc = _device.scratch(dev, _lib.load().ibgs_cagg_required_scratch(s, h, w))
    _device.call(dev, "ibgs_cagg_levels", s, h, w, x.data_ptr(), min(nb, s), levels.data_ptr(), sc.data_ptr(), sc.numel())
    return levels


def count_levels(warped_image, nb_visible_src_frames=3):
    """warped_image (3 S, H, W) or (S, 3, H, W) at FULL resolution -> the 0-d int32 DEVICE tensor min(slots whose colours are not all zero,
    nb_visible_src_frames, S): the level count of `per_view_features` without its forward (ibgs_cagg_levels).  Nothing waits for the host.
    `resample.count_levels` is this function: the reduced-resolution tail is its caller, and its refusal of a CPU tensor names that module."""
    name = "count_levels"
    if not torch.is_tensor(warped_image) or warped_image.dim() not in (3, 4):
        raise ValueError("%s: warped_image must be a (3 S, H, W) or (S, 3, H, W) tensor" % name)
    h, w = int(warped_image.shape[-2]), int(warped_image.shape[-1])
    if h * w == 0 or h > _lib.CAGG_MAX_SIDE or w > _lib.CAGG_MAX_SIDE:
        raise ValueError("%s: a frame of %d x %d is out of range (sides 1 .. %d)" % (name, h, w, _lib.CAGG_MAX_SIDE))
    s = _planes(name, "warped_image", warped_image, 3, h, w)
    nb = _count(name, "nb_visible_src_frames", nb_visible_src_frames, 1)
    _device.refuse_cpu("resample", "%s's warped_image" % name, warped_image)
    return _levels_of(warped_image, s, h, w, nb)


def per_view_features(render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2, nb_visible_src_frames=3, mode="mean", levels=None):
    """The front end on the rasterizer's outputs taken whole: render (3, H, W) (or the exposure-corrected image made of it); warped_image (3 S, H, W) or
    (S, 3, H, W); cam_feat (4 S, H, W) or (S, 4, H, W); camera_ray (3, H, W); the four parameters of `per_view_mlp` in nn.Linear layout (32, 7), (32,),
    (32, 32), (32,); 1 <= S <= 5.  -> (cnn_input (1, 38, H, W) float32, levels: a 0-d int32 DEVICE tensor).

    levels = min(slots whose warped colours are not all zero, nb_visible_src_frames, S) is counted on the device and read there; a caller who knows it
    passes `levels=int`, which is capped the same way.  A 0-d int32 device tensor -- the one an earlier call returned, say -- is taken as it is: the host
    never reads it, so nb_visible_src_frames does not cap it; the kernels only keep it within 0 .. S.  With levels == 0 the 32 aggregated channels and every gradient through them are exactly zero.
    mode: "mean" or "max" (the gradient goes to the first slot attaining the maximum).

    Differentiable in render, warped_image (full shape, zero in the unused slots: the rasterizer's dL_dwarped) and the four parameters.  cam_feat and
    camera_ray get NO gradient: the rasterizer's backward has no input for either, so they are treated as data.  With render and warped_image detached
    only the parameter gradients are computed."""
    name = "per_view_features"
    s, h, w, nb, levels, _ = _front_end_arguments("coloragg", name, render, warped_image, cam_feat, camera_ray, w1, b1, w2, b2, MODES, mode, levels,
                                                  lambda: _count(name, "nb_visible_src_frames", nb_visible_src_frames, 1), levels_optional=True)
    if levels is None:
        levels = _levels_of(warped_image, s, h, w, nb)
    elif not torch.is_tensor(levels):
        with torch.cuda.device(render.device):
            levels = torch.full((), min(levels, nb, s), dtype=torch.int32, device=render.device)
    out = _PerView.apply(render, warped_image, w1, b1, w2, b2, cam_feat.detach(), camera_ray.detach(), levels, (s, h, w), MODES[mode])
    return out, levels


class PerViewFrontEnd(nn.Module):
    """The four parameters of the reference's `per_view_mlp` (nn.Linear's default initialisation).  `load_state_dict` takes this module's keys (w1, b1, w2,
    b2) or the reference's (per_view_mlp.0.weight, .0.bias, .2.weight, .2.bias), so the front end of a ColorFusionResidualNet checkpoint loads unchanged:
    `front_end.load_state_dict({k: v for k, v in ckpt.items() if k.startswith("per_view_mlp.")})`."""

    def __init__(self, mode="mean"):
        super().__init__()
        if mode not in MODES:
            raise ValueError("PerViewFrontEnd: mode must be 'mean' or 'max', got %r" % (mode,))
        self.mode = mode
        a, b = nn.Linear(7, _lib.CAGG_FEATURES), nn.Linear(_lib.CAGG_FEATURES, _lib.CAGG_FEATURES)
        self.w1, self.b1 = nn.Parameter(a.weight.detach().clone()), nn.Parameter(a.bias.detach().clone())
        self.w2, self.b2 = nn.Parameter(b.weight.detach().clone()), nn.Parameter(b.bias.detach().clone())

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for theirs, mine in REFERENCE_KEYS.items():
            if prefix + theirs in state_dict:
                if prefix + mine in state_dict:
                    raise ValueError("PerViewFrontEnd.load_state_dict: both %r and %r are given" % (prefix + theirs, prefix + mine))
                state_dict[prefix + mine] = state_dict.pop(prefix + theirs)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, render, warped_image, cam_feat, camera_ray, nb_visible_src_frames=3, levels=None):
        """-> (cnn_input, levels) of `per_view_features` with this module's parameters."""
        return per_view_features(render, warped_image, cam_feat, camera_ray, self.w1, self.b1, self.w2, self.b2, nb_visible_src_frames, self.mode, levels)


def fuse_color_inputs(render_pkg, front_end, nb_visible_src_frames=3, none_if_no_level=False, enable_exposure_correction=False):
    """What the reference's fuse_color builds for the hourglass CNN, from the `render()` dictionary (keys "render", "warped_image", "cam_feat", "camera_ray",
    "min_depth_diff"; residual_resolution_scale 1).  -> (cnn_input (1, 38, H, W), valid_warp_mask = (min_depth_diff < 0.999) as float).
    `enable_exposure_correction` (the reference's option; render_pkg must also hold "use_first_src_frame_mask"): `exposure.exposure_correct` fits the affine
    colour map and the corrected image takes the place of "render" -- it is channels 35 .. 37 of cnn_input; a caller who wants the map itself calls
    exposure_correct.  Without the keyword every bit is what it was.
    During the reference's burn-in pass "render" and "warped_image" detached: only the front end's parameters then receive a gradient.

    The reference returns None when no slot level carries a colour.  That needs the count on the host: with `none_if_no_level` this function reads it back
    (ONE synchronisation, the only one) and returns None then; without it nothing waits, and the 32 aggregated channels are exactly zero instead."""
    name = "fuse_color_inputs"
    if not isinstance(front_end, PerViewFrontEnd):
        raise TypeError("%s: front_end must be a PerViewFrontEnd, got %s" % (name, type(front_end).__name__))
    for key in ("render", "warped_image", "cam_feat", "camera_ray", "min_depth_diff"):
        if key not in render_pkg:
            raise KeyError("%s: render_pkg lacks %r" % (name, key))
    render = render_pkg["render"]
    h, w = _image3(name, "render_pkg['render']", render)
    camera_ray = render_pkg["camera_ray"]
    if torch.is_tensor(camera_ray) and camera_ray.numel() == 3 * h * w:
        camera_ray = camera_ray.view(3, h, w)
    if enable_exposure_correction:
        from .exposure import correct_package          # (exposure.py takes its argument checks from this module)
        render = correct_package(name, render_pkg, render, render_pkg["warped_image"])[0]
    cnn_input, levels = front_end(render, render_pkg["warped_image"], render_pkg["cam_feat"], camera_ray, nb_visible_src_frames)
    if none_if_no_level and int(levels.item()) == 0:
        return None
    return cnn_input, (render_pkg["min_depth_diff"] < 0.999).float()
