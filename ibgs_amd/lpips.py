"""LPIPS (VGG16, version 0.1) on the device: the third column of the reference's image evaluation (metrics.py:82; lpipsPyTorch/modules/{lpips,networks,utils}.py
with net_type 'vgg'), as thirteen launches of one matrix-core convolution kernel over both images of a pair, five head launches and a final sum (C ABI
include/ibgs_lpips.h, csrc/lpips.hip).

  z = (v - mean_c) / std_c on whatever comes in (metrics.py feeds [0, 1] images; nothing is rescaled to [-1, 1] here either)
  features: the thirteen 3 x 3 convolutions of vgg16.features with their ReLUs and four 2 x 2 pools, up to relu5_3
  taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (64, 128, 256, 512, 512 channels at H, H/2, H/4, H/8, H/16)
  per tap and pixel: n = f / (sqrt(sum_c f^2) + 1e-10);  m_k(p) = sum_c w_k[c] (n_x - n_y)^2;  v_k = mean_p m_k;  lpips = sum_k v_k

THE WEIGHTS ARE NOT SHIPPED and nothing here opens a URL.  `LPIPSNet.from_files(vgg16_path, lin_path)` reads the two files a user of LPIPS already has:
torchvision's VGG16 ImageNet checkpoint (vgg16-397923af.pth, what `torchvision.models.vgg16(weights=IMAGENET1K_V1)` leaves in the torch hub cache,
~/.cache/torch/hub/checkpoints) and the `lpips` package's linear layers (lpips/weights/v0.1/vgg.pth inside the installed package; the reference's
lpipsPyTorch leaves the same file in the hub cache as vgg.pth).  A freshly constructed `LPIPSNet` holds random values of the right shapes.

Float32: the convolutions are float32 multiply-add chains on the matrix cores, the head sums in double and rounds once.  The contract is a tolerance against
a float64 restatement (tests/lpips_ref.py).  Known follow-up, out of scope here: a half-precision form (as csrc/hghalf.hip is for the
hourglass), which would run the convolutions at the f16 matrix rate.  Forward only: nothing is differentiable.

HIP only: raises when the library or a GPU tensor is missing (no torch fallback in the product path)."""
import ctypes

import torch
from torch import nn

from . import _device, _lib

CHANNELS = _lib.LPIPS_CHANNELS
LEVEL = _lib.LPIPS_LEVEL
TAP_CONV = _lib.LPIPS_TAP_CONV
TAP_CHANNELS = tuple(CHANNELS[i + 1] for i in TAP_CONV)
# the thirteen convolutions in the order of the C ABI, and where each sits in vgg16.features
CONV_NAMES = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3")
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
LIN_NAMES = ("lin1", "lin2", "lin3", "lin4", "lin5")
# other people's names of the 31 tensors -> this module's: torchvision's VGG16 and the `lpips` package's lin layers, then the reference module's
FOREIGN_KEYS = {}
for _i, (_name, _at) in enumerate(zip(CONV_NAMES, FEATURE_INDEX)):
    for _theirs in ("features.%d" % _at, "net.layers.%d" % _at):
        FOREIGN_KEYS[_theirs + ".weight"] = _name + "_w"
        FOREIGN_KEYS[_theirs + ".bias"] = _name + "_b"
for _k, _name in enumerate(LIN_NAMES):
    FOREIGN_KEYS["lin%d.model.1.weight" % _k] = _name + "_w"
    FOREIGN_KEYS["lin.%d.1.weight" % _k] = _name + "_w"
# what such files hold beside them and this module has no use for: the classifier of VGG16, the reference module's z-score buffers
IGNORED_PREFIXES = ("classifier.", "net.mean", "net.std")


def level_sides(h, w):
    """-> ((H0, W0), .., (H4, W4)): the resolution of the five levels (a pool drops an odd last row or column)."""
    out = [(int(h), int(w))]
    for _ in range(_lib.LPIPS_TAPS - 1):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return tuple(out)


def _stage_offsets(h, w):
    """The arena of include/ibgs_lpips.h: float offsets of the thirteen stages (both images each), then the byte offset of the partials."""
    sides = level_sides(h, w)
    n = [2 * c * hh * ww for c, (hh, ww) in zip(TAP_CHANNELS, sides)]
    q, p = 0, n[0]
    r3 = p + n[2]
    r4 = r3 + n[3]
    return (p, q, p, p + n[1], p, r3, p, r3, r4, r3, r4, r4 + n[4], r4 + 2 * n[4]), 8 * n[0]


def _tap_views(arena, h, w):
    """-> ([relu1_2, .., relu5_3 of x], [the same of y]): float32 views (C, Hk, Wk) into the arena."""
    sides = level_sides(h, w)
    stage, _ = _stage_offsets(h, w)
    words = arena.view(torch.float32)          # (the arena's size is a multiple of 128 bytes)
    fx, fy = [], []
    for conv, c, (hh, ww) in zip(TAP_CONV, TAP_CHANNELS, sides):
        both = words[stage[conv]:stage[conv] + 2 * c * hh * ww].view(2, c, hh, ww)
        fx.append(both[0])
        fy.append(both[1])
    return fx, fy


class LPIPSNet(nn.Module):
    """The 31 tensors of LPIPS on VGG16: <conv>_w (Cout, Cin, 3, 3) and <conv>_b (Cout) for conv1_1 .. conv5_3 (26 parameters), lin1_w .. lin5_w of shape (C,)
    (the bias-free 1 x 1 `lin` layers of the five taps); all with requires_grad False.  Construction gives RANDOM values of the right shapes (He-normal
    weights, small biases, lin weights in [0, 1)): the library ships no weights.  `load_state_dict` takes any of
      * this module's own keys;
      * torchvision's VGG16 keys (features.N.weight / .bias; classifier.* is ignored) together with the `lpips` package's linK.model.1.weight (1, C, 1, 1);
      * the reference module's keys (net.layers.N.weight / .bias, lin.K.1.weight; net.mean and net.std are ignored),
    and raises naming the key on a tensor given under two names, on a wrong shape and on a missing layer.  `from_files` reads two local files (the module's
    docstring says which); no code path opens a URL."""

    def __init__(self):
        super().__init__()
        for i, name in enumerate(CONV_NAMES):
            cin, cout = CHANNELS[i], CHANNELS[i + 1]
            setattr(self, name + "_w", nn.Parameter(torch.randn(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5, requires_grad=False))
            setattr(self, name + "_b", nn.Parameter(torch.rand(cout) * 0.2 - 0.1, requires_grad=False))
        for name, c in zip(LIN_NAMES, TAP_CHANNELS):
            setattr(self, name + "_w", nn.Parameter(torch.rand(c), requires_grad=False))

    @staticmethod
    def parameter_names():
        return [n + s for n in CONV_NAMES for s in ("_w", "_b")] + [n + "_w" for n in LIN_NAMES]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        who = "LPIPSNet.load_state_dict"
        for key in list(state_dict):
            if key.startswith(prefix) and key[len(prefix):].startswith(IGNORED_PREFIXES):
                del state_dict[key]
        for theirs, mine in FOREIGN_KEYS.items():
            if prefix + theirs in state_dict:
                if prefix + mine in state_dict:
                    raise ValueError("%s: %r is given twice (as %r as well)" % (who, prefix + mine, prefix + theirs))
                state_dict[prefix + mine] = state_dict.pop(prefix + theirs)
        for mine in self.parameter_names():
            want = tuple(getattr(self, mine).shape)
            if prefix + mine not in state_dict:
                raise KeyError("%s: missing layer: no tensor for %r" % (who, prefix + mine))
            t = state_dict[prefix + mine]
            if mine.startswith("lin") and torch.is_tensor(t) and tuple(t.shape) == (1, want[0], 1, 1):
                t = state_dict[prefix + mine] = t.reshape(want)          # the 1 x 1 convolution of the `lpips` package and of the reference
            if not torch.is_tensor(t) or tuple(t.shape) != want:
                raise ValueError("%s: wrong shape: %r must be %s, got %s" % (who, prefix + mine, want, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @classmethod
    def from_files(cls, vgg16_path, lin_path, map_location="cpu"):
        """vgg16_path: torchvision's VGG16 state dict (vgg16-397923af.pth); lin_path: the `lpips` package's v0.1 vgg.pth.  Both are read with torch.load from
        the local file system."""
        state = {}
        for path in (vgg16_path, lin_path):
            part = torch.load(path, map_location=map_location, weights_only=True)
            if not isinstance(part, dict):
                raise ValueError("LPIPSNet.from_files: %s does not hold a state dict" % path)
            for key, value in part.items():
                if key in state:
                    raise ValueError("LPIPSNet.from_files: %r is in both files" % key)
                state[key] = value
        net = cls()
        net.load_state_dict(state)
        return net

    def forward(self, renders, gts, return_maps=False, return_features=False):
        """`lpips` with this network."""
        return lpips(renders, gts, self, return_maps, return_features)


def _pair_batch(name, what, t):
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor, got %s" % (name, what, type(t).__name__))
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError("%s: %s must be (N, 3, H, W) or (3, H, W), got %s" % (name, what, tuple(t.shape)))
    if t.shape[1] != 3:
        raise ValueError("%s: %s has %d channels; LPIPS on VGG16 takes 3" % (name, what, t.shape[1]))
    return t


def lpips(renders, gts, net, return_maps=False, return_features=False, return_tap_values=False):
    """renders, gts: (N, 3, H, W) or (3, H, W) (one pair), any strides, any floating dtype, 16 <= H, W <= 4096, values as the reference feeds them ([0, 1]);
    net: an `LPIPSNet`.  -> (N,) float32 on the device: LPIPS of every pair.  Nothing waits for the host.

    `return_maps`: also a list of five tensors (N, Hk, Wk), the per-pixel maps m_k of every pair (lpips = sum_k mean m_k).
    `return_features`: also (features of renders, features of gts), five tensors (C_k, Hk, Wk) each: VIEWS into the call's arena holding the taps of the
    LAST pair, valid until the next call on that device (a caller who keeps one longer clones it) -- the convention of `hourglass_forward`'s return_stages.
    `return_tap_values`: also (N, 5), the five v_k.
    The extras follow the scalar in that order.  The arena serves one pair (about 2.1 GB at 1080p: include/ibgs_lpips.h); a batch loops over it on the host.
    Raises on CPU tensors, on devices that differ, on a channel count other than 3 and on sides out of range."""
    name = "lpips"
    if not isinstance(net, LPIPSNet):
        raise TypeError("%s: net must be an LPIPSNet, got %s" % (name, type(net).__name__))
    x, y = _pair_batch(name, "renders", renders), _pair_batch(name, "gts", gts)
    if x.shape != y.shape:
        raise ValueError("%s: renders are %s, gts %s" % (name, tuple(x.shape), tuple(y.shape)))
    n, h, w = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    if min(h, w) < _lib.LPIPS_MIN_SIDE or max(h, w) > _lib.LPIPS_MAX_SIDE:
        raise ValueError("%s: a frame of %d x %d is out of range (sides %d .. %d: four pools must leave a pixel, and the arena stays below 20 GB)"
                         % (name, h, w, _lib.LPIPS_MIN_SIDE, _lib.LPIPS_MAX_SIDE))
    if not (x.is_floating_point() and y.is_floating_point()):
        raise TypeError("%s: renders and gts must be floating point, got %s and %s" % (name, x.dtype, y.dtype))
    params = [(p, getattr(net, p)) for p in net.parameter_names()]
    _device.refuse_cpu("lpips", "%s's renders" % name, x)
    _device.refuse_cpu("lpips", "%s's gts" % name, y)
    for what, t in params:
        _device.refuse_cpu("lpips", "%s's %s" % (name, what), t)
    dev = x.device
    for what, t in [("gts", y)] + params:
        if t.device != dev:
            raise ValueError("%s: renders are on %s, %s on %s" % (name, dev, what, t.device))
    flat = [t.detach().float().contiguous() for _, t in params]
    table = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    conv_w, conv_b, lin_w = table(flat[0:26:2]), table(flat[1:26:2]), table(flat[26:])
    sides = level_sides(h, w)
    with torch.cuda.device(dev):
        out = torch.empty((n,), dtype=torch.float32, device=dev)
        taps = torch.empty((n, _lib.LPIPS_TAPS), dtype=torch.float32, device=dev) if return_tap_values else None
        maps = [torch.empty((n, hh, ww), dtype=torch.float32, device=dev) for hh, ww in sides] if return_maps else None
    arena = _device.scratch(dev, _lib.load().ibgs_lpips_required_scratch(h, w))
    for i in range(n):          # the arena serves one pair
        xi, yi = x[i].detach().float().contiguous(), y[i].detach().float().contiguous()
        _device.call(dev, "ibgs_lpips_forward", h, w, xi.data_ptr(), yi.data_ptr(), conv_w, conv_b, lin_w, out[i:].data_ptr(),
                     None if taps is None else taps[i:].data_ptr(), None if maps is None else table([m[i] for m in maps]), arena.data_ptr(), arena.numel())
    result = (out,)
    if return_maps:
        result += (maps,)
    if return_features:
        result += (_tap_views(arena, h, w),)
    if return_tap_values:
        result += (taps,)
    return result[0] if len(result) == 1 else result
