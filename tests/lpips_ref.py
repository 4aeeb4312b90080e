"""Restatements of LPIPS on VGG16 (ibgs_amd/lpips.py, csrc/lpips.hip), written from its definition (include/ibgs_lpips.h), which restates
the reference's lpipsPyTorch/modules: networks.py:41-51 (the z-score), networks.py:53-63 and 88-96 (vgg16.features up to its 30th module, taps after modules
4, 9, 16, 23, 30), utils.py:6-8 (the channel normalisation) and lpips.py:30-36 (squared difference, the bias-free 1 x 1 `lin`, spatial mean, sum over taps):

  forward_ref        float64 numpy, tap by tap, pool by slicing: THE ARBITER.
  torch_composition  the same function from torch.nn.functional ops (conv2d, relu, max_pool2d) and tensor expressions at a chosen dtype, on the CPU.
  chain_f32          float32 in which every convolution output is ONE k-ordered multiply-add chain started from the bias, each step rounded once
                     (acc = f32(f64(acc) + f64(w) f64(x)): the product of two floats is exact in float64) -- what the f32 matrix-core instruction is; the
                     z-score and the head in float32 numpy.

All three take x, y (3, H, W) float32 and `params`, a dict of float32 numpy arrays <conv>_w (Cout, Cin, 3, 3), <conv>_b (Cout) for conv1_1 .. conv5_3 and
lin1_w .. lin5_w (C,), and return {"taps_x": [5], "taps_y": [5], "maps": [5], "v": (5,), "lpips": scalar}.  No torchvision here, and no weights: see
`seeded_params`."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3")
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)          # the convolutions inside vgg16.features
POOL_BEFORE = (2, 4, 7, 10)                                              # the convolutions that read a pooled input (features 4, 9, 16, 23 are the pools)
TAP_AFTER = (1, 3, 6, 9, 12)                                             # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
TAP_CHANNELS = (64, 128, 256, 512, 512)
LINS = ("lin1", "lin2", "lin3", "lin4", "lin5")
# networks.py:41-44 holds them as float32 tensors: the float32 values are the function's constants, at every precision
MEAN = np.array([-.030, -.088, -.188], dtype=np.float32)
STD = np.array([.458, .448, .450], dtype=np.float32)
EPS = 1e-10


def seeded_params(seed, kind="default"):
    """He-normal convolution weights N(0, 2 / (9 Cin)), biases U(-0.1, 0.1), lin weights U(0, 1) (the real ones are non-negative), float32.  With nn.Conv2d's
    default initialisation the activations shrink by orders of magnitude over thirteen layers and the 1e-10 of the normalisation dominates; with this one
    about half of every tap is ReLU-dead and the tap maxima are 0.2 .. 11 (tests/test_lpips_host.py prints them).
    kind "dead_tap5": conv5_3's bias is -100, so relu5_3 is exactly zero everywhere."""
    assert kind in ("default", "dead_tap5")
    g = np.random.default_rng(seed)
    p = {}
    for i, name in enumerate(CONVS):
        cin, cout = CHANNELS[i], CHANNELS[i + 1]
        p[name + "_w"] = (g.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        p[name + "_b"] = g.uniform(-0.1, 0.1, cout).astype(np.float32)
    for name, c in zip(LINS, TAP_CHANNELS):
        p[name + "_w"] = g.uniform(0.0, 1.0, c).astype(np.float32)
    if kind == "dead_tap5":
        p["conv5_3_b"] = np.full_like(p["conv5_3_b"], -100.0)
    return p


def seeded_pair(seed, h, w):
    """x uniform in [0, 1), y = clamp(x + 0.1 randn, 0, 1): float32 (3, h, w) each."""
    g = np.random.default_rng(seed)
    x = g.random((3, h, w)).astype(np.float32)
    y = np.clip(x + 0.1 * g.standard_normal((3, h, w)), 0.0, 1.0).astype(np.float32)
    return x, y


def state_dicts(p):
    """The same 31 tensors under the three namings `LPIPSNet.load_state_dict` takes -> (own, torchvision + lpips package, reference module), torch tensors.
    The second carries classifier.* entries and the third the z-score buffers, which a loader must ignore."""
    own = {k: torch.tensor(v) for k, v in p.items()}
    tv, theirs = {}, {}
    for name, at in zip(CONVS, FEATURE_INDEX):
        for s, t in (("_w", "weight"), ("_b", "bias")):
            tv["features.%d.%s" % (at, t)] = own[name + s].clone()
            theirs["net.layers.%d.%s" % (at, t)] = own[name + s].clone()
    for k, name in enumerate(LINS):
        tv["lin%d.model.1.weight" % k] = own[name + "_w"].reshape(1, -1, 1, 1).clone()
        theirs["lin.%d.1.weight" % k] = own[name + "_w"].reshape(1, -1, 1, 1).clone()
    tv["classifier.0.weight"], tv["classifier.0.bias"], tv["classifier.6.bias"] = torch.zeros(4, 7), torch.zeros(4), torch.zeros(10)
    theirs["net.mean"], theirs["net.std"] = torch.tensor(MEAN).reshape(1, 3, 1, 1), torch.tensor(STD).reshape(1, 3, 1, 1)
    return own, tv, theirs


def pool_ref(t):
    h, w = t.shape[-2:]
    t = t[..., :h // 2 * 2, :w // 2 * 2]
    return np.maximum(np.maximum(t[..., 0::2, 0::2], t[..., 0::2, 1::2]), np.maximum(t[..., 1::2, 0::2], t[..., 1::2, 1::2]))


def _conv_f64(t, wt, bias):
    """t: (B, Cin, h, w) float64"""
    cout = wt.shape[0]
    b, c, h, w = t.shape
    tp = np.zeros((b, c, h + 2, w + 2), dtype=np.float64)
    tp[:, :, 1:1 + h, 1:1 + w] = t
    out = np.broadcast_to(bias.astype(np.float64)[None, :, None, None], (b, cout, h, w)).copy()
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,bchw->bohw", wt[:, :, ky, kx].astype(np.float64), tp[:, :, ky:ky + h, kx:kx + w])
    return out


def _conv_chain(t, wt, bias):
    """t: (B, Cin, h, w) float32 -> float32, every element one chain over k = 9 ci + 3 ky + kx from the bias"""
    cout, cin = wt.shape[:2]
    b, c, h, w = t.shape
    tp = np.zeros((b, c, h + 2, w + 2), dtype=np.float64)
    tp[:, :, 1:1 + h, 1:1 + w] = t
    w64 = wt.astype(np.float64)
    acc = np.broadcast_to(bias.astype(np.float32)[None, :, None, None], (b, cout, h, w)).copy()
    for ci in range(cin):
        for ky in range(3):
            for kx in range(3):
                prod = w64[None, :, ci, ky, kx, None, None] * tp[:, ci, None, ky:ky + h, kx:kx + w]
                acc = (acc.astype(np.float64) + prod).astype(np.float32)
    return acc


def _features(x, y, p, conv, dtype):
    t = np.stack([np.asarray(x), np.asarray(y)]).astype(dtype)
    assert t.shape[1] == 3 and t.ndim == 4
    t = ((t - MEAN.astype(dtype)[None, :, None, None]) / STD.astype(dtype)[None, :, None, None]).astype(dtype)
    taps = []
    for i, name in enumerate(CONVS):
        if i in POOL_BEFORE:
            t = pool_ref(t)
        t = np.maximum(conv(t, p[name + "_w"], p[name + "_b"]), 0)
        if i in TAP_AFTER:
            taps.append(t)
    return taps


def _head(taps, p, dtype):
    maps, v = [], []
    for f, name in zip(taps, LINS):
        n = f / (np.sqrt((f * f).sum(axis=1, keepdims=True, dtype=dtype)) + dtype(EPS))
        d = (n[0] - n[1]) ** 2
        m = (p[name + "_w"].astype(dtype)[:, None, None] * d).sum(axis=0, dtype=dtype)
        maps.append(m)
        v.append(m.mean(dtype=dtype))
    v = np.array(v, dtype=dtype)
    return {"taps_x": [f[0] for f in taps], "taps_y": [f[1] for f in taps], "maps": maps, "v": v, "lpips": v.sum(dtype=dtype)}


def forward_ref(x, y, params):
    """-> float64 arrays: THE ARBITER."""
    return _head(_features(x, y, params, _conv_f64, np.float64), params, np.float64)


def chain_f32(x, y, params):
    """-> the same in float32: multiply-add chains for the convolutions, float32 numpy for the z-score and the head."""
    return _head(_features(x, y, params, _conv_chain, np.float32), params, np.float32)


def torch_composition(x, y, params, dtype):
    """-> the same as torch CPU tensors of `dtype`, from conv2d / relu / max_pool2d and the reference's tensor expressions."""
    tt = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    p = {k: tt(v) for k, v in params.items()}
    t = torch.stack([tt(x), tt(y)])
    t = (t - tt(MEAN)[None, :, None, None]) / tt(STD)[None, :, None, None]
    taps = []
    for i, name in enumerate(CONVS):
        if i in POOL_BEFORE:
            t = F.max_pool2d(t, 2, 2)
        t = F.relu(F.conv2d(t, p[name + "_w"], p[name + "_b"], padding=1))
        if i in TAP_AFTER:
            taps.append(t)
    maps, v = [], []
    for f, name in zip(taps, LINS):
        n = f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + EPS)
        d = (n[0:1] - n[1:2]) ** 2
        m = F.conv2d(d, p[name + "_w"].reshape(1, -1, 1, 1))
        maps.append(m[0, 0])
        v.append(m.mean((2, 3), True).reshape(()))
    v = torch.stack(v)
    return {"taps_x": [f[0] for f in taps], "taps_y": [f[1] for f in taps], "maps": maps, "v": v, "lpips": torch.sum(v)}


def flat_items(result):
    """-> [(name, array)] of the ten tap tensors and the five maps, in a fixed order."""
    out = []
    for k in range(5):
        out.append(("tap%d x" % (k + 1), result["taps_x"][k]))
        out.append(("tap%d y" % (k + 1), result["taps_y"][k]))
    for k in range(5):
        out.append(("map%d" % (k + 1), result["maps"][k]))
    return out


def arena_layout(h, w):
    """A restatement of the arena of include/ibgs_lpips.h -> (total bytes, {stage name: float offset of [x | y]}, byte offset of the partials)."""
    sides = [(h, w)]
    for _ in range(4):
        sides.append((sides[-1][0] // 2, sides[-1][1] // 2))
    n = [2 * c * hh * ww for c, (hh, ww) in zip(TAP_CHANNELS, sides)]
    q, p = 0, n[0]
    r3, r4 = p + n[2], p + n[2] + n[3]
    assert 2 * n[1] <= n[0] and 2 * n[2] <= n[1] and 2 * n[3] <= n[2] and 3 * n[4] <= n[3]          # every nesting fits
    at = dict(zip(CONVS, (p, q, p, p + n[1], p, r3, p, r3, r4, r3, r4, r4 + n[4], r4 + 2 * n[4])))
    partials = sum((hh * ww + 255) // 256 for hh, ww in sides)
    total = 4 * 2 * n[0] + 8 * partials
    return (total + 127) // 128 * 128, at, 8 * n[0]
