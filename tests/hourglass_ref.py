"""Restatements of the hourglass CNN (ibgs_amd/hourglass.py, csrc/hourglass.hip), written from its definition (include/ibgs_hourglass.h):

  forward_ref        float64 numpy, tap by tap, pool by slicing, `up` by the integer rule: THE ARBITER.  Returns every stage.
  torch_composition  the same network from torch.nn.functional ops (conv2d, max_pool2d, interpolate, cat) at a chosen dtype.
  chain_f32          float32 in which every convolution output is ONE k-ordered multiply-add chain started from the bias, each step rounded once
                     (acc = f32(f64(acc) + f64(w) f64(x)): the product of two floats is exact in float64) -- what the f32 matrix-core instruction is.

`params` is a dict of numpy arrays <layer>_w (Cout, Cin, k, k) and <layer>_b (Cout) for enc1, enc2, enc3, up2_conv, dec2, up1_conv, dec1, fuse_input, final."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = (("enc1", 38, 38, 3), ("enc2", 19, 38, 3), ("enc3", 9, 19, 3), ("up2_conv", 19, 9, 3), ("dec2", 19, 38, 3), ("up1_conv", 38, 19, 3), ("dec1", 38, 76, 3),
          ("fuse_input", 38, 76, 1), ("final", 3, 38, 1))
STAGES = ("e1", "e2", "b", "u2", "d2", "u1")
REFERENCE_NAMES = {name: (name if name == "final" else name + ".0") for name, _, _, _ in LAYERS}


def seeded_params(seed, bias_shift=0.0):
    """nn.Conv2d's default initialisation under a seed, as float32 numpy; bias_shift is added to every bias."""
    torch.manual_seed(seed)
    out = {}
    for name, cout, cin, k in LAYERS:
        conv = torch.nn.Conv2d(cin, cout, kernel_size=k)
        out[name + "_w"] = conv.weight.detach().numpy().copy()
        out[name + "_b"] = (conv.bias.detach() + bias_shift).numpy().astype(np.float32)
    return out


def pool_ref(t):
    c, h, w = t.shape
    t = t[:, :h // 2 * 2, :w // 2 * 2]
    return np.maximum(np.maximum(t[:, 0::2, 0::2], t[:, 0::2, 1::2]), np.maximum(t[:, 1::2, 0::2], t[:, 1::2, 1::2]))


def up_index(n_out, n_in):
    return np.minimum(np.arange(n_out, dtype=np.int64) * n_in // n_out, n_in - 1)


def up_ref(t, h, w):
    return t[:, up_index(h, t.shape[1])][:, :, up_index(w, t.shape[2])]


def _conv_f64(t, wt, bias):
    cout, cin, k, _ = wt.shape
    c, h, w = t.shape
    assert c == cin
    pad = k // 2
    tp = np.zeros((c, h + 2 * pad, w + 2 * pad), dtype=np.float64)
    tp[:, pad:pad + h, pad:pad + w] = t
    out = np.broadcast_to(bias.astype(np.float64)[:, None, None], (cout, h, w)).copy()
    for ky in range(k):
        for kx in range(k):
            out += np.einsum("oc,chw->ohw", wt[:, :, ky, kx].astype(np.float64), tp[:, ky:ky + h, kx:kx + w])
    return out


def _conv_chain(t, wt, bias):
    cout, cin, k, _ = wt.shape
    c, h, w = t.shape
    pad = k // 2
    tp = np.zeros((c, h + 2 * pad, w + 2 * pad), dtype=np.float32)
    tp[:, pad:pad + h, pad:pad + w] = t
    acc = np.broadcast_to(bias.astype(np.float32)[:, None, None], (cout, h, w)).copy()
    for ci in range(cin):
        for ky in range(k):
            for kx in range(k):
                prod = wt[:, ci, ky, kx].astype(np.float64)[:, None, None] * tp[ci, ky:ky + h, kx:kx + w].astype(np.float64)[None]
                acc = (acc.astype(np.float64) + prod).astype(np.float32)
    return acc


def _network(x, p, conv, dtype):
    relu = lambda t: np.maximum(t, 0)
    x = np.asarray(x, dtype=dtype).reshape(38, x.shape[-2], x.shape[-1])
    h, w = x.shape[1:]
    s = {}
    s["e1"] = relu(conv(x, p["enc1_w"], p["enc1_b"]))
    s["e2"] = relu(conv(pool_ref(s["e1"]), p["enc2_w"], p["enc2_b"]))
    s["b"] = relu(conv(pool_ref(s["e2"]), p["enc3_w"], p["enc3_b"]))
    s["u2"] = relu(conv(up_ref(s["b"], h // 2, w // 2), p["up2_conv_w"], p["up2_conv_b"]))
    s["d2"] = relu(conv(np.concatenate([s["u2"], s["e2"]]), p["dec2_w"], p["dec2_b"]))
    s["u1"] = relu(conv(up_ref(s["d2"], h, w), p["up1_conv_w"], p["up1_conv_b"]))
    s["d1"] = relu(conv(np.concatenate([s["u1"], s["e1"]]), p["dec1_w"], p["dec1_b"]))
    s["f"] = relu(conv(np.concatenate([s["d1"], x]), p["fuse_input_w"], p["fuse_input_b"]))
    s["residual"] = conv(s["f"], p["final_w"], p["final_b"])
    return s


def forward_ref(x, params, burned_in_gauss=1.0):
    """x: (1, 38, H, W) or (38, H, W).  -> dict of float64 arrays: e1, e2, b, u2, d2, u1, d1, f, residual, image_pred."""
    s = _network(x, params, _conv_f64, np.float64)
    xr = np.asarray(x, dtype=np.float64).reshape(38, x.shape[-2], x.shape[-1])
    s["image_pred"] = float(burned_in_gauss) * xr[35:38] + s["residual"]
    return s


def chain_f32(x, params):
    """-> the same dict (without image_pred) in float32 multiply-add chains."""
    return _network(x, params, _conv_chain, np.float32)


def torch_composition(x, params, dtype):
    """-> dict of torch CPU tensors of `dtype` (batch dimension dropped)."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    p = {k: t(v) for k, v in params.items()}
    x = t(x).reshape(1, 38, x.shape[-2], x.shape[-1])
    conv = lambda v, name, pad: F.conv2d(v, p[name + "_w"], p[name + "_b"], padding=pad)
    s = {}
    s["e1"] = F.relu(conv(x, "enc1", 1))
    s["e2"] = F.relu(conv(F.max_pool2d(s["e1"], 2), "enc2", 1))
    s["b"] = F.relu(conv(F.max_pool2d(s["e2"], 2), "enc3", 1))
    s["u2"] = F.relu(conv(F.interpolate(s["b"], size=s["e2"].shape[-2:], mode="nearest"), "up2_conv", 1))
    s["d2"] = F.relu(conv(torch.cat([s["u2"], s["e2"]], 1), "dec2", 1))
    s["u1"] = F.relu(conv(F.interpolate(s["d2"], size=s["e1"].shape[-2:], mode="nearest"), "up1_conv", 1))
    s["d1"] = F.relu(conv(torch.cat([s["u1"], s["e1"]], 1), "dec1", 1))
    s["f"] = F.relu(conv(torch.cat([s["d1"], x], 1), "fuse_input", 0))
    s["residual"] = conv(s["f"], "final", 0)
    return {k: v[0] for k, v in s.items()}


def seeded_input(seed, h, w, signed=False):
    """A cnn_input as the front end makes it: 32 non-negative features (arbitrary sign with `signed`), a unit ray, a colour in [0, 1]."""
    g = np.random.default_rng(seed)
    feat = g.standard_normal((32, h, w)) if signed else np.maximum(g.standard_normal((32, h, w)), 0) * 0.5
    ray = g.standard_normal((3, h, w))
    ray /= np.linalg.norm(ray, axis=0, keepdims=True)
    return np.concatenate([feat, ray, g.random((3, h, w))]).astype(np.float32)[None]
