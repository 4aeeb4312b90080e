"""Restatements for the half-precision backward of the hourglass (ibgs_amd/hourglass.py with precision="float16", csrc/hghtrain.hip; the operation:
include/ibgs_hg_half_train.h), built on tests/hourglass_bwd_ref.py and tests/hghalf_ref.py.

  backward_decided    float64 numpy on the UNROUNDED float32 parameters: THE ARBITER.  tests/hourglass_bwd_ref.backward_ref with every decision HANDED to it:
                      the eight ReLU masks (e1, e2, b, u2, d2, u1, d1, f as boolean arrays) and the two tensors whose 2 x 2 windows' first maximum routes the
                      pools' gradients.  A preactivation within binary16's reach of zero occurs in every frame, so no input exists on which a float64
                      recomputation and a binary16 one take the same decisions; one flipped sign moves a pixel's gradient by its whole size.  The values
                      (the layers' inputs, d1, f) stay those of the float64 forward it is handed.
  autocast_backward   THE YARDSTICK: the network in torch ops under torch.autocast("cpu", float16), forward and backward, the loss multiplied by 2^k and the
                      gradients divided by it in float32.  -> (the nineteen gradients, its own eight decision sets, its e1 and e2).
  scale_k             the automatic scale rule, restated: k = E_TARGET - floor(log2 max |g|); 0 when that maximum is zero or not finite."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import hourglass_bwd_ref as bref
from tests import hourglass_ref as ref

E_TARGET = 10
DECISIONS = bref.RELU_STAGES


def scale_k(m):
    m = float(np.float32(m))
    if m == 0.0 or not math.isfinite(m):
        return 0
    return E_TARGET - int(math.floor(math.log2(abs(m))))          # (log2 of a float32, subnormals included, is exact enough in double: its floor is the exponent)


def decisions_of(stages):
    """{stage: value > 0} for the eight ReLU stages of a dict that holds them"""
    return {k: np.asarray(stages[k]) > 0 for k in DECISIONS}


def backward_decided(x, p, stages, decisions, pool_from, g_res, g_ip, burned=1.0):
    """x, p: float32 (unrounded); stages: the float64 forward's e1, e2, b, u2, d2, u1; decisions: {stage: bool array} for the eight ReLU stages; pool_from:
    {"e1": ..., "e2": ...}, whose windows' first maxima route the pools; g_res, g_ip: (3, H, W) or None (not both).  -> the nineteen gradients, float64."""
    dtype = np.float64
    x = np.asarray(x, dtype=dtype).reshape(38, x.shape[-2], x.shape[-1])
    h, w = x.shape[1:]
    s = {k: np.asarray(stages[k], dtype=dtype) for k in ref.STAGES}
    live = lambda k: np.asarray(decisions[k]).astype(dtype)
    layer, conv = bref._layer_f64, ref._conv_f64
    zero = np.zeros((3, h, w), dtype=dtype)
    gr = zero if g_res is None else np.asarray(g_res, dtype=dtype)
    gp = zero if g_ip is None else np.asarray(g_ip, dtype=dtype)
    g = gr + gp
    out = {}
    cat1 = np.concatenate([s["u1"], s["e1"]])
    d1 = np.maximum(conv(cat1, p["dec1_w"], p["dec1_b"]), 0)
    cat0 = np.concatenate([d1, x])
    f = np.maximum(conv(cat0, p["fuse_input_w"], p["fuse_input_b"]), 0)
    out["final_w"], out["final_b"], g_f = layer(f, p["final_w"], g)
    g_f = g_f * live("f")
    out["fuse_input_w"], out["fuse_input_b"], g_cat = layer(cat0, p["fuse_input_w"], g_f)
    G_d1 = g_cat[:38] * live("d1")
    g_x = g_cat[38:].copy()
    if g_ip is not None:
        g_x[35:] = g_x[35:] + float(burned) * gp
    out["dec1_w"], out["dec1_b"], gi = layer(cat1, p["dec1_w"], G_d1)
    G_u1, g_e1a = gi[:38] * live("u1"), gi[38:]
    out["up1_conv_w"], out["up1_conv_b"], gi = layer(ref.up_ref(s["d2"], h, w), p["up1_conv_w"], G_u1)
    G_d2 = bref.up_bwd(gi, h // 2, w // 2) * live("d2")
    out["dec2_w"], out["dec2_b"], gi = layer(np.concatenate([s["u2"], s["e2"]]), p["dec2_w"], G_d2)
    G_u2, g_e2a = gi[:19] * live("u2"), gi[19:]
    out["up2_conv_w"], out["up2_conv_b"], gi = layer(ref.up_ref(s["b"], h // 2, w // 2), p["up2_conv_w"], G_u2)
    G_b = bref.up_bwd(gi, h // 2 // 2, w // 2 // 2) * live("b")
    out["enc3_w"], out["enc3_b"], gi = layer(ref.pool_ref(s["e2"]), p["enc3_w"], G_b)
    G_e2 = (g_e2a + bref.pool_bwd(gi, np.asarray(pool_from["e2"], dtype=dtype))) * live("e2")
    out["enc2_w"], out["enc2_b"], gi = layer(ref.pool_ref(s["e1"]), p["enc2_w"], G_e2)
    G_e1 = (g_e1a + bref.pool_bwd(gi, np.asarray(pool_from["e1"], dtype=dtype))) * live("e1")
    out["enc1_w"], out["enc1_b"], gi = layer(x, p["enc1_w"], G_e1)
    out["x"] = g_x + gi
    out["_G"] = {"gS": g, "f": g_f, "d1": G_d1, "u1": G_u1, "d2": G_d2, "u2": G_u2, "b": G_b, "e2": G_e2, "e1": G_e1}          # the pre-activation gradients, for the exponent table
    return out


def autocast_backward(x, params, g_res, g_ip, burned, k):
    """-> ({name: float32 numpy gradient}, {stage: bool numpy}, {"e1": ..., "e2": ...} float64 numpy): torch's CPU autocast run with the loss scaled by 2^k."""
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    p = {name: t(v).requires_grad_(True) for name, v in params.items()}
    x = t(x).reshape(1, 38, x.shape[-2], x.shape[-1]).requires_grad_(True)
    conv = lambda v, name, pad: F.conv2d(v, p[name + "_w"], p[name + "_b"], padding=pad)
    s = {}
    with torch.autocast("cpu", dtype=torch.float16):
        s["e1"] = F.relu(conv(x, "enc1", 1))
        s["e2"] = F.relu(conv(F.max_pool2d(s["e1"], 2), "enc2", 1))
        s["b"] = F.relu(conv(F.max_pool2d(s["e2"], 2), "enc3", 1))
        s["u2"] = F.relu(conv(F.interpolate(s["b"], size=s["e2"].shape[-2:], mode="nearest"), "up2_conv", 1))
        s["d2"] = F.relu(conv(torch.cat([s["u2"], s["e2"]], 1), "dec2", 1))
        s["u1"] = F.relu(conv(F.interpolate(s["d2"], size=s["e1"].shape[-2:], mode="nearest"), "up1_conv", 1))
        s["d1"] = F.relu(conv(torch.cat([s["u1"], s["e1"]], 1), "dec1", 1))
        s["f"] = F.relu(conv(torch.cat([s["d1"], x], 1), "fuse_input", 0))
        residual = conv(s["f"], "final", 0)[0]
    image_pred = float(burned) * x[0, 35:38] + residual.float()
    scale = 2.0 ** k
    loss = 0
    if g_res is not None:
        loss = loss + (residual.float() * (t(g_res) * scale)).sum()
    if g_ip is not None:
        loss = loss + (image_pred * (t(g_ip) * scale)).sum()
    names = [n for n in bref.GRADS if n != "x"]
    grads = torch.autograd.grad(loss, [x] + [p[n] for n in names])
    out = {"x": (grads[0][0].float() / scale).numpy()}
    out.update({n: (v.float() / scale).numpy() for n, v in zip(names, grads[1:])})
    decisions = {name: (v[0] > 0).numpy() for name, v in s.items()}
    return out, decisions, {name: s[name][0].detach().double().numpy() for name in ("e1", "e2")}
