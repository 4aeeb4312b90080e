"""Restatements of the backward of the hourglass CNN (ibgs_amd/hourglass.py `hourglass_backward`, csrc/hgtrain.hip), written from its definition
(include/ibgs_hg_train.h), one code path with the primitives swapped, as tests/hourglass_ref._network:

  backward_ref        float64 numpy: THE ARBITER.  The decisions (ReLU masks, the pools' argmax) are taken from the stages it is handed; d1 and f are
                      recomputed in float64.
  backward_chain_f32  float32: every input-gradient element is ONE singly rounded multiply-add chain over (output channel, tap), every weight- and
                      bias-gradient element one chain over the pixels in row-major order; d1 and f are tests/hourglass_ref's float32 chains.  The routing
                      copies (pool^T) or adds in float32 (up^T, the skip sums).
  torch_grads         torch autograd of the functional composition on the CPU at a chosen dtype.

All return {"x": (38, H, W), "enc1_w": ..., ..., "final_b": ...}: the nineteen gradients.  `preacts_f64` and `decided` state when float64 and float32
differentiate the same function (every ReLU and pool decision is out of float32's reach)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import hourglass_ref as ref

GRADS = ("x",) + tuple(n + s for n, _, _, _ in ref.LAYERS for s in ("_w", "_b"))
RELU_STAGES = ref.STAGES + ("d1", "f")


# ---- routing ---------------------------------------------------------------------------------------------------------------------------------------------
def pool_bwd(g_pool, t):
    """g_pool: (c, h // 2, w // 2); t: (c, h, w), the pooled tensor.  The gradient lands on the FIRST maximum of a window in row-major order."""
    c, h, w = t.shape
    h2, w2 = h // 2, w // 2
    win = t[:, :2 * h2, :2 * w2].reshape(c, h2, 2, w2, 2).transpose(0, 1, 3, 2, 4).reshape(c, h2, w2, 4)
    first = np.argmax(win, axis=-1)          # (numpy's argmax returns the first of equal maxima)
    out = np.zeros((c, h, w), dtype=g_pool.dtype)
    for k in range(4):
        out[:, (k >> 1):2 * h2:2, (k & 1):2 * w2:2] = np.where(first == k, g_pool, 0)
    return out


def up_bwd(g_up, hin, win):
    """g_up: (c, h, w) -> (c, hin, win): the sum over the children of the integer rule, rows first, in g_up's dtype."""
    c, h, w = g_up.shape
    iy, ix = ref.up_index(h, hin), ref.up_index(w, win)
    rows = np.zeros((c, hin, w), dtype=g_up.dtype)
    for y in range(h):
        rows[:, iy[y]] += g_up[:, y]
    out = np.zeros((c, hin, win), dtype=g_up.dtype)
    for x in range(w):
        out[:, :, ix[x]] += rows[:, :, x]
    return out


# ---- one layer -------------------------------------------------------------------------------------------------------------------------------------------
def _pad(t, pad, dtype):
    c, h, w = t.shape
    out = np.zeros((c, h + 2 * pad, w + 2 * pad), dtype=dtype)
    out[:, pad:pad + h, pad:pad + w] = t
    return out


def _layer_f64(inp, wt, G, need_input=True):
    """-> (dW, db, g_I) of a k x k layer (k = 1 or 3) in float64."""
    cout, cin, k, _ = wt.shape
    c, h, w = inp.shape
    pad = k // 2
    ip, gp = _pad(inp, pad, np.float64), _pad(G, pad, np.float64)
    dw = np.zeros(wt.shape, dtype=np.float64)
    gi = np.zeros((cin, h, w), dtype=np.float64)
    w64 = wt.astype(np.float64)
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = np.einsum("ohw,ihw->oi", G, ip[:, ky:ky + h, kx:kx + w])
            if need_input:
                gi += np.einsum("oi,ohw->ihw", w64[:, :, ky, kx], gp[:, 2 * pad - ky:2 * pad - ky + h, 2 * pad - kx:2 * pad - kx + w])
    return dw, G.sum(axis=(1, 2)), gi


def _layer_chain(inp, wt, G, need_input=True):
    """The same in float32 chains: g_I over (output channel, tap), dW and db over the pixels in row-major order; every step rounded once."""
    cout, cin, k, _ = wt.shape
    c, h, w = inp.shape
    pad = k // 2
    ip, gp = _pad(inp, pad, np.float32), _pad(G, pad, np.float32)
    gi = np.zeros((cin, h, w), dtype=np.float32)
    if need_input:
        for o in range(cout):
            for ky in range(k):
                for kx in range(k):
                    prod = wt[o, :, ky, kx].astype(np.float64)[:, None, None] * gp[o, 2 * pad - ky:2 * pad - ky + h, 2 * pad - kx:2 * pad - kx + w].astype(np.float64)[None]
                    gi = (gi.astype(np.float64) + prod).astype(np.float32)
    dw = np.zeros(wt.shape, dtype=np.float32)
    db = np.zeros(cout, dtype=np.float32)
    G64 = G.astype(np.float64)
    for y in range(h):
        for x in range(w):
            g = G64[:, y, x]
            dw = (dw.astype(np.float64) + g[:, None, None, None] * ip[:, y:y + k, x:x + k].astype(np.float64)[None]).astype(np.float32)
            db = (db.astype(np.float64) + g).astype(np.float32)
    return dw, db, gi


def _backward(x, p, stages, g_res, g_ip, burned, layer, conv, dtype, need_input=True):
    x = np.asarray(x, dtype=dtype).reshape(38, x.shape[-2], x.shape[-1])
    h, w = x.shape[1:]
    s = {k: np.asarray(stages[k], dtype=dtype) for k in ref.STAGES}
    relu = lambda t: np.maximum(t, 0)
    live = lambda t: (t > 0).astype(dtype)
    zero = np.zeros((3, h, w), dtype=dtype)
    gr = zero if g_res is None else np.asarray(g_res, dtype=dtype)
    gp = zero if g_ip is None else np.asarray(g_ip, dtype=dtype)
    g = gr + gp if (g_res is not None and g_ip is not None) else (gr if g_ip is None else gp)
    out = {}
    cat1 = np.concatenate([s["u1"], s["e1"]])
    d1 = relu(conv(cat1, p["dec1_w"], p["dec1_b"]))
    cat0 = np.concatenate([d1, x])
    f = relu(conv(cat0, p["fuse_input_w"], p["fuse_input_b"]))
    out["final_w"], out["final_b"], g_f = layer(f, p["final_w"], g)
    g_f = g_f * live(f)
    out["fuse_input_w"], out["fuse_input_b"], g_cat = layer(cat0, p["fuse_input_w"], g_f)
    G_d1 = g_cat[:38] * live(d1)
    g_x = g_cat[38:].copy()
    if g_ip is not None:
        g_x[35:] = g_x[35:] + np.asarray(burned, dtype=dtype) * gp
    out["dec1_w"], out["dec1_b"], gi = layer(cat1, p["dec1_w"], G_d1)
    G_u1, g_e1a = gi[:38] * live(s["u1"]), gi[38:]
    out["up1_conv_w"], out["up1_conv_b"], gi = layer(ref.up_ref(s["d2"], h, w), p["up1_conv_w"], G_u1)
    G_d2 = up_bwd(gi, h // 2, w // 2) * live(s["d2"])
    out["dec2_w"], out["dec2_b"], gi = layer(np.concatenate([s["u2"], s["e2"]]), p["dec2_w"], G_d2)
    G_u2, g_e2a = gi[:19] * live(s["u2"]), gi[19:]
    out["up2_conv_w"], out["up2_conv_b"], gi = layer(ref.up_ref(s["b"], h // 2, w // 2), p["up2_conv_w"], G_u2)
    G_b = up_bwd(gi, h // 2 // 2, w // 2 // 2) * live(s["b"])
    out["enc3_w"], out["enc3_b"], gi = layer(ref.pool_ref(s["e2"]), p["enc3_w"], G_b)
    G_e2 = (g_e2a + pool_bwd(gi, s["e2"])) * live(s["e2"])
    out["enc2_w"], out["enc2_b"], gi = layer(ref.pool_ref(s["e1"]), p["enc2_w"], G_e2)
    G_e1 = (g_e1a + pool_bwd(gi, s["e1"])) * live(s["e1"])
    out["enc1_w"], out["enc1_b"], gi = layer(x, p["enc1_w"], G_e1, need_input)
    out["x"] = g_x + gi
    assert sorted(out) == sorted(GRADS)
    return out


def backward_ref(x, params, stages, g_res, g_ip, burned=1.0):
    """The arbiter: float64.  stages: a dict with e1, e2, b, u2, d2, u1 (more keys are ignored); g_res, g_ip: (3, H, W) or None (not both)."""
    return _backward(x, params, stages, g_res, g_ip, burned, _layer_f64, ref._conv_f64, np.float64)


def backward_chain_f32(x, params, stages, g_res, g_ip, burned=1.0):
    return _backward(x, params, stages, g_res, g_ip, burned, _layer_chain, ref._conv_chain, np.float32)


def torch_grads(x, params, g_res, g_ip, burned, dtype):
    """Autograd of the functional composition (tests/hourglass_ref.torch_composition's network) on the CPU.  -> the nineteen gradients as numpy arrays."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    p = {k: t(v).requires_grad_(True) for k, v in params.items()}
    x = t(x).reshape(1, 38, x.shape[-2], x.shape[-1]).requires_grad_(True)
    conv = lambda v, name, pad: F.conv2d(v, p[name + "_w"], p[name + "_b"], padding=pad)
    e1 = F.relu(conv(x, "enc1", 1))
    e2 = F.relu(conv(F.max_pool2d(e1, 2), "enc2", 1))
    b = F.relu(conv(F.max_pool2d(e2, 2), "enc3", 1))
    u2 = F.relu(conv(F.interpolate(b, size=e2.shape[-2:], mode="nearest"), "up2_conv", 1))
    d2 = F.relu(conv(torch.cat([u2, e2], 1), "dec2", 1))
    u1 = F.relu(conv(F.interpolate(d2, size=e1.shape[-2:], mode="nearest"), "up1_conv", 1))
    d1 = F.relu(conv(torch.cat([u1, e1], 1), "dec1", 1))
    f = F.relu(conv(torch.cat([d1, x], 1), "fuse_input", 0))
    residual = conv(f, "final", 0)[0]
    image_pred = float(burned) * x[0, 35:38] + residual
    loss = 0
    if g_res is not None:
        loss = loss + (residual * t(g_res)).sum()
    if g_ip is not None:
        loss = loss + (image_pred * t(g_ip)).sum()
    names = [k for k in GRADS if k != "x"]
    grads = torch.autograd.grad(loss, [x] + [p[k] for k in names])
    out = {"x": grads[0][0].numpy()}
    out.update({k: v.numpy() for k, v in zip(names, grads[1:])})
    return out


# ---- decided cases -------------------------------------------------------------------------------------------------------------------------------------------
def preacts_f64(x, p):
    """-> ({stage: pre-activation} for the eight ReLU layers, {stage: post-ReLU value}) in float64."""
    conv = ref._conv_f64
    relu = lambda t: np.maximum(t, 0)
    x = np.asarray(x, dtype=np.float64).reshape(38, x.shape[-2], x.shape[-1])
    h, w = x.shape[1:]
    pre, s = {}, {}
    def step(name, layer, inp):
        pre[name] = conv(inp, p[layer + "_w"], p[layer + "_b"])
        s[name] = relu(pre[name])
    step("e1", "enc1", x)
    step("e2", "enc2", ref.pool_ref(s["e1"]))
    step("b", "enc3", ref.pool_ref(s["e2"]))
    step("u2", "up2_conv", ref.up_ref(s["b"], h // 2, w // 2))
    step("d2", "dec2", np.concatenate([s["u2"], s["e2"]]))
    step("u1", "up1_conv", ref.up_ref(s["d2"], h, w))
    step("d1", "dec1", np.concatenate([s["u1"], s["e1"]]))
    step("f", "fuse_input", np.concatenate([s["d1"], x]))
    return pre, s


def decided(x, p, d_ref):
    """Whether float32 cannot take another ReLU or pool decision than float64 on this case: every pre-activation of the eight ReLU layers is at least
    4 d_ref(stage) from zero, and every pool window with a positive maximum has a gap of at least 8 d_ref(stage) to its second value.  d_ref: {stage: the
    case's forward yardstick} for e1, e2, b, u2, d2, u1, d1, f."""
    pre, s = preacts_f64(x, p)
    for k in RELU_STAGES:
        if np.abs(pre[k]).min() < 4 * d_ref[k]:
            return False
    for k in ("e1", "e2"):
        t = s[k]
        c, h, w = t.shape
        h2, w2 = h // 2, w // 2
        win = np.sort(t[:, :2 * h2, :2 * w2].reshape(c, h2, 2, w2, 2).transpose(0, 1, 3, 2, 4).reshape(c, h2, w2, 4), axis=-1)
        top, second = win[..., 3], win[..., 2]
        if ((top > 0) & (top - second < 8 * d_ref[k])).any():
            return False
    return True
