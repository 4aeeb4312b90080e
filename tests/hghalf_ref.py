"""Restatements for the half-precision hourglass (ibgs_amd/hourglass.py with precision="float16", csrc/hghalf.hip; the operation: include/ibgs_hg_half.h).
Built on tests/hourglass_ref.py, which stays THE ARBITER (forward_ref: float64 on the UNROUNDED float32 input and parameters).

  autocast_composition  the network from torch.nn.functional ops under torch.autocast("cpu", dtype=torch.float16), every stage returned: what the reference
                        runs at test time (tests/golden/hghalf.npz pins that) and THE YARDSTICK of the device's distance from float64.  conv2d runs in half
                        (inputs, weights and bias cast), relu / max_pool2d / interpolate keep the half they get, cat of a half and the float32 x gives
                        float32, which the next convolution rounds.
  h16                   float32 -> binary16 -> float64: the rounding (to nearest even) of the operands.
  layer_f64             ONE layer in float64 on binary16-rounded operands (the input already pooled / upsampled / concatenated by the caller).
  layer_chain           the same layer as a float32 k-ordered multiply-add chain from the bias (tests/hourglass_ref._conv_chain) on the same rounded operands.
  ulp16                 the spacing of binary16 at a float64 value (subnormals: 2^-24)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import hourglass_ref as ref

CHECKED = ref.STAGES + ("residual",)


def h16(a):
    with np.errstate(over="ignore"):          # overflow becomes +-inf, as in torch
        return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float64)


def ulp16(v):
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def autocast_composition(x, params):
    """x: (1, 38, H, W) or (38, H, W) float32; params: float32 numpy.  -> dict of torch CPU tensors (batch dimension dropped; half but for what torch
    promotes), keys e1, e2, b, u2, d2, u1, d1, f, residual."""
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    p = {k: t(v) for k, v in params.items()}
    x = t(x).reshape(1, 38, x.shape[-2], x.shape[-1])
    conv = lambda v, name, pad: F.conv2d(v, p[name + "_w"], p[name + "_b"], padding=pad)
    s = {}
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
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


def d_ref(x, params, want=None):
    """-> (arbiter stages, {stage: max |autocast_composition - float64|}) for the stored stages and the residual."""
    want = ref.forward_ref(x, params) if want is None else want
    auto = autocast_composition(x, params)
    return want, {k: float(np.abs(auto[k].double().numpy() - want[k]).max()) for k in CHECKED}


def layer_f64(inputs, w, b, relu=True):
    """inputs (Cin, h, w): any float values, rounded to binary16 here; w (Cout, Cin, k, k), b (Cout): float32, rounded here.  -> float64 (Cout, h, w)."""
    out = ref._conv_f64(h16(inputs), h16(w), h16(b))
    return np.maximum(out, 0) if relu else out


def layer_chain(inputs, w, b, relu=True):
    out = ref._conv_chain(h16(inputs).astype(np.float32), h16(w).astype(np.float32), h16(b).astype(np.float32))
    return np.maximum(out, 0) if relu else out


def layer_inputs(stages, x, layer):
    """The input of `layer` from a dict of stages (numpy, (C, h, w) each) and x (38, H, W): pool, up and the concatenations, exact."""
    h, w = x.shape[-2:]
    if layer == "enc1":
        return x
    if layer == "enc2":
        return ref.pool_ref(stages["e1"])
    if layer == "enc3":
        return ref.pool_ref(stages["e2"])
    if layer == "up2_conv":
        return ref.up_ref(stages["b"], h // 2, w // 2)
    if layer == "dec2":
        return np.concatenate([stages["u2"], stages["e2"]])
    if layer == "up1_conv":
        return ref.up_ref(stages["d2"], h, w)
    raise KeyError(layer)


# the stored stage each of the first six layers writes
LAYER_STAGE = (("enc1", "e1"), ("enc2", "e2"), ("enc3", "b"), ("up2_conv", "u2"), ("dec2", "d2"), ("up1_conv", "u1"))
