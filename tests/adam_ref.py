"""numpy restatement of the optimiser step (header of ibgs_amd/csrc/adam_math.h) and of the SH gradient from per-view factors (ibgs_sh_grad_from_views,
ibgs_amd/csrc/preprocess_bwd.hip).  Nothing here comes from ibgs_amd.  Every operation is one IEEE operation on operands of `dtype` (no python float reaches
such an expression), so with dtype = float32 `adam_step` is what the kernels compute, bit for bit (`adam_one` is compiled without contraction), and with
dtype = float64 it is the arbiter.  `sh_grad_from_views` states the sum; the kernels may contract its products, so it is compared by distance, not by bits."""
import math

import numpy as np


def adam_scalars(t, lr, betas, eps, dtype):
    """The per-tensor constants: formed in float64 (python floats), each rounded to `dtype` exactly once."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - math.pow(b1, float(t))
    bc2 = 1.0 - math.pow(b2, float(t))
    return {"b2": dtype(b2), "omb1": dtype(1.0 - b1), "omb2": dtype(1.0 - b2), "step_size": dtype(float(lr) / bc1),
            "inv_bc2_sqrt": dtype(1.0 / math.sqrt(bc2)), "eps": dtype(float(eps))}


def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-15, dtype=np.float32, parts=None):
    """Step number t (1-based) of Adam without weight decay or amsgrad; returns the new (p, m, v), the inputs stay as they were.
    parts: a dict that receives the intermediate `scaled` = sqrt(v) * inv_bc2_sqrt and `denom` = scaled + eps."""
    s = adam_scalars(t, lr, betas, eps, dtype)
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m = m + s["omb1"] * (g - m)
        v = s["b2"] * v + s["omb2"] * g * g
        scaled = np.sqrt(v) * s["inv_bc2_sqrt"]
        denom = scaled + s["eps"]
        p = p - s["step_size"] * (m / denom)
    if parts is not None:
        parts["scaled"], parts["denom"] = scaled, denom
    assert p.dtype == m.dtype == v.dtype == np.dtype(dtype)
    return p, m, v


# Real spherical harmonics up to l = 3 in the sign and order convention of the reference (Y_l^m for m = -l .. l, Condon-Shortley signs folded into the constants)
_PI = math.pi
C0 = 0.5 / math.sqrt(_PI)
C1 = math.sqrt(3.0 / (4.0 * _PI))
C2 = (0.5 * math.sqrt(15.0 / _PI), -0.5 * math.sqrt(15.0 / _PI), 0.25 * math.sqrt(5.0 / _PI), -0.5 * math.sqrt(15.0 / _PI), 0.25 * math.sqrt(15.0 / _PI))
C3 = (-0.25 * math.sqrt(35.0 / (2.0 * _PI)), 0.5 * math.sqrt(105.0 / _PI), -0.25 * math.sqrt(21.0 / (2.0 * _PI)), 0.25 * math.sqrt(7.0 / _PI),
      -0.25 * math.sqrt(21.0 / (2.0 * _PI)), 0.25 * math.sqrt(105.0 / _PI), -0.25 * math.sqrt(35.0 / (2.0 * _PI)))


def sh_basis(degree, dirs, dtype=np.float64):
    """dirs (N, 3) unit vectors -> (N, (degree + 1)^2) basis values."""
    d = np.asarray(dirs, dtype)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c = lambda a: dtype(a)
    B = [np.full(x.shape, c(C0), dtype)]
    if degree > 0:
        B += [-c(C1) * y, c(C1) * z, -c(C1) * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B += [c(C2[0]) * xy, c(C2[1]) * yz, c(C2[2]) * (c(2.0) * zz - xx - yy), c(C2[3]) * xz, c(C2[4]) * (xx - yy)]
    if degree > 2:
        B += [c(C3[0]) * y * (c(3.0) * xx - yy), c(C3[1]) * xy * z, c(C3[2]) * y * (c(4.0) * zz - xx - yy),
              c(C3[3]) * z * (c(2.0) * zz - c(3.0) * xx - c(3.0) * yy), c(C3[4]) * x * (c(4.0) * zz - xx - yy),
              c(C3[5]) * z * (xx - yy), c(C3[6]) * x * (xx - c(3.0) * yy)]
    out = np.stack(B, axis=1)
    assert out.dtype == np.dtype(dtype)
    return out


def sh_grad_from_views(means, camposes, dcolor, degree, M, dtype=np.float64):
    """means (P, 3), camposes (V, 3), dcolor (V, P, 3) -> (P, M, 3): sum over the views, in index order, of basis(normalise(mean - campos_v)) (x) dcolor_v;
    zero for the coefficients above (degree + 1)^2."""
    means, camposes, dcolor = (np.asarray(a, dtype) for a in (means, camposes, dcolor))
    P, nb = means.shape[0], (degree + 1) ** 2
    assert nb <= M and dcolor.shape == (camposes.shape[0], P, 3)
    out = np.zeros((P, M, 3), dtype)
    for v in range(camposes.shape[0]):
        d = means - camposes[v][None, :]
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        B = sh_basis(degree, d / length[:, None], dtype)
        out[:, :nb, :] = out[:, :nb, :] + B[:, :, None] * dcolor[v][:, None, :]
    return out


def adam_step_sh(tensors, k0s, t, lrs, grad=None, means=None, camposes=None, dcolor=None, degree=None, betas=(0.9, 0.999), eps=1e-15, dtype=np.float32):
    """The coefficient tensors [(p, m, v)] of shapes (P, K, 3), tensor j holding coefficients k0s[j] .. k0s[j] + K - 1, stepped (step numbers t[j], learning rates
    lrs[j]) on the gradient of the factors -- or on `grad` (P, M, 3) where the caller already holds it.  Returns the new [(p, m, v)]."""
    if grad is None:
        M = max(k0 + ten[0].shape[1] for k0, ten in zip(k0s, tensors))
        grad = sh_grad_from_views(means, camposes, dcolor, degree, M, dtype)
    out = []
    for (p, m, v), k0, tj, lr in zip(tensors, k0s, t, lrs):
        K = p.shape[1]
        out.append(adam_step(p, np.ascontiguousarray(grad[:, k0:k0 + K, :]), m, v, tj, lr, betas, eps, dtype))
    return out
