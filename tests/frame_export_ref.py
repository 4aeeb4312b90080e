"""The numpy restatement of the frame export's rules (include/ibgs_export.h; ibgs_amd/frame_export.py): the yardstick of tests/test_gpu_frame_export.py, itself
checked against np.percentile and against the recorded run of the reference's own colorize (tests/test_frame_export_host.py, tests/golden/frame_export.npz).
Every operation is one float32 numpy operation, in the reference's order; nothing here is contracted because numpy does not contract."""
import numpy as np

F = np.float32
ZERO_RESIDUAL, NO_VALID = 1, 2


def _byte(t):
    """clamp to [0, 255] (a NaN: 0), truncate"""
    t = np.where(np.isnan(t), F(0), t)
    return np.clip(t, F(0), F(255)).astype(np.uint8)


def round_u8(x):
    """torchvision's save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8), elementwise on a float32 array"""
    x = np.asarray(x, F)
    t = x * F(255)
    t = t + F(0.5)
    return _byte(t)


def fma_u8(x):
    """what a kernel that contracted x * 255 + 0.5 into one fma would store: the exact x * 255 + 0.5 (float64 holds it), rounded ONCE to float32"""
    t = (np.asarray(x, F).astype(np.float64) * 255.0 + 0.5).astype(F)
    return _byte(t)


def truncate_u8(x):
    x = np.asarray(x, F)
    x = np.where(np.isnan(x), F(0), x)
    return _byte(np.clip(x, F(0), F(1)) * F(255))


def _hwc(planes, order="rgb"):
    planes = planes[::-1] if order == "bgr" else planes
    return np.ascontiguousarray(np.moveaxis(planes, 0, -1))


def to_u8(image, rule="round", order="rgb"):
    """(C, H, W) float32 -> (H, W, C) uint8"""
    return _hwc({"round": round_u8, "truncate": truncate_u8}[rule](image), order)


def normal_to_u8(normal):
    n = np.asarray(normal, F)
    t = (n + F(1)) / F(2)
    t = t * F(255)
    return _hwc(_byte(t))


def residual_vis_u8(residual):
    """-> (image, status)"""
    r = np.abs(np.asarray(residual, F))
    m = r.max()          # (of the bits of |r|: a NaN would win; the tests hold none)
    if m == 0:
        return np.zeros(r.shape[1:] + r.shape[:1], np.uint8), ZERO_RESIDUAL
    return _hwc(round_u8(r / m)), 0


def valid_mask(value, invalid_val=None, invalid_mask=None):
    value = np.asarray(value, F)
    ok = ~np.isnan(value)
    if invalid_val is not None:
        ok &= value != F(invalid_val)
    if invalid_mask is not None:
        ok &= np.asarray(invalid_mask).reshape(value.shape) == 0
    return ok


def percentile(values, qs, invalid_val=None, invalid_mask=None):
    """-> ((len(qs),) float32, status).  np.percentile's linear rule as numpy 2.x evaluates it for a float32 array, from the two order statistics."""
    values = np.asarray(values, F)
    v = np.sort(values[valid_mask(values, invalid_val, invalid_mask)].reshape(-1))
    n = v.size
    if n == 0:
        return np.zeros(len(qs), F), NO_VALID
    out = []
    for q in qs:
        q32 = F(q) / F(100)
        vi = F(n - 1) * q32
        lo = np.floor(vi)
        g = F(vi - lo)
        lo = min(int(lo), n - 1)
        hi = min(lo + 1, n - 1)
        a, b = v[lo], v[hi]
        d = F(b - a)
        out.append(F(b - F(d * F(F(1) - g))) if g >= F(0.5) else F(a + F(d * g)))
    return np.asarray(out, F) + F(0), 0          # (+ 0: a -0.0 result counts as +0.0)


def percentile_contracted(values, qs):
    """the same rule with its multiply-add pairs fused (a + d g and b - d (1 - g) each rounded ONCE): what a kernel compiled with contraction would return"""
    v = np.sort(np.asarray(values, F).reshape(-1))
    n = v.size
    out = []
    for q in qs:
        vi = F(n - 1) * (F(q) / F(100))
        lo = np.floor(vi)
        g = F(vi - lo)
        lo = min(int(lo), n - 1)
        a, b = v[lo], v[min(lo + 1, n - 1)]
        d = np.float64(F(b - a))          # (float64 holds a float32 product and its sum with a float32 exactly enough: 24 + 24 bits, one exponent apart)
        out.append(F(np.float64(b) - d * np.float64(F(F(1) - g))) if g >= F(0.5) else F(np.float64(a) + d * np.float64(g)))
    return np.asarray(out, F) + F(0)


def lookup(x, lut):
    """matplotlib's Colormap.__call__ for a float array with bytes=True, on its 256-entry table: (..., 3) uint8; NaN -> 0, 0, 0 (the `bad` colour)"""
    x = np.asarray(x, F)
    xa = x * F(256)
    nan = np.isnan(xa)
    safe = np.where(nan, F(0), xa)
    idx = np.where(safe == F(256), 255, np.where(safe < 0, 0, np.where(safe >= F(256), 255, np.clip(safe, 0, 255).astype(np.int64))))
    out = np.asarray(lut, np.uint8)[idx]
    out[nan] = 0
    return out


def colorize(value, lut, vmin=None, vmax=None, invalid_val=-99.0, invalid_mask=None, background=(128, 128, 128)):
    """utils/general_utils.py:153-184 -> ((H, W, 3) uint8, status)"""
    value = np.asarray(value, F)
    value = value.reshape(value.shape[-2:])
    if invalid_mask is not None:
        invalid_val = None
    ok = valid_mask(value, invalid_val, invalid_mask)
    status = 0
    if vmin is None or vmax is None:
        (p2, p85), status = percentile(value, (2, 85), invalid_val, invalid_mask)
    vmin = p2 if vmin is None else F(vmin)
    vmax = p85 if vmax is None else F(vmax)
    with np.errstate(all="ignore"):
        x = (value - vmin) / F(vmax - vmin) if vmin != vmax else value * F(0)
        img = lookup(x, lut)
    img[~ok] = np.asarray(background, np.uint8)
    return img, status


def quantize(x):
    return round_u8(x).astype(F) / F(255)


def export_frame(render, depth, normal, lut, gt=None, image_pred=None, residual=None, split="test"):
    """-> ({name: (H, W, 3) uint8}, status)"""
    out = {"render": to_u8(render) if split == "test" else to_u8(render, "truncate", "bgr")}
    status = 0
    if gt is not None:
        out["gt"] = to_u8(gt)
    if image_pred is not None:
        out["aggregate"] = to_u8(image_pred)
        out["residual"], s = residual_vis_u8(residual)
        status |= s
    out["depth"], s = colorize(depth, lut)
    status |= s
    out["normal"] = normal_to_u8(normal)
    return out, status


def fma_sensitive_inputs():
    """The float32 values within 4 ulps of (k + 0.5) / 255, k = 0 .. 254, for which the two-step rounding and a fused multiply-add store DIFFERENT bytes.
    The search comes back EMPTY, and not by accident (tests/test_frame_export_host.py gives the argument and checks it): the byte of rule 1 cannot tell a
    contracted kernel from an uncontracted one.  The percentile's interpolation can: `percentile_contracted`."""
    hits = []
    for k in range(255):
        c = F((k + 0.5) / 255.0)
        cand = [c]
        lo = hi = c
        for _ in range(4):
            lo, hi = np.nextafter(lo, F(-1)), np.nextafter(hi, F(2))
            cand += [lo, hi]
        cand = np.asarray(cand, F)
        differ = round_u8(cand) != fma_u8(cand)
        hits += list(cand[differ])
    return np.asarray(hits, F)


# ---- the inputs the host and the device tests share ----------------------------------------------------------------------------------------------------
SELECT_SIZES = (1, 2, 3, 4, 35, 100, 2145, 5064, 40000, 921600, 2073600)          # the sizes the rule was checked at against np.percentile


def depth_values(n, ties=False, seed=None):
    v = np.random.default_rng(n if seed is None else seed).gamma(2.0, 1.5, n).astype(F)
    if ties:
        v[::3] = 0
    return v


def _bits(u):
    return np.asarray(u, np.uint32).view(F)


def percentile_cases():
    """-> [(name, values, qs, invalid_val, invalid_mask)], small: every way the select can go wrong at a size a test runs in no time"""
    rng = np.random.default_rng(7)
    cases = [("n%d" % n, depth_values(n), (2, 85), None, None) for n in (1, 2, 3, 4, 2145)]
    cases.append(("four_qs", depth_values(2145, seed=3), (0, 50, 99.5, 100), None, None))
    cases.append(("one_q", depth_values(35), (37.5,), None, None))
    cases.append(("all_equal", np.full(100, 1.25, F), (2, 85), None, None))
    run = depth_values(200, seed=5) + F(1)
    run[:150] = 0
    cases.append(("ties_span_lo_and_hi", rng.permutation(run), (2, 50), None, None))
    cases.append(("low_10_bits_only", rng.permutation(_bits(0x40490000 + np.arange(1024))), (2, 85), None, None))
    top = np.arange(4, 2040, dtype=np.uint32) << 21          # every exponent, two mantissa bits: keys that differ in the first digit alone (no Inf, no NaN)
    cases.append(("top_11_bits_only", rng.permutation(np.concatenate([_bits(top[top < 0x7F800000]), -_bits(top[top < 0x7F800000])])), (2, 85), None, None))
    signed = np.concatenate([-depth_values(100, seed=8) - F(0.1), np.zeros(150, F), -np.zeros(150, F), depth_values(100, seed=9) + F(0.1)])
    cases.append(("both_zeros", rng.permutation(signed), (10, 50, 62.4), None, None))
    den = np.concatenate([_bits(np.arange(1, 400)), -_bits(np.arange(1, 300)), np.zeros(3, F)])
    cases.append(("denormals", rng.permutation(den), (2, 85), None, None))
    v = depth_values(999, seed=11)
    v[::3] = -99
    cases.append(("invalid_val", v, (2, 85), -99.0, None))
    cases.append(("invalid_mask", depth_values(999, seed=12), (2, 85), None, rng.random(999) < 0.4))
    cases.append(("val_and_mask", v, (2, 85), -99.0, (rng.random(999) < 0.2).astype(np.uint8)))
    cases.append(("all_invalid", np.full(50, -99, F), (2, 85), -99.0, None))
    w = depth_values(500, seed=13)
    w[[3, 77, 499]] = np.nan
    cases.append(("nan_among_values", w, (2, 85), None, None))
    return cases


def rule_inputs(h, w, seed=0):
    """(3, h, w) float32 for rules 1-3: the neighbourhoods of the rounding boundaries (k + 0.5) / 255 and k / 255, values below 0, above 1, exactly 0, 1 and
    0.5 / 255, +-1 and beyond, +-0.0, the rest uniform in [-0.2, 1.2]; the LAST element holds the largest magnitude."""
    rng = np.random.default_rng(100 * h + w + seed)
    x = rng.uniform(-0.2, 1.2, 3 * h * w).astype(F)
    special = [0.0, -0.0, 1.0, -1.0, 0.5 / 255, 2.0, -2.0, 1.0 + 2.0 ** -23, 255.5 / 255, 254.5 / 255, 0.5 - 2.0 ** -25, 1e-40, -1e-40, 1e30, -1e30]
    k = rng.integers(0, 255, 64)
    near = np.concatenate([np.nextafter(F((k + 0.5) / 255.0), F(j)) for j in (-1, 2)] + [F((k + 0.5) / 255.0), F(k / 255.0), np.nextafter(F(k / 255.0), F(-1))])
    pool = np.concatenate([np.asarray(special, F), near.astype(F)])
    m = min(pool.size, x.size)
    x[rng.permutation(x.size)[:m]] = pool[rng.permutation(pool.size)[:m]]
    x = x.reshape(3, h, w)
    if x.size > 1:
        x[-1, -1, -1] = -3.5 if np.abs(x).max() < 3.5 else F(-2) * np.abs(x).max()
    return x
