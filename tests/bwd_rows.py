"""The per-Gaussian backward (csrc/preprocess_bwd.hip, stages B3 + B4) held row by row: numpy and the oracle only, nothing from the kernels.

The stage turns one 16-float accumulation row per Gaussian (written by csrc/render_bwd.hip) into every gradient of the operator.  `intermediates` restates in
float64 what the stage derives from a row before the chain starts, `chain` runs the oracle's own per-Gaussian stage (orc_preprocess_backward) on them in a
named build, `row_verdict` judges every row of every output against the float64 build with the fp32 builds' own distance from it as the unit, and
`check_short` holds the outputs that are one to three operations away from the row to a bound derived from the number of roundings.

THE ROW BAR.  Per output array X and per visible row i whose float64 value is not all zero
    r(.)_i  = |X_i - X64_i|_inf / |X64_i|_inf
    rho_i   = max of r_i over the fp32 reference evaluations ("plain": no contraction; "fma": gcc contracts where it likes)
    rho_bar = the median of rho over the array's rows
    a row passes iff r_i(hip) <= K * max(rho_i, rho_bar);  rows whose float64 value is all zero must be all zero (the sign bit ignored).
No share of rows is left out.

K = 64.  Measured on the CPU from the references alone (tests/test_bwd_rows_host.py::test_fp32_builds_meet_each_others_row_bar keeps the measurement as a
test): the fma build judged by this rule with the plain build as the only reference, and the other way round, on the stage alone with identical rows, over
every case of tests/test_gpu_bwd_rows.py (`seeded_cases`: every column group under both scale modifiers, every layout, the ends, the needle scene under both
row formats) and over the blend's own rows of the base and the needle scene (oracle.backward's accumulators; near-singular conics left out there, see
RA_LFORM below).  Every call is judged PER FORMAT CLASS, as the GPU tests judge: the near-singular rows and the ordinary rows of the needle scene each with
the rho_bar of their own class.  Worst ratio r_i / max(rho_i, rho_bar) per array, fp32 references only:
                     all classes   without the needle scene   RA_ASSOC rows on needles, as a class of their own
    dL_dmeans3D        16.2            13.8                       16.2
    dL_dcov3D          16.7             8.1                        7.3
    dL_dsh              2.4             2.4                        1.7
    dL_dscales         19.7             8.8                        7.3
    dL_drotations      10.4             8.9                        7.2
K is the smallest power of two that is at least twice the worst of them (2 x 19.7 = 39.4 -> 64).  With a single reference rho_i is that reference's own error, so
the ratio says how much worse than its twin a sound fp32 evaluation can look in one row; the HIP path is a third such evaluation, contracted in a pattern of its own.
K also absorbs one error that is not in rho_i: the fp32 builds are fed the correctly rounded float64 dL_dmean2D, while the kernel forms it in float32 (up to four
roundings, and a*Sx + b*Sy may cancel) before it reaches dL_dmeans3D; `check_short` bounds that error at its source.
The median row error rho_bar is 8e-8 .. 2.2e-7 on the base scene and 1e-5 .. 3e-4 on the needle scene (single rows up to 1e-2: the chain inverts a near-singular cov2D).

THE RA_ASSOC CLASS (near-singular conics under IBGS_FLAG_REF_ARITH: the reference's ill-conditioned chain, run on purpose) measures a worst ratio of 16.2 as a
class of its own, i.e. a K of its own of 64 (2 x 16.2 = 32.4): not above 64, so the class stays under the row bar.  (Judged in ONE pool with the ordinary rows of
the same call it would show 33.3, a K of 128: the pool's rho_bar is then the ordinary rows' 1e-5, ten times below the class's own -- which is why no test here pools
the two.)  Because its rho_bar is 1e-4 .. 1e-3 and the row bar correspondingly wide there, the class is ALSO held to the whole-array arbiter rule of
tests/test_gpu_anisotropic.py (`array_verdict`: relative L2 over the class's rows, |HIP - f64| <= max(1e-3, 2 x |plain - f64|)).
RA_LFORM rows have ONE fp32 reference (oracle.variant("lform"); the float64 side is variant("f64_lform")), so no ratio can be measured on them; they are held to
the same K.  Their optional dL_dconic output is rebuilt from cov2D, which this file restates in numpy in both precisions (`cov2d`, `lform_conic`).

Planted mistakes (a one-off experiment with scratch copies of the oracle's C source standing in for the HIP side, nothing of it kept): at K = 64, on the base scene,
the verdict flags frustum-clamp masks ignored (569 rows with seeded rows, 183 with the blend's own), the SH clamp mask ignored (176 / 41), one degree-3 term of the
direction gradient dropped (1309 / 343) and one sign flipped in dL_drot (1347 / 349); the unmodified build: 0."""
import functools

import numpy as np

import oracle
from ibgs_amd import synthetic as syn
from tests.scenes import scene

K = 64.0
F64_K = 2.0          # the whole-array arbiter's factor and floor (tests/test_gpu_anisotropic.py: F64_K, base_tol), for the RA_ASSOC class
ARBITER_FLOOR = 1e-3

# csrc/common.h:112-113   constexpr float EXP2_SCALE = 0.5f * 1.4426950408889634f;  constexpr float EXP2_UNSCALE = 1.0f / EXP2_SCALE;
EXP2_UNSCALE = np.float32(1.0) / (np.float32(0.5) * np.float32(1.4426950408889634))
# csrc/common.h:140-141   constexpr float BLEND_REF_POWER_RISK = 0.999f;  risky iff b * b > BLEND_REF_POWER_RISK * (a * c), in float
BLEND_REF_POWER_RISK = np.float32(0.999)

ORDINARY, LFORM, ASSOC = 0, 1, 2
FORMATS = {"ordinary": ORDINARY, "lform": LFORM, "assoc": ASSOC}
EPS = 2.0 ** -24          # half an ulp of a float32 in [1, 2): the relative error bound of one rounding

# Per-column scales of the non-zero accumulation rows of a real backward (the base scene, dL/dcolor and dL/dnormal ~ N(0, 1); from oracle.backward's accumulators
# through `rows_from_accumulators`): the median magnitude / 0.6745 of each column -- the rows are heavy-tailed, their standard deviations are 10^2 .. 10^3 times
# larger.  0 Sx, 1 Sy, 2 Ax, 3 Ay, 4 Sxx, 5 Sxy, 6 Syy, 7 S0, 8-10 rgb, 11-13 normal, 14 dist (given the normals' scale), 15 unused.
COLUMN_SCALE = np.array([0.17, 0.13, 0.0073, 0.0062, 8.6, 5.4, 5.5, 0.0039, 0.0044, 0.0044, 0.0042, 0.0046, 0.0039, 0.0034, 0.004, 0.0], np.float32)
GROUPS = {"mean": (0, 1, 2, 3), "cov": (4, 5, 6), "opacity": (7,), "sh": (8, 9, 10), "all_map": (11, 12, 13, 14), "all": tuple(range(15))}

CHAIN_OUTPUTS = ("dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
SHORT_OUTPUTS = ("dL_dmeans2D", "dL_dmeans2D_abs", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dall_map")


# ---- what the stage derives from a row ---------------------------------------------------------------------------------------------------------------
def near_singular(rec):
    """Which conics the kernels treat as near-singular: their own test, in float32 on the record's values."""
    a, b, c = (np.ascontiguousarray(rec[:, k], np.float32) for k in (4, 5, 6))
    return b * b > BLEND_REF_POWER_RISK * (a * c)


def cov2d(inp, cov3D, dtype):
    """cov2D = A Sigma A^T + 0.3 I of every Gaussian, (a, b, c) as (P,3) in `dtype`, operation by operation as forward.cu:112-150 writes it (A = J W with the
    frustum clamp of t).  float32: one fp32 evaluation without contraction; float64: the exact side."""
    f = dtype
    m = np.asarray(inp["means3D"], f).reshape(-1, 3); vm = np.asarray(inp["viewmatrix"], np.float32).reshape(-1).astype(f)
    W, H = int(inp["W"]), int(inp["H"]); tanx, tany = f(np.float32(inp["tanfovx"])), f(np.float32(inp["tanfovy"]))
    fx, fy = f(W) / (f(2.0) * tanx), f(H) / (f(2.0) * tany)
    t = [vm[k] * m[:, 0] + vm[4 + k] * m[:, 1] + vm[8 + k] * m[:, 2] + vm[12 + k] for k in range(3)]
    limx, limy = f(np.float32(1.3)) * tanx, f(np.float32(1.3)) * tany
    with np.errstate(all="ignore"):
        tx = np.minimum(limx, np.maximum(-limx, t[0] / t[2])) * t[2]
        ty = np.minimum(limy, np.maximum(-limy, t[1] / t[2])) * t[2]
        j00, j02 = fx / t[2], -(fx * tx) / (t[2] * t[2])
        j11, j12 = fy / t[2], -(fy * ty) / (t[2] * t[2])
        A = np.empty((2, 3) + t[2].shape, f)
        for r in range(3):
            A[0][r] = vm[4 * r] * j00 + vm[4 * r + 1] * f(0.0) + vm[4 * r + 2] * j02
            A[1][r] = vm[4 * r] * f(0.0) + vm[4 * r + 1] * j11 + vm[4 * r + 2] * j12
        c6 = np.asarray(cov3D, f).reshape(-1, 6)
        S = [[c6[:, 0], c6[:, 1], c6[:, 2]], [c6[:, 1], c6[:, 3], c6[:, 4]], [c6[:, 2], c6[:, 4], c6[:, 5]]]
        SA = [[S[r][0] * A[i][0] + S[r][1] * A[i][1] + S[r][2] * A[i][2] for r in range(3)] for i in range(2)]
        a = A[0][0] * SA[0][0] + A[0][1] * SA[0][1] + A[0][2] * SA[0][2] + f(np.float32(0.3))
        b = A[0][0] * SA[1][0] + A[0][1] * SA[1][1] + A[0][2] * SA[1][2]
        c = A[1][0] * SA[1][0] + A[1][1] * SA[1][1] + A[1][2] * SA[1][2] + f(np.float32(0.3))
    return np.stack([a, b, c], axis=1)


def intermediates(rows, rec, W, H, fmt, cov=None):
    """float64 restatement of what the stage derives from the 16-float rows before the chain starts (the contract of csrc/render_bwd.hip's rows).
    rows (P,16) float32: 0 Sx, 1 Sy, 2 Ax, 3 Ay, 4 Sxx, 5 Sxy, 6 Syy, 7 S0, 8-10 rgb, 11-13 normal, 14 dist;  rec (P,16): the forward's records ((a, b, c) =
    rec[:, 4:7], o = rec[:, 2]).  fmt = "ordinary" | "lform" | "assoc": the format in which the rows of NEAR-SINGULAR conics are read (every other row is ordinary).
    cov (P,3) float64: cov2D, needed only to rebuild dL_dconic of "lform" rows.
    Returns the six short outputs, "chain_conic" (P,4: what the chain takes in dL_dconic's place -- the conic gradient, or dL/dcov2D's (a, b, -, c) of lform rows),
    "cls" (P,) the format of every row, and "bound": per short output the allowed |error| of a float32 evaluation, (roundings + 1) * 2^-24 * sum |terms|
    (0 = a copy or an exact scaling: bit-equal)."""
    g = np.asarray(rows, np.float32).astype(np.float64); P = g.shape[0]
    a, b, c, o = (np.asarray(rec[:, k], np.float32).astype(np.float64) for k in (4, 5, 6, 2))
    cls = np.where(near_singular(rec), FORMATS[fmt], ORDINARY)
    u = float(EXP2_UNSCALE); hw, hh = 0.5 * W, 0.5 * H
    o_ = {k: np.zeros((P, n)) for k, n in (("dL_dmeans2D", 3), ("dL_dmeans2D_abs", 3), ("dL_dconic", 4), ("dL_dopacity", 1), ("dL_dcolors", 3), ("dL_dall_map", 5),
                                           ("chain_conic", 4))}
    bd = {k: np.zeros_like(o_[k]) for k in SHORT_OUTPUTS}
    od, lf, ra = cls == ORDINARY, cls == LFORM, cls == ASSOC
    # dL_dmean2D
    for col, half, (p, q, sp, sq) in ((0, hw, (a, b, g[:, 0], g[:, 1])), (1, hh, (c, b, g[:, 1], g[:, 0]))):
        v = np.where(od, -half * (p * sp + q * sq), np.where(lf, -half * (sp * u), half * sp))
        terms = np.where(od, half * (np.abs(p * sp) + np.abs(q * sq)), np.abs(v))
        nround = np.where(od, 4, np.where(lf, 2, 1))          # two products, their sum, the scaling | the unscale, the scaling | the scaling
        o_["dL_dmeans2D"][:, col] = v; bd["dL_dmeans2D"][:, col] = (nround + 1) * EPS * terms
    # its abs twin: the sums were formed with the conic in exp2 units (not so the reference's own sums of RA_ASSOC rows)
    for col, half in ((0, hw), (1, hh)):
        v = np.where(ra, half * g[:, 2 + col], half * (g[:, 2 + col] * u))
        o_["dL_dmeans2D_abs"][:, col] = v; bd["dL_dmeans2D_abs"][:, col] = (np.where(ra, 1, 2) + 1) * EPS * np.abs(v)
    # dL_dconic = -0.5 (Sxx, Sxy, 0, Syy): exact in float32
    for k, col in ((0, 4), (1, 5), (3, 6)):
        o_["dL_dconic"][:, k] = -0.5 * g[:, col]
    o_["chain_conic"][:] = o_["dL_dconic"]
    if lf.any():
        m = g[:, 4:7] * (u * u)          # sum q l l^T with the unscaled conic
        o_["chain_conic"][lf, 0] = 0.5 * m[lf, 0]; o_["chain_conic"][lf, 1] = m[lf, 1]; o_["chain_conic"][lf, 3] = 0.5 * m[lf, 2]
        o_["dL_dconic"][lf] = 0.0
        if cov is not None:          # d = cov2D l, so sum q d d^T = cov2D (sum q l l^T) cov2D  (preprocess_bwd.hip:270-274)
            o_["dL_dconic"][lf] = lform_conic(m, cov)[lf]
    # dL_dopacity = S0 / o (0 when o <= 0); RA_ASSOC rows hold the reference's own sum
    with np.errstate(all="ignore"):
        v = np.where(ra, g[:, 7], np.where(o > 0, g[:, 7] / np.where(o > 0, o, 1.0), 0.0))
    o_["dL_dopacity"][:, 0] = v; bd["dL_dopacity"][:, 0] = np.where(ra, 0.0, 2 * EPS * np.abs(v))
    o_["dL_dcolors"][:] = g[:, 8:11]
    o_["dL_dall_map"][:, 0:3] = g[:, 11:14]; o_["dL_dall_map"][:, 4] = g[:, 14]
    o_["cls"] = cls; o_["bound"] = bd
    return o_


def lform_conic(m, cov):
    """dL_dconic (P,4) of RA_LFORM rows from their second moments m (P,3: m00, m01, m11, unscaled) and cov2D (P,3), in the arrays' own precision."""
    a, b, c = cov[:, 0], cov[:, 1], cov[:, 2]; h = cov.dtype.type(0.5); two = cov.dtype.type(2.0)
    out = np.zeros((m.shape[0], 4), cov.dtype)
    out[:, 0] = -h * (a * a * m[:, 0] + two * a * b * m[:, 1] + b * b * m[:, 2])
    out[:, 1] = -h * (a * b * m[:, 0] + (a * c + b * b) * m[:, 1] + b * c * m[:, 2])
    out[:, 3] = -h * (b * b * m[:, 0] + two * b * c * m[:, 1] + c * c * m[:, 2])
    return out


def live_rows(rows, radii):
    """Gaussians the stage computes anything for: radius > 0 and a row that is not all (+-) zero."""
    return (np.asarray(radii).reshape(-1) > 0) & (np.asarray(rows, np.float32) != 0).any(axis=1)


def clamp_bits(clamped):
    """(P,3) uint8 flags <-> (P,) bit mask (bit ch = channel ch clamped), whichever is given -> (flags, bits)."""
    c = np.asarray(clamped, np.uint8)
    if c.ndim == 2:
        return c, (c[:, 0] | (c[:, 1] << 1) | (c[:, 2] << 2)).astype(np.uint8)
    return np.stack([(c >> k) & 1 for k in range(3)], axis=1).astype(np.uint8), c


def chain(inp, fwd_like, inter, variant, live=None):
    """orc_preprocess_backward of the named oracle build ("plain", "fma", "f64") on the intermediates.  Ordinary and RA_ASSOC rows go to that build; RA_LFORM rows
    go to "lform" (for "plain") or "f64_lform" (for "f64") -- the "fma" build has no l-form twin, its result holds the ordinary rows only (see `lform_refs`).
    fwd_like: "radii", "clamped" ((P,3) flags or (P,) bits), "cov3D", taken as given.  live: rows to evaluate (default: radius > 0)."""
    radii = np.asarray(fwd_like["radii"], np.int32).reshape(-1)
    if live is not None:
        radii = np.where(live, radii, 0).astype(np.int32)
    flags, _ = clamp_bits(fwd_like["clamped"])
    cls = inter["cls"]
    out = None
    for sel, name in ((cls != LFORM, variant), (cls == LFORM, {"plain": "lform", "f64": "f64_lform"}.get(variant))):
        if name is None or not (sel & (radii > 0)).any():
            continue
        with oracle.variant(name):
            r = oracle.preprocess_backward(inp, np.where(sel, radii, 0).astype(np.int32), flags, fwd_like["cov3D"],
                                           inter["dL_dmeans2D"], inter["chain_conic"], inter["dL_dcolors"])
        out = r if out is None else {k: out[k] + r[k] for k in r}          # (disjoint rows; the others are exact zeros)
    if out is None:
        P = radii.shape[0]; M = 0 if inp.get("shs") is None else int(np.asarray(inp["shs"]).shape[1])
        out = {"dL_dmeans3D": np.zeros((P, 3)), "dL_dcov3D": np.zeros((P, 6)), "dL_dsh": np.zeros((P, M, 3)), "dL_dscales": np.zeros((P, 3)),
               "dL_drotations": np.zeros((P, 4))}
    return out


def reference(inp, fwd_like, rows, rec, fmt):
    """Everything the tests compare against, for one set of rows: (inter, ref32s, ref64, live).  ref32s: the fp32 evaluations of the chain ("plain" and "fma";
    RA_LFORM rows are exact copies of the "lform" build in both, their single fp32 reference), ref64 the float64 build.  Both also carry "dL_dconic_lform":
    the rebuilt dL_dconic on RA_LFORM rows (zero elsewhere) from `cov2d` in the respective precision."""
    W, H = int(inp["W"]), int(inp["H"])
    live = live_rows(rows, fwd_like["radii"])
    cov_src = inp["cov3D_precomp"] if inp.get("cov3D_precomp") is not None else fwd_like["cov3D"]
    fl = dict(fwd_like); fl["cov3D"] = cov_src
    with np.errstate(all="ignore"):
        cov64 = cov2d(inp, cov_src, np.float64)
    inter = intermediates(rows, rec, W, H, fmt, cov=cov64)
    for k in SHORT_OUTPUTS + ("chain_conic",):
        inter[k][~live] = 0.0
    lf = (inter["cls"] == LFORM) & live
    r64 = chain(inp, fl, inter, "f64", live)
    plain = chain(inp, fl, inter, "plain", live); fma = chain(inp, fl, inter, "fma", live)
    for k in fma:          # the l-form rows' only fp32 reference is the "lform" build
        fma[k] = np.array(fma[k]); fma[k][lf] = plain[k][lf]
    u32 = EXP2_UNSCALE * EXP2_UNSCALE
    m32 = np.asarray(rows, np.float32)[:, 4:7] * u32
    c32 = lform_conic(m32, cov2d(inp, cov_src, np.float32)) if lf.any() else np.zeros((rows.shape[0], 4), np.float32)
    c32[~lf] = 0
    c64 = np.where(lf[:, None], inter["dL_dconic"], 0.0)
    plain["dL_dconic_lform"] = c32; fma["dL_dconic_lform"] = c32; r64["dL_dconic_lform"] = c64
    return inter, [plain, fma], r64, live


# ---- the verdicts ----------------------------------------------------------------------------------------------------------------------------------------
def _rows2d(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1).astype(np.float64)


def row_ratios(hip, ref32s, ref64, visible):
    """Per row of one array: (rows judged, r_hip, rho, rho_bar, zero-rule violations)."""
    h, t = _rows2d(hip), _rows2d(ref64)
    scale = np.abs(t).max(axis=1) if t.shape[1] else np.zeros(t.shape[0])
    judged = np.asarray(visible, bool) & (scale > 0)
    must_zero = scale == 0
    bad_zero = np.flatnonzero(must_zero & ((h != 0).any(axis=1) if h.shape[1] else False))
    idx = np.flatnonzero(judged)
    if idx.size == 0:
        return idx, np.zeros(0), np.zeros(0), 0.0, bad_zero
    with np.errstate(all="ignore"):
        r = np.abs(h[idx] - t[idx]).max(axis=1) / scale[idx]
        r = np.where(np.isfinite(r), r, np.inf)
        rho = np.max([np.abs(_rows2d(f)[idx] - t[idx]).max(axis=1) / scale[idx] for f in ref32s], axis=0)
    return idx, r, rho, float(np.median(rho)), bad_zero


def row_verdict(hip, ref32s, ref64, visible, k=K, names=None):
    """hip / ref32s[j] / ref64: dicts of (P, ...) arrays.  Returns the failing rows as (array, row, r_hip, rho_i, rho_bar) -- r_hip = inf for a row that had to be
    all zero and is not -- worst first, and the worst ratio r / max(rho_i, rho_bar) per array."""
    fails, worst = [], {}
    for name in (names if names is not None else [n for n in hip if n in ref64]):
        idx, r, rho, rho_bar, bad_zero = row_ratios(hip[name], [f[name] for f in ref32s], ref64[name], visible)
        fails += [(name, int(i), float("inf"), 0.0, rho_bar) for i in bad_zero]
        bar = k * np.maximum(rho, rho_bar)
        for j in np.flatnonzero(~(r <= bar)):
            fails.append((name, int(idx[j]), float(r[j]), float(rho[j]), rho_bar))
        with np.errstate(all="ignore"):
            q = r / np.maximum(rho, rho_bar)
        worst[name] = float(np.nanmax(np.where(r == 0, 0.0, q))) if idx.size else 0.0
    fails.sort(key=lambda f: -(f[2] / max(f[3], f[4], 1e-300)))
    return fails, worst


def array_verdict(hip, ref32, ref64, sel, names):
    """The whole-array arbiter on the rows `sel` alone (the RA_ASSOC class): per array, relative L2 of hip against the float64 build at most
    max(ARBITER_FLOOR, F64_K x that of the fp32 build `ref32`); rows that are all zero in float64 must be all zero.  Returns (failures as strings, {array: (e, floor)})."""
    fails, seen = [], {}
    for name in names:
        h, b, t = (_rows2d(x[name])[sel] for x in (hip, ref32, ref64))
        zero = ~np.abs(t).any(axis=1) if t.shape[1] else np.zeros(t.shape[0], bool)
        if h[zero].any():
            fails.append("%s: %d rows that must be all zero are not" % (name, int(h[zero].any(axis=1).sum())))
        nt = np.sqrt((t * t).sum())
        if nt == 0:
            continue
        e, floor = np.sqrt(((h - t) ** 2).sum()) / nt, np.sqrt(((b - t) ** 2).sum()) / nt
        seen[name] = (float(e), float(floor))
        if not e <= max(ARBITER_FLOOR, F64_K * floor):
            fails.append("%s relL2 vs float64 %.3e (oracle fp32 vs float64: %.3e)" % (name, e, floor))
    return fails, seen


def verdict_message(fails, k=K):
    return "%d rows miss r <= %g max(rho_i, rho_bar); worst: " % (len(fails), k) + "; ".join(
        "%s[%d] r %.3e rho_i %.3e rho_bar %.3e" % f for f in fails[:5])


def check_short(hip, inter, live):
    """The outputs one to three operations away from the row: bit-equal where the bound is 0 (copies, exact scalings, zeros), else within the derived bound
    of the float64 value.  Returns the failures as (array, row, column, hip, exact, bound)."""
    fails = []
    for name in SHORT_OUTPUTS:
        if hip.get(name) is None:
            continue
        h = _rows2d(hip[name]); t = inter[name]; bd = inter["bound"][name]
        if name == "dL_dconic":          # rebuilt values of RA_LFORM rows are held by row_verdict
            skip = (inter["cls"] == LFORM) & live
            t = np.where(skip[:, None], h, t)
        t32 = t.astype(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.where(bd == 0, h == t32, np.abs(h - t) <= bd)
        for i, c in zip(*np.nonzero(~ok)):
            fails.append((name, int(i), int(c), float(h[i, c]), float(t[i, c]), float(bd[i, c])))
    return fails


# ---- accumulators of the oracle's blend <-> rows ----------------------------------------------------------------------------------------------------------
def rows_from_accumulators(gb, rec, W, H):
    """The inverse of `intermediates` for ordinary rows: oracle.backward's per-Gaussian results (dL_dmeans2D, dL_dmeans2D_abs, dL_dconic, dL_dopacity, dL_dcolors,
    dL_dall_map) -> (P,16) float32 rows.  Columns 0-1 are a 2 x 2 solve per Gaussian with the conic, done in float64."""
    P = rec.shape[0]
    a, b, c, o = (np.asarray(rec[:, k], np.float32).astype(np.float64) for k in (4, 5, 6, 2))
    g2 = np.asarray(gb["dL_dmeans2D"], np.float64); ga = np.asarray(gb["dL_dmeans2D_abs"], np.float64); gc = np.asarray(gb["dL_dconic"], np.float64)
    rows = np.zeros((P, 16), np.float64)
    rx, ry = g2[:, 0] / (-0.5 * W), g2[:, 1] / (-0.5 * H)          # a Sx + b Sy,  b Sx + c Sy
    det = a * c - b * b
    with np.errstate(all="ignore"):
        rows[:, 0] = np.where(det != 0, (c * rx - b * ry) / det, 0.0); rows[:, 1] = np.where(det != 0, (a * ry - b * rx) / det, 0.0)
        rows[:, 7] = np.asarray(gb["dL_dopacity"], np.float64).reshape(-1) * o
    u = float(EXP2_UNSCALE)
    rows[:, 2] = ga[:, 0] / (0.5 * W) / u; rows[:, 3] = ga[:, 1] / (0.5 * H) / u
    rows[:, 4] = -2.0 * gc[:, 0]; rows[:, 5] = -2.0 * gc[:, 1]; rows[:, 6] = -2.0 * gc[:, 3]
    rows[:, 8:11] = np.asarray(gb["dL_dcolors"], np.float64)
    am = np.asarray(gb["dL_dall_map"], np.float64); rows[:, 11:14] = am[:, 0:3]; rows[:, 14] = am[:, 4]
    return np.where(np.isfinite(rows), rows, 0.0).astype(np.float32)


# ---- scenes and rows of the cases ---------------------------------------------------------------------------------------------------------------------------
SH_C0 = 0.28209479177387814


def fwd_like_of(ref):
    return {"radii": ref["radii"], "clamped": ref["clamped"], "cov3D": ref["cov3D"]}


def rec_of(ref):
    """(P,16) records with the two fields the stage reads: opacity (2) and conic (4..6)."""
    rec = np.zeros((ref["radii"].shape[0], 16), np.float32)
    rec[:, 2] = ref["conic_opacity"][:, 3]; rec[:, 4:7] = ref["conic_opacity"][:, :3]; rec[:, 0:2] = ref["means2D"]
    return rec


def with_all_map(inp):
    inp = dict(inp)
    inp["all_map"] = syn.plane_all_map(inp["means3D"], inp["scales"], inp["rotations"], inp["_cam"])
    inp["render_geo"] = True
    return inp


@functools.lru_cache(maxsize=None)
def _base(P, seed):
    inp = scene(P=P, W=208, H=144, deg=3, seed=seed, opacity="trained")
    cam = syn.make_camera(208, 144, radius=2.0)
    inp.update(tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"], _cam=cam)
    inp = with_all_map(inp)
    # (the classes below must be populated under both scale modifiers the tests use: a smaller modifier takes Gaussians off the screen)
    f0 = oracle.forward(inp, cull=True); f7 = oracle.forward(dict(inp, scale_modifier=0.7), cull=True)
    vis = np.flatnonzero((f0["radii"] > 0) & (f7["radii"] > 0)); tiled = (f0["tiles_touched"] > 0) & (f7["tiles_touched"] > 0)
    # every SH clamp mask 0..7 among the first 160 Gaussians: DC set so that a channel's colour is 0.5 (free) or -1.5 (clamped at 0) before the higher degrees' +-0.2.
    # Masks 1..7 cycle over the Gaussians with tiles first, so that none of them goes short; mask 0 is what hundreds of the others have anyway.
    shs = inp["shs"].copy()
    first = np.arange(min(160, P))
    order = np.concatenate([first[tiled[first]], first[~tiled[first]]])
    for n, i in enumerate(order):
        for ch in range(3):
            shs[i, 0, ch] = (-2.0 / SH_C0) if ((n % 7 + 1) >> ch) & 1 else 0.0
    inp["shs"] = shs
    # 20 visible Gaussians with opacity exactly 0: they keep their radius and take the `o > 0 ? ... : 0` guard
    op = inp["opacities"].copy()
    cand = vis[vis >= 160]
    zero_op = cand[:: max(1, cand.size // 20)][:20]
    op[zero_op] = 0.0
    inp["opacities"] = op
    inp["_zero_opacity"] = zero_op
    return inp


def base_scene(P=2000, seed=7, M=16, deg=3):
    """The base scene of the row tests (camera at radius 2: hundreds of Gaussians beyond the frustum clamps, ~30 % invisible), SH layout (M, deg)."""
    inp = dict(_base(P, seed))
    inp["shs"] = np.ascontiguousarray(inp["shs"][:, :M]); inp["sh_degree"] = deg
    return inp


@functools.lru_cache(maxsize=None)
def _needle():
    inp = scene(P=2000, W=208, H=144, deg=3, seed=31, opacity="trained", anisotropy="needle")
    return with_all_map(inp)


def needle_scene():
    return dict(_needle())


def subset(inp, idx):
    """The scene with Gaussians idx only (in that order)."""
    out = dict(inp)
    for k in ("means3D", "shs", "scales", "rotations", "opacities", "all_map", "colors_precomp", "cov3D_precomp"):
        if out.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(out[k])[idx])
    out.pop("_zero_opacity", None)
    return out


def end_scene(P):
    """P Gaussians of the 1000-Gaussian base scene, a Gaussian with tiles first (so that P = 1 computes something)."""
    big = base_scene(1000)
    f0 = oracle.forward(big, cull=True)
    lead = int(np.flatnonzero(f0["tiles_touched"] > 0)[0])
    idx = np.concatenate([[lead], np.delete(np.arange(1000), lead)])[:P]
    return subset(big, idx)


def seed_rows(P, group, radii, seed, n_zero=50, n_negzero=10):
    """(P,16) float32 rows: normals with COLUMN_SCALE in the group's columns, zeros elsewhere; n_zero visible rows all zero, n_negzero of them all -0.0;
    every invisible Gaussian gets a non-zero row.  Returns (rows, zero rows, -0.0 rows)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((P, 16), np.float32)
    cols = list(GROUPS[group])
    rows[:, cols] = (rng.normal(size=(P, len(cols))) * COLUMN_SCALE[cols]).astype(np.float32)
    vis = np.flatnonzero(np.asarray(radii).reshape(-1) > 0)
    n_zero = min(n_zero, vis.size // 4); n_negzero = min(n_negzero, n_zero // 2)
    zr = rng.choice(vis, size=n_zero, replace=False) if n_zero else np.zeros(0, np.int64)
    rows[zr] = 0.0
    rows[zr[:n_negzero]] = -0.0
    return rows, zr, zr[:n_negzero]


def class_counts(inp, ref):
    """Populations of the classes the row tests are about, on the oracle's forward."""
    m = np.asarray(inp["means3D"], np.float64); vm = np.asarray(inp["viewmatrix"], np.float64).reshape(-1)
    t = [vm[k] * m[:, 0] + vm[4 + k] * m[:, 1] + vm[8 + k] * m[:, 2] + vm[12 + k] for k in range(3)]
    vis = ref["radii"] > 0
    with np.errstate(all="ignore"):
        xc = np.abs(t[0] / t[2]) > 1.3 * float(inp["tanfovx"]); yc = np.abs(t[1] / t[2]) > 1.3 * float(inp["tanfovy"])
    _, bits = clamp_bits(ref["clamped"])
    return {"visible": int(vis.sum()), "invisible": int((~vis).sum()), "x_clamped": int((xc & vis).sum()), "y_clamped": int((yc & vis).sum()),
            "tiled": int((ref["tiles_touched"] > 0).sum()),
            "clamp_masks": [int(((bits == k) & (ref["tiles_touched"] > 0)).sum()) for k in range(8)],
            "near_singular": int((near_singular(rec_of(ref)) & vis).sum()),
            "zero_opacity": int(((ref["conic_opacity"][:, 3] == 0) & vis).sum())}


def precomp_scene(P=1000):
    """No SH and no scales: precomputed colours, and the forward's own cov3D as the precomputed covariance."""
    inp = base_scene(P)
    cov = oracle.forward(inp, cull=True)["cov3D"]
    alt = {k: v for k, v in inp.items() if k not in ("shs", "scales", "rotations")}
    alt["colors_precomp"] = np.random.default_rng(11).uniform(0, 1, (P, 3)).astype(np.float32)
    alt["cov3D_precomp"] = cov + 0
    alt["sh_degree"] = 0
    return alt


LAYOUTS = [(16, 3), (16, 2), (16, 0), (9, 2), (4, 1), (1, 0)]
END_SIZES = [1, 63, 64, 65, 127]


def seeded_cases():
    """Every seeded-row case of tests/test_gpu_bwd_rows.py as (id, scene factory, format of near-singular rows, column group, row seed)."""
    for mod in (1.0, 0.7):
        for n, group in enumerate(GROUPS):
            def mk(mod=mod):
                inp = base_scene(2000); inp["scale_modifier"] = mod
                return inp
            yield "chain-mod%g-%s" % (mod, group), mk, "lform", group, 100 + n
    for M, D in LAYOUTS:
        yield "layout-M%d-D%d" % (M, D), (lambda M=M, D=D: base_scene(1000, M=M, deg=D)), "lform", "all", 200 + M + D
    yield "precomp", precomp_scene, "lform", "all", 300
    for P in END_SIZES:
        for M, D in ((16, 3), (9, 2)):
            yield "ends-P%d-M%d" % (P, M), (lambda P=P, M=M, D=D: _with_layout(end_scene(P), M, D)), "lform", "all", 400 + P + M
    for fmt in ("lform", "assoc"):
        yield "needle-%s" % fmt, needle_scene, fmt, "all", 500


def _with_layout(inp, M, D):
    inp = dict(inp); inp["shs"] = np.ascontiguousarray(inp["shs"][:, :M]); inp["sh_degree"] = D
    return inp
