"""The oracle against the REFERENCE'S OWN CODE: the reference's forward.cu / backward.cu / rasterizer_impl.cu compiled for the CPU
(oracle/ref_cpu, oracle/reference.py) and run on the cases of tests/reference_cases.py.  CPU only.

What is asserted, per case:
* integer state and decisions -- radii, tiles_touched, clamped, the sorted keys and values, ranges, num_rendered, n_contrib, the median contributors,
  valid_src_indices, use_first_src_frame_mask, markVisible -- EXACT between the plain builds (oracle.forward(cull=False) follows the reference's lists);
* every float outside an atomic sum -- FORWARD::preprocess, FORWARD::render fed the reference's own lists and state, BACKWARD::preprocess fed given
  gradients -- BIT-IDENTICAL between the plain builds (both float32, no contraction, one libm).  The fma twins are not bit-identical to each other: where the
  compiler contracts is its choice in a C and in a C++/glm translation unit alike, an evaluation-order freedom.  Each stage of the oracle's fma build -- the
  three above, each on inputs identical for all runs -- must lie within the distance between the reference's OWN plain and fma builds on that array (relative L2,
  factor 1); decisions taken on those floats may differ on at most as many elements as the reference's two builds differ from each other, plus one;
* the float-atomicAdd sums of BACKWARD::render and the ten gradients of the whole backward: the yardstick is d_order, the relative-L2 distance between two runs of
  the reference with the blocks visited first-to-last and last-to-first.  The oracle (plain: double sums; acc32: float sums in pixel order) must lie within
  min(2 d_order, 1e-3) of the first-to-last run; where d_order is 0 (every Gaussian touched from one block) within 2^-22 of the array's largest magnitude.  On the
  needle scene the float64 build arbitrates: the oracle may also pass by being no further from float64 than 2 x the reference is.
Every figure is printed before it is asserted (pytest -s).

Two needle cases.  "needles" is the needle scene of tests/fuzz_cases.py (pinned case 9103 / 117 of the trained sweep at this file's frame): the reference reproduces its own
gradients to 1e-4 ... 6e-3 there, and every test applies.  "needles_singular" (giant_needles, stretch 8, thin 0.02) is the one scene that takes the `power > 0` skip (8 064 pairs);
its conics are within rounding of singular, and behind the atomic sums the reference's own two block orders differ by 0.4 ... 0.7 RELATIVE in dL_dmeans3D, dL_dscales and
dL_drotations, so the ten-gradient test leaves it out (see WHOLE_NAMES) and every other test keeps it.  Wherever one Gaussian carries an array's distance (largest single-row
share of d_order^2: 0.48 ... 0.96 in every case) the ratio of two single draws is heavy-tailed: with other upstream-gradient seeds single arrays measured 2.1 ... 3.4
(geo5_L8 dL_dscales, geo3_L3_quant dL_dscales, geo1_L4 dL_dcov3D; on geo5_L8 every float32 evaluation 1.0e-05 from float64); the seeds are written out in UPSTREAM_SEEDS.  DESIGN.md section 5 has the table."""
import functools

import numpy as np
import pytest

import oracle
from oracle import reference as ref
from tests import reference_cases as rc
from tests import scenes
from tests.metrics import rel_l2

pytestmark = pytest.mark.skipif(not ref.available(), reason=ref.why_unavailable())

F64_K = 2.0
INT_STATE = ("radii", "tiles_touched", "clamped", "keys", "point_list", "ranges", "n_contrib", "cache_low", "cache_high", "use_first_src_frame_mask")
PRE_FLOATS = ("means2D", "depths", "cov3D", "rgb", "conic_opacity")
RENDER_FLOATS = ("color", "normal_map", "median_depth", "cam_feat", "warped_image", "min_depth_diff", "camera_ray", "final_T", "cache_sum_w", "valid_src_w")
RENDER_INTS = ("n_contrib", "cache_low", "cache_high", "use_first_src_frame_mask")
ATOMIC = ("dL_dmeans2D", "dL_dmeans2D_abs", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dall_map")
PRE_BWD = ("dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
TEN = ("dL_dmeans3D", "dL_dmeans2D", "dL_dmeans2D_abs", "dL_dcolors", "dL_dall_map", "dL_dopacity", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def _inside():
    return scenes.inside_cloud(2500, rc.W, rc.H, (0.2, -0.3, 0.1), (0.9, 0.6, 0.0), 1.2, 0.9, seed=17, deg=2, opacity="trained", scale_mul=0.6)


def _depth_only():
    inp = scenes.scene(P=1500, W=rc.W, H=rc.H, deg=1, seed=41, opacity="trained", planes=True, scale_mul=2.0)
    inp["render_depth_only"] = True
    return inp


def _sh2_mod():
    inp = rc.color_case(2, 13)
    inp = rc.with_camera(inp, scenes.camera_at(rc.W, rc.H, (0.5, -3.8, 1.2), (0.0, 0.0, 0.0), 0.8, 0.45))
    inp["scale_modifier"] = 0.7
    return inp


def _alpha_floor():
    """sh1's cloud plus three Gaussians in front of everything whose centres project EXACTLY onto pixel centres and whose opacity is exactly 1/255 in float32:
    at those pixels power = 0, alpha = opacity and the skip test `alpha < 1/255` is taken on equality (the pair blends)."""
    inp = rc.color_case(1, 14, P=300)
    cam = np.asarray(inp["campos"], np.float64)
    fwd = -cam / np.linalg.norm(cam)

    def pixels(points):
        one = dict(inp)
        n = len(points)
        one.update(means3D=np.asarray(points, np.float32), scales=np.full((n, 3), 0.02, np.float32), rotations=np.tile(np.float32([1, 0, 0, 0]), (n, 1)),
                   opacities=np.full((n, 1), 0.5, np.float32), shs=np.zeros((n, 16, 3), np.float32))
        return oracle.forward(one)["means2D"].astype(np.float64), one["means3D"]

    placed, at = [], []
    for kx, ky, depth in ((20, 17, 1.0), (41, 30, 1.1), (55, 9, 1.2), (50, 40, 1.2), (30, 44, 1.3), (12, 25, 1.4), (60, 21, 1.5), (37, 12, 1.6)):
        if len(placed) == 3:
            break
        p = cam + depth * fwd
        for _ in range(4):          # Newton on the projection, finite differences
            m, _ = pixels([p, p + [1e-3, 0, 0], p + [0, 1e-3, 0], p + [0, 0, 1e-3]])
            J = ((m[1:] - m[0]) / 1e-3).T
            p = p + np.linalg.lstsq(J, np.float64([kx, ky]) - m[0], rcond=None)[0]
        p32 = p.astype(np.float32)
        steps = np.arange(-12, 13)
        grid = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), -1).reshape(-1, 3)
        cand = np.stack([p32 + np.float32(np.spacing(np.abs(p32))) * g.astype(np.float32) for g in grid]).astype(np.float32)
        m, c32 = pixels(cand)
        hit = np.flatnonzero((m[:, 0] == kx) & (m[:, 1] == ky))
        if hit.size:          # (the float32 points around a pixel centre need not contain one that projects onto it exactly in both coordinates)
            placed.append(c32[hit[0]]); at.append((kx, ky))
    n = len(placed)
    assert n == 3, "fewer than three float32 points found that project exactly onto a pixel centre"
    inp["means3D"] = np.concatenate([np.asarray(placed, np.float32), inp["means3D"]]).astype(np.float32)
    inp["scales"] = np.concatenate([np.full((n, 3), 0.02, np.float32), inp["scales"]])
    inp["rotations"] = np.concatenate([np.tile(np.float32([1, 0, 0, 0]), (n, 1)), inp["rotations"]])
    inp["opacities"] = np.concatenate([np.full((n, 1), np.float32(1.0) / np.float32(255.0), np.float32), inp["opacities"].reshape(-1, 1)])
    inp["shs"] = np.concatenate([np.full((n, 16, 3), 0.8, np.float32), inp["shs"]])
    inp["_placed"] = tuple(at)
    return inp


def _fuzz_needles():
    """The needle scene of tests/fuzz_cases.py: the pinned case (9103, 117) of the trained sweep -- 9 000 Gaussians, anisotropy "needle", scale sigma 1, scales x 15,
    SH degree 3 -- with every drawn parameter kept and the frame reduced from 801 x 510 to this file's 72 x 56."""
    from tests import fuzz_cases as fc
    c = fc.draw_parity(fc._pinned_rng(9103, 117, "trained"), "trained")
    assert c["sseed"] == 733679, "tests/golden/fuzz_pins.json no longer pins the case"
    c["W"], c["H"] = rc.W, rc.H
    inp = fc.build_parity(c)
    assert c["knobs"].startswith("anisotropy needle")
    return inp


NEEDLES = ("needles", "needles_singular")          # the cases whose ill-conditioned arrays the float64 build arbitrates

# name -> (builder, tex_quant)
CASES = {
    "alpha_exactly_1_255": (_alpha_floor, False),
    "sh0_black": (lambda: rc.color_case(0, 11), False),
    "sh1_bg": (lambda: rc.color_case(1, 12, bg=(0.2, 0.5, 1.0)), False),
    "sh2_mod0.7_fx_ne_fy": (_sh2_mod, False),
    "sh3_white_two_rounds": (rc.FIXTURES["sh3_white"]["build"], False),
    "precomp": (rc.precomp_case, False),
    "inside_camera": (_inside, False),
    "depth_only": (_depth_only, False),
    "needles": (_fuzz_needles, False),
    "needles_singular": (lambda: scenes.giant_needles(P=300, W=rc.W, H=rc.H, seed=6, stretch=8.0, thin=0.02), False),
    "geo1_L4": (lambda: rc.geo_case(1, 4, 5), False),
    "geo3_L3_quant": (lambda: rc.geo_case(3, 3, 6), True),
    "geo3_L4_thr_rejects": (lambda: rc.geo_case(3, 4, 7, depth_thr=0.0015), False),
    "geo5_L8": (lambda: rc.geo_case(5, 8, 8), False),
    "geo5_L3_close_quant": (rc.FIXTURES["geo5_L3_close"]["build"], True),
}
NAMES = tuple(CASES)
# seeds of the upstream gradients, one per case, written out (they once were crc32 of the case name: a renamed case keeps its draw)
UPSTREAM_SEEDS = {
    "alpha_exactly_1_255": 3516499480,
    "sh0_black": 909443829,
    "sh1_bg": 1046276567,
    "sh2_mod0.7_fx_ne_fy": 1962674690,
    "sh3_white_two_rounds": 2293743129,
    "precomp": 2356341636,
    "inside_camera": 3414465253,
    "depth_only": 108811358,
    "needles": 1795253094,
    "needles_singular": 73876348,
    "geo1_L4": 3257520533,
    "geo3_L3_quant": 1178029435,
    "geo3_L4_thr_rejects": 1202476581,
    "geo5_L8": 1157434089,
    "geo5_L3_close_quant": 2034390533,
}


def _terminated(v):
    """valid_src_indices with every slot after the first -1 set to -1: the reference defines the slots only up to its terminator (forward.cu:648-655)."""
    v = np.asarray(v).reshape(5, -1).copy()
    dead = np.cumsum(v == -1, axis=0) > 0
    v[dead] = -1
    return v


def _shape_like(a, b):
    return np.asarray(a).reshape(np.asarray(b).shape)


@functools.lru_cache(maxsize=None)
def run(name):
    """Everything both sides compute for one case, once (the tests below only read it)."""
    build, q = CASES[name]
    inp = build()
    g = rc.upstream(inp, UPSTREAM_SEEDS[name]); ga = rc.grad_args(g)
    depth_only = bool(inp.get("render_depth_only"))
    r = {"inp": inp, "g": g, "q": q}
    for b, fma in (("plain", False), ("fma", True)):
        with oracle.variant(b):
            fo = oracle.forward(inp, tex_quant=q, cull=False)
        fr = ref.forward(inp, tex_quant=q, fma=fma)
        with oracle.variant(b):
            so = oracle.render_forward(inp, fr, tex_quant=q)          # the oracle's blend stage on the reference's lists and state
        r[b] = {"fo": fo, "fr": fr, "so": so}
    # the reference's PLAIN blend stage on the fma build's lists and state: with r["fma"]["fr"] (the fma build on the same state) the reference's own pair on identical inputs
    r["fma"]["rp_stage"] = ref.stage_render_forward(inp, r["fma"]["fr"], tex_quant=q, fma=False)
    if not depth_only:
        fr = r["plain"]["fr"]
        r["plain"]["bo_stage"] = oracle.render_backward(inp, fr, *ga, tex_quant=q)
        gs = r["plain"]["br_stage"] = ref.stage_render_backward(inp, fr, *ga, tex_quant=q)
        # BACKWARD::preprocess of all four builds on ONE set of inputs: the plain reference's state and the plain reference's atomic sums
        cov = inp["cov3D_precomp"] if inp.get("cov3D_precomp") is not None else fr["cov3D"]
        for b, fma in (("plain", False), ("fma", True)):
            with oracle.variant(b):
                r[b]["po"] = oracle.preprocess_backward(inp, fr["radii"], fr["clamped"], cov, gs["dL_dmeans2D"], gs["dL_dconic"], gs["dL_dcolors"])
            r[b]["pr"] = ref.preprocess_backward(inp, fr["radii"], fr["clamped"], cov, gs["dL_dmeans2D"], gs["dL_dconic"], gs["dL_dcolors"], fma=fma)
        r["br_stage_rev"] = ref.stage_render_backward(inp, fr, *ga, tex_quant=q, reverse_blocks=True)
        with oracle.variant("acc32"):
            r["bo_stage_acc32"] = oracle.render_backward(inp, fr, *ga, tex_quant=q)
            r["bo_acc32"] = oracle.backward(inp, oracle.forward(inp, tex_quant=q, cull=False), *ga, tex_quant=q)
        r["bo"] = oracle.backward(inp, r["plain"]["fo"], *ga, tex_quant=q)
        r["br"] = ref.backward(inp, fr, *ga, tex_quant=q)
        r["br_rev"] = ref.backward(inp, fr, *ga, tex_quant=q, reverse_blocks=True)
    return r


def _int_mismatches(a, b, keys):
    n = {}
    for k in keys:
        x, y = np.asarray(a[k]), _shape_like(b[k], a[k])
        n[k] = int((x != y).sum()) if x.shape == y.shape else max(x.size, y.size)
    x, y = _terminated(a["valid_src_idx"]), _terminated(b["valid_src_idx"])
    n["valid_src_idx"] = int((x != y).any(axis=0).sum())
    return n


@pytest.mark.parametrize("name", NAMES)
def test_integer_state_and_decisions_match_exactly(name):
    r = run(name); fo, fr = r["plain"]["fo"], r["plain"]["fr"]
    assert int(fo["num_rendered"]) == int(fr["num_rendered"]), (fo["num_rendered"], fr["num_rendered"])
    n = _int_mismatches(fo, fr, INT_STATE)
    print(name, "num_rendered", fr["num_rendered"], "mismatching elements", n)
    assert not any(n.values()), n
    inp = r["inp"]
    assert np.array_equal(oracle.mark_visible(inp["means3D"], inp["viewmatrix"]), ref.mark_visible(inp["means3D"], inp["viewmatrix"], inp["projmatrix"]))


@pytest.mark.parametrize("name", NAMES)
def test_plain_builds_are_bit_identical_stage_by_stage(name):
    r = run(name)["plain"]; fo, fr, so = r["fo"], r["fr"], r["so"]
    vis = fr["radii"] > 0          # the reference leaves the state of culled Gaussians unwritten
    bad = [k for k in PRE_FLOATS if not np.array_equal(np.asarray(fo[k])[vis], _shape_like(fr[k], fo[k])[vis])]
    bad += ["render:" + k for k in RENDER_FLOATS + RENDER_INTS if not np.array_equal(np.asarray(so[k]), _shape_like(fr[k], so[k]))]
    if not np.array_equal(_terminated(so["valid_src_idx"]), _terminated(fr["valid_src_idx"])):
        bad.append("render:valid_src_idx")
    if "po" in r:
        bad += ["bwd:" + k for k in PRE_BWD if not np.array_equal(np.asarray(r["po"][k]), _shape_like(r["pr"][k], r["po"][k]))]
    print(name, "arrays that are not bit-identical:", bad)
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_fma_builds_stay_within_the_references_own_contraction_distance(name):
    """Contraction is the compiler's choice in both translation units (module docstring).  Every stage is judged on IDENTICAL inputs for three runs: the oracle's fma
    build, the reference's fma build and the reference's plain build -- FORWARD::preprocess on the case's inputs, FORWARD::render on the reference's fma lists and state,
    BACKWARD::preprocess on the plain reference's state and atomic sums.  Per array the oracle's fma build may be no further from the reference's fma build than the
    reference's own plain build is (relative L2; factor 1); decisions may flip on at most as many elements as between the reference's own two builds, plus one."""
    R = run(name); p, f = R["plain"], R["fma"]
    hw = int(R["inp"]["W"]) * int(R["inp"]["H"])
    own = _int_mismatches(f["rp_stage"], f["fr"], RENDER_INTS)
    got = _int_mismatches(f["so"], f["fr"], RENDER_INTS)
    print(name, "render decision flips on the fma lists: oracle fma vs reference fma", got, "| reference plain vs reference fma", own)
    for k in got:
        assert own[k] < 0.001 * hw, (k, own[k])          # every case keeps the reference's own flips under 0.1 % of the pixels, so the cap below is tight
        assert got[k] <= own[k] + 1, (k, got[k], own[k])
    pre_n = {k: int((np.asarray(f["fo"][k]) != _shape_like(f["fr"][k], f["fo"][k])).sum()) for k in ("radii", "tiles_touched", "clamped")}
    pre_own = {k: int((np.asarray(p["fr"][k]) != np.asarray(f["fr"][k])).sum()) for k in pre_n}
    print(name, "preprocess decisions: oracle fma vs reference fma", pre_n, "| reference plain vs fma", pre_own)
    for k in pre_n:
        assert pre_n[k] <= pre_own[k] + 1, (k, pre_n[k], pre_own[k])
    same_vis = (f["fo"]["radii"] > 0) & (f["fr"]["radii"] > 0) & (p["fr"]["radii"] > 0)
    same_px = np.ones(hw, bool)
    for k in RENDER_INTS:          # floats are compared where all three runs took the same decisions
        same_px &= (np.asarray(f["so"][k]).reshape(-1) == np.asarray(f["fr"][k]).reshape(-1)) & (np.asarray(f["rp_stage"][k]).reshape(-1) == np.asarray(f["fr"][k]).reshape(-1))
    same_px &= (_terminated(f["so"]["valid_src_idx"]) == _terminated(f["fr"]["valid_src_idx"])).all(axis=0) & (_terminated(f["rp_stage"]["valid_src_idx"]) == _terminated(f["fr"]["valid_src_idx"])).all(axis=0)
    fails = []

    def judge(tag, a_orc, a_ref_fma, a_ref_plain):
        d_own, d = rel_l2(a_ref_plain, a_ref_fma), rel_l2(a_orc, a_ref_fma)
        print("  %-28s oracle-fma vs reference-fma %.3e   reference plain vs fma %.3e" % (tag, d, d_own))
        if not d <= d_own:
            fails.append((tag, d, d_own))
    for k in PRE_FLOATS:
        judge(k, np.asarray(f["fo"][k])[same_vis], _shape_like(f["fr"][k], f["fo"][k])[same_vis], _shape_like(p["fr"][k], f["fo"][k])[same_vis])
    sel = lambda a: np.asarray(a).reshape(-1, hw)[:, same_px]
    for k in RENDER_FLOATS:
        if np.abs(sel(f["fr"][k])).sum() == 0:
            continue
        judge("render:" + k, sel(f["so"][k]), sel(f["fr"][k]), sel(f["rp_stage"][k]))
    if "po" in f:
        for k in PRE_BWD:
            a = np.asarray(f["pr"][k])
            if a.size == 0 or not np.abs(a).any():
                assert not np.abs(np.asarray(f["po"][k])).any(), k
                continue
            judge("bwd:" + k, _shape_like(f["po"][k], a), a, _shape_like(p["pr"][k], a))
    assert not fails, fails


def _order_rule(tag, orc, r_fwd, r_rev, arbiter=None):
    """(ok, text): `orc` against the reference's first-to-last run by the d_order rule of the module docstring; arbiter = (oracle f64 array) adds the two-grain pass."""
    orc, r_fwd, r_rev = np.asarray(orc, np.float64), np.asarray(r_fwd, np.float64).reshape(np.asarray(orc).shape), np.asarray(r_rev, np.float64).reshape(np.asarray(orc).shape)
    top = np.abs(r_fwd).max() if r_fwd.size else 0.0
    if top == 0.0:
        ok = not np.abs(orc).any()
        return ok, "%-18s all zero in the reference; oracle all zero: %s" % (tag, ok)
    d_order, d = rel_l2(r_rev, r_fwd), rel_l2(orc, r_fwd)
    if d_order == 0.0:
        e = np.abs(orc - r_fwd).max() / top
        ok, text = e <= 2.0 ** -22, "%-18s d_order 0: max|oracle - reference| / max|reference| = %.3e (bar 2^-22 = %.3e)" % (tag, e, 2.0 ** -22)
    else:
        bar = min(F64_K * d_order, 1e-3)
        ok, text = d <= bar, "%-18s d_order %.3e  oracle vs reference %.3e  ratio %.2f (bar %.1f, and 1e-3 at most)" % (tag, d_order, d, d / d_order, F64_K)
    if not ok and arbiter is not None:
        a = np.asarray(arbiter, np.float64).reshape(orc.shape)
        e_o, e_r = rel_l2(orc, a), rel_l2(r_fwd, a)
        ok = e_o <= F64_K * e_r
        text += "  | float64 arbiter: oracle %.3e, reference %.3e, ratio %.2f" % (e_o, e_r, e_o / max(e_r, 1e-300))
    return ok, text


def _arbiter(name, r, stage, diagnostic=False):
    if name not in NEEDLES and not diagnostic:
        return None
    inp, ga, q = r["inp"], rc.grad_args(r["g"]), r["q"]
    with oracle.variant("f64"):
        f64 = oracle.forward(inp, tex_quant=q, cull=False)
        return oracle.render_backward(inp, f64, *ga, tex_quant=q) if stage else oracle.backward(inp, f64, *ga, tex_quant=q)


BWD_NAMES = tuple(n for n in NAMES if n != "depth_only")


@pytest.mark.parametrize("name", BWD_NAMES)
def test_atomic_sums_of_the_backward_blend_within_the_references_order_scatter(name):
    r = run(name); arb = _arbiter(name, r, True)
    fails = []
    for build, key in (("plain", "bo_stage"), ("acc32", "bo_stage_acc32")):
        bo = r["plain"][key] if build == "plain" else r[key]
        for k in ATOMIC:
            ok, text = _order_rule(k, bo[k], r["plain"]["br_stage"][k], r["br_stage_rev"][k], None if arb is None else arb[k])
            print(name, build, text)
            if not ok:
                fails.append((build, text))
    assert not fails, fails


# needles_singular is judged up to the atomic sums only: behind them its per-Gaussian chain turns the last bit of dL_dconic into the whole result -- the reference's OWN two
# block orders differ by tens of per cent in dL_dmeans3D, dL_dscales and dL_drotations there (asserted in test_the_cases_have_the_properties_they_are_named_for), so neither
# d_order nor the float64 build measures anything on those arrays: with one seed of the upstream gradients the oracle's ratio was 2.10, with the next 0.6.  The chain itself
# is held bit-identical on that case by test_plain_builds_are_bit_identical_stage_by_stage, and "needles" (tests/fuzz_cases.py's scene) carries the ten-gradient check.
WHOLE_NAMES = tuple(n for n in BWD_NAMES if n != "needles_singular")


@pytest.mark.parametrize("name", WHOLE_NAMES)
def test_whole_backward_all_ten_gradients_within_the_references_order_scatter(name):
    r = run(name); arb = _arbiter(name, r, False)
    fails = []
    for build, bo in (("plain", r["bo"]), ("acc32", r["bo_acc32"])):
        for k in TEN:
            ok, text = _order_rule(k, bo[k], r["br"][k], r["br_rev"][k], None if arb is None else arb[k])
            if not ok and arb is None:          # not a pass: how far both sides are from float64, for the reader of the failure
                a64 = np.asarray(_arbiter(name, r, False, diagnostic=True)[k], np.float64).reshape(np.asarray(bo[k]).shape)
                text += "  | for information, vs float64: oracle %.3e, reference %.3e" % (rel_l2(bo[k], a64), rel_l2(_shape_like(r["br"][k], bo[k]), a64))
            print(name, build, text)
            if not ok:
                fails.append((build, text))
    assert not fails, fails


def test_the_cases_have_the_properties_they_are_named_for():
    two = run("sh3_white_two_rounds")["plain"]["fr"]
    lens = (two["ranges"][:, 1].astype(np.int64) - two["ranges"][:, 0]).reshape(-1)
    assert lens.max() > 256, "no tile list takes two fetch rounds"
    gx = (rc.W + 15) // 16
    tile_of = (np.arange(rc.H)[:, None] // 16) * gx + np.arange(rc.W)[None, :] // 16
    sat = (two["n_contrib"].reshape(rc.H, rc.W) < lens[tile_of]) & (two["final_T"].reshape(rc.H, rc.W) < 0.01)
    assert sat.any(), "no pixel saturates before its list ends"
    assert rc.W % 16 and rc.H % 16
    rej = run("geo3_L4_thr_rejects")["plain"]["fr"]
    nvalid = (_terminated(rej["valid_src_idx"]) >= 0).sum(axis=0)[rej["final_T"] < 0.5]
    assert (nvalid < 3).any() and (nvalid > 0).any(), "depth_thr rejects no source, or every one"
    ins = run("inside_camera")["plain"]["fr"]
    assert (ins["radii"] == 0).mean() > 0.3 and ins["radii"].max() > max(rc.W, rc.H)
    nd = run("needles_singular")
    oracle.forward(nd["inp"], cull=False)
    assert oracle.power_skips()[0] > 0, "the needle scene never takes the power > 0 skip"
    for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations"):          # why that case is left out of WHOLE_NAMES: the reference does not reproduce itself there
        assert rel_l2(nd["br_rev"][k], nd["br"][k]) > 0.1, k
    fz = run("needles")
    assert max(rel_l2(fz["br_rev"][k], fz["br"][k]) for k in TEN) < 0.05, "the fuzz needle scene's gradients are not reproducible by the reference itself"
    af = run("alpha_exactly_1_255"); fa = af["plain"]["fr"]
    for i, (kx, ky) in enumerate(af["inp"]["_placed"]):
        assert tuple(fa["means2D"][i]) == (kx, ky) and fa["conic_opacity"][i, 3] == np.float32(1.0) / np.float32(255.0)
        assert fa["point_list"][fa["ranges"][(ky // 16) * ((rc.W + 15) // 16) + kx // 16, 0]] < 3, "a placed Gaussian is not the front of its tile's list"
    for n in ("geo1_L4", "geo3_L3_quant", "geo5_L8", "geo5_L3_close_quant"):
        f = run(n)["plain"]["fr"]
        assert (_terminated(f["valid_src_idx"])[0] >= 0).mean() > 0.2, n
    q = run("geo3_L3_quant")["inp"]
    assert not np.array_equal(ref.forward(q, tex_quant=True)["warped_image"], ref.forward(q, tex_quant=False)["warped_image"])


def test_no_gaussians():
    inp = rc.color_case(1, 3, P=4)
    for k in ("means3D", "shs", "scales", "rotations", "opacities"):
        inp[k] = inp[k][:0]
    fo, fr = oracle.forward(inp), ref.forward(inp)
    assert fo["num_rendered"] == fr["num_rendered"] == 0
    for k in ("color", "final_T", "n_contrib", "ranges", "radii"):
        assert np.array_equal(fo[k], fr[k]), k
    g = np.ones((3, rc.H, rc.W), np.float32)
    bo, br = oracle.backward(inp, fo, g), ref.backward(inp, fr, g)
    for k in TEN:
        assert np.asarray(bo[k]).shape == np.asarray(br[k]).shape and not np.asarray(br[k]).size, k
    assert ref.mark_visible(inp["means3D"].reshape(0, 3), inp["viewmatrix"], inp["projmatrix"]).shape == (0,)
