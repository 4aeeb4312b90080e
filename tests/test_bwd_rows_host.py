"""tests/bwd_rows.py on the CPU: the restatement of the per-Gaussian backward's row contract against the oracle's own backward, the measurement behind the
row bar K kept as a test, and the verdict's own behaviour.  No GPU."""
import numpy as np
import pytest

import oracle
from tests import bwd_rows as br


def rnd(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def ulps(a, b):
    """|a - b| in units of the float32 spacing at max(|a|, |b|)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


@pytest.fixture(scope="module")
def base():
    inp = br.base_scene(2000)
    ref = oracle.forward(inp, cull=True)
    H, W = inp["H"], inp["W"]
    gb = oracle.backward(inp, ref, rnd((3, H, W), 1), rnd((3, H, W), 2))
    return inp, ref, gb


def blend_rows(inp, seed=1):
    ref = oracle.forward(inp, cull=True)
    H, W = inp["H"], inp["W"]
    gb = oracle.backward(inp, ref, rnd((3, H, W), seed), rnd((3, H, W), seed + 1))
    return ref, br.rows_from_accumulators(gb, br.rec_of(ref), W, H)


def test_classes_of_the_scenes_are_populated(base):
    inp, ref, _ = base
    c = br.class_counts(inp, ref)
    assert c["x_clamped"] >= 100 and c["y_clamped"] >= 100 and c["invisible"] >= 100, c
    assert min(c["clamp_masks"]) >= 10 and c["zero_opacity"] == 20, c
    small = br.base_scene(1000)
    c = br.class_counts(small, oracle.forward(small, cull=True))
    assert c["x_clamped"] >= 50 and c["y_clamped"] >= 50 and c["invisible"] >= 100 and min(c["clamp_masks"]) >= 10 and c["zero_opacity"] == 20, c
    nd = br.needle_scene()
    c = br.class_counts(nd, oracle.forward(nd, cull=True))
    assert c["near_singular"] >= 100, c
    for P in br.END_SIZES:
        e = br.end_scene(P)
        assert oracle.forward(e, cull=True)["tiles_touched"][0] > 0


def test_restatement_reproduces_the_oracles_backward(base):
    """Rows built from oracle.backward's own accumulators (the inverse of the row contract), through `intermediates` and the plain chain: every output of
    oracle.backward again, bit for bit -- dL_dmean2D, which passes through a 2 x 2 solve with the conic in float64 and a float32 row, within 4 ulp (of the larger of
    its two terms: the row holds the solve's result to half an ulp each, and the terms may cancel); the chain then takes the oracle's own value of it.
    Two more outputs are held to 4 ulp instead of bit for bit, for the same reason: dL_dmean2D_abs and dL_dopacity.  Their row columns are the oracle's values
    divided by the exp2 unscale and multiplied by the opacity, rounded to float32, and that does not round-trip through the contract's multiplication / division."""
    inp, ref, gb = base
    W, H = inp["W"], inp["H"]
    rec = br.rec_of(ref)
    rows = br.rows_from_accumulators(gb, rec, W, H)
    vis = ref["radii"] > 0
    touched = (rows != 0).any(axis=1)
    assert touched.sum() > 300 and not touched[~vis].any()
    inter = br.intermediates(rows, rec, W, H, "ordinary")
    assert (inter["cls"] == br.ORDINARY).all()
    live = br.live_rows(rows, ref["radii"])
    for name in ("dL_dconic", "dL_dcolors", "dL_dall_map"):
        assert np.array_equal(inter[name].astype(np.float32)[live], gb[name][live]), name
    a, b, c = (rec[:, k].astype(np.float64) for k in (4, 5, 6))
    big = np.stack([0.5 * W * np.maximum(np.abs(a * rows[:, 0]), np.abs(b * rows[:, 1])), 0.5 * H * np.maximum(np.abs(c * rows[:, 1]), np.abs(b * rows[:, 0]))], axis=1)
    err = np.abs(inter["dL_dmeans2D"][:, :2] - gb["dL_dmeans2D"][:, :2]) / np.spacing(np.maximum(big, np.abs(gb["dL_dmeans2D"][:, :2])).astype(np.float32))
    assert err[live].max() <= 4.0, err[live].max()
    assert ulps(inter["dL_dmeans2D_abs"][live], gb["dL_dmeans2D_abs"][live]).max() <= 4.0
    zo = rec[:, 2] > 0
    assert ulps(inter["dL_dopacity"][live & zo], gb["dL_dopacity"][live & zo]).max() <= 4.0
    inter["dL_dmeans2D"][:] = gb["dL_dmeans2D"]
    out = br.chain(inp, br.fwd_like_of(ref), inter, "plain")          # (every visible Gaussian, like oracle.backward)
    for name in br.CHAIN_OUTPUTS:
        assert np.array_equal(out[name].view(np.uint32), gb[name].view(np.uint32)), name


def _all_inputs():
    for cid, mk, fmt, group, seed in br.seeded_cases():
        inp = mk()
        ref = oracle.forward(inp, cull=True)
        rows, _, _ = br.seed_rows(ref["radii"].shape[0], group, ref["radii"], seed)
        yield cid, inp, ref, rows, fmt
    # the blend's own rows (section 3 of the GPU tests runs with default flags: near-singular conics are RA_LFORM rows there, which have no fp32 twin and
    # are left out below; the oracle's accumulators of those Gaussians are not in that format anyway)
    for tag, inp in (("blend-base", br.base_scene(2000)), ("blend-needle", br.needle_scene())):
        ref, rows = blend_rows(inp)
        yield tag, inp, ref, rows, "lform"


def test_fp32_builds_meet_each_others_row_bar():
    """THE MEASUREMENT BEHIND K: the fma build judged by the row bar with the plain build as its only reference, and the other way round, on the stage alone with
    identical rows, over every seeded case and the blend's own rows of both scenes, on the classes that are held row by row.  Both pass at K, and K is at
    least twice the worst ratio seen."""
    worst, per_case = {}, {}
    for cid, inp, ref, rows, fmt in _all_inputs():
        inter, (plain, fma), r64, live = br.reference(inp, br.fwd_like_of(ref), rows, br.rec_of(ref), fmt)
        # per format class, as the GPU tests judge (l-form rows have one fp32 reference and are left out)
        for cls, tag in ((br.ORDINARY, cid), (br.ASSOC, cid + "/RA_ASSOC")):
            sel = live & (inter["cls"] == cls)
            if not sel.any():
                continue
            for judged, only in ((fma, plain), (plain, fma)):
                fails, w = br.row_verdict(judged, [only], r64, sel, names=br.CHAIN_OUTPUTS)
                assert not fails, tag + ": " + br.verdict_message(fails)
                for k, v in w.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                    per_case.setdefault(tag, {})[k] = max(per_case.get(tag, {}).get(k, 0.0), v)
            if cls == br.ASSOC:          # the class also meets the whole-array arbiter rule it is held to in addition
                fails, _ = br.array_verdict(fma, plain, r64, sel, br.CHAIN_OUTPUTS)
                assert not fails, fails
    for cid in ("needle-assoc", "needle-assoc/RA_ASSOC", "needle-lform", "blend-needle", "blend-base"):
        print(cid, " ".join("%s %.1f" % kv for kv in per_case[cid].items()))
    rest = {k: max(v[k] for c, v in per_case.items() if "needle" not in c) for k in worst}
    print("without the needle scene: " + ", ".join("%s %.1f" % kv for kv in rest.items()))
    print("worst ratio per array, fp32 references only: " + ", ".join("%s %.1f" % kv for kv in worst.items()))
    assert 2.0 * max(worst.values()) <= br.K, worst
    # the RA_ASSOC class on needles, judged as a class of its own: its K must not come out above 64, or it would have to leave the row bar (tests/bwd_rows.py)
    assert 2.0 * max(per_case["needle-assoc/RA_ASSOC"].values()) <= 64.0, per_case["needle-assoc/RA_ASSOC"]


def test_verdict_flags_a_planted_row_error(base):
    inp, ref, _ = base
    rows, zr, nz = br.seed_rows(2000, "all", ref["radii"], 105)
    inter, refs, r64, live = br.reference(inp, br.fwd_like_of(ref), rows, br.rec_of(ref), "lform")
    assert not br.row_verdict(refs[1], refs, r64, live, names=br.CHAIN_OUTPUTS)[0]
    victims = {"dL_dmeans3D": int(np.flatnonzero(live)[3]), "dL_dsh": int(np.flatnonzero(live)[40]), "dL_drotations": int(np.flatnonzero(live)[-1])}
    hip = {k: np.array(refs[0][k], np.float64) for k in br.CHAIN_OUTPUTS}
    for name, i in victims.items():
        _, _, rho, rho_bar, _ = br.row_ratios(refs[0][name], [f[name] for f in refs], r64[name], live)
        t = np.asarray(r64[name]).reshape(2000, -1)[i]
        flat = hip[name].reshape(2000, -1)
        flat[i, np.argmax(np.abs(t))] = t[np.argmax(np.abs(t))] * (1.0 + 100.0 * br.K * rho_bar)
    dead = int(zr[0])
    hip["dL_dcov3D"][dead, 2] = 1e-30          # a row that must be all zero
    fails, _ = br.row_verdict(hip, refs, r64, live, names=br.CHAIN_OUTPUTS)
    assert sorted((f[0], f[1]) for f in fails) == sorted(list(victims.items()) + [("dL_dcov3D", dead)]), br.verdict_message(fails)
    assert "dL_dcov3D[%d]" % dead in br.verdict_message(fails)


def test_short_bounds_hold_for_a_float32_evaluation_and_catch_a_wrong_constant(base):
    """`check_short` on a numpy float32 evaluation of the row contract (one operation at a time) passes; with the exp2 unscale forgotten, or W / 2 taken for H / 2, it does not."""
    inp, ref, _ = base
    W, H = inp["W"], inp["H"]
    rec = br.rec_of(ref)
    rows, zr, nz = br.seed_rows(2000, "all", ref["radii"], 105)
    live = br.live_rows(rows, ref["radii"])
    inter = br.intermediates(rows, rec, W, H, "lform")
    for k in br.SHORT_OUTPUTS:
        inter[k][~live] = 0.0
    f = np.float32
    a, b, c, o = rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 2]

    def evaluate(u=br.EXP2_UNSCALE, hh=f(0.5 * H)):
        hip = {"dL_dmeans2D": np.zeros((2000, 3), f), "dL_dmeans2D_abs": np.zeros((2000, 3), f), "dL_dconic": np.zeros((2000, 4), f)}
        hip["dL_dmeans2D"][:, 0] = -f(0.5 * W) * (a * rows[:, 0] + b * rows[:, 1]); hip["dL_dmeans2D"][:, 1] = -hh * (c * rows[:, 1] + b * rows[:, 0])
        hip["dL_dmeans2D_abs"][:, 0] = f(0.5 * W) * (rows[:, 2] * u); hip["dL_dmeans2D_abs"][:, 1] = hh * (rows[:, 3] * u)
        hip["dL_dconic"][:, 0] = f(-0.5) * rows[:, 4]; hip["dL_dconic"][:, 1] = f(-0.5) * rows[:, 5]; hip["dL_dconic"][:, 3] = f(-0.5) * rows[:, 6]
        with np.errstate(all="ignore"):
            hip["dL_dopacity"] = np.where(o > 0, rows[:, 7] / np.where(o > 0, o, f(1)), f(0)).reshape(-1, 1)
        hip["dL_dcolors"] = rows[:, 8:11].copy()
        hip["dL_dall_map"] = np.concatenate([rows[:, 11:14], np.zeros((2000, 1), f), rows[:, 14:15]], axis=1)
        for k in hip:
            hip[k][~live] = 0
        return hip
    assert not br.check_short(evaluate(), inter, live)
    bad = br.check_short(evaluate(u=f(1.0)), inter, live)
    assert bad and {x[0] for x in bad} == {"dL_dmeans2D_abs"}
    bad = br.check_short(evaluate(hh=f(0.5 * W)), inter, live)
    assert {x[0] for x in bad} == {"dL_dmeans2D", "dL_dmeans2D_abs"} and {x[2] for x in bad} == {1}
