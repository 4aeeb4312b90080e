"""ibgs_amd.registration on the MI355X against the host restatement of its contract (tests/registration_ref.py: numpy, no code shared with the kernels):
transform and crop to the bit, voxel_down_sample to one f32 ulp, the ICP moments to the round-off of an f64 sum, the ICP loop and the TnT chain against the
planted similarity, and the contract's edges."""
import numpy as np
import pytest
import torch

from ibgs_amd import _lib, registration as reg
from tests import mesh_eval_ref
from tests import registration_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
# an 8-vertex concave polygon in (u, v): a square with a slot cut into its top
POLY_UV = np.array([[-1, -1], [1, -1], [1, 0.5], [0.25, 0.5], [0.25, -0.25], [-0.25, -0.25], [-0.25, 1], [-1, 1]], np.float64)
AFFINE = np.array([[0.9, 0.2, -0.1, 0.3], [-0.15, 1.1, 0.05, -0.2], [0.02, -0.3, 0.8, 0.1], [0, 0, 0, 1]], np.float64)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _polygon(axis):
    w, u, v = ref.AXES[axis]
    poly = np.full((len(POLY_UV), 3), 7.0)          # (the coordinate along the axis is not used)
    poly[:, u], poly[:, v] = POLY_UV[:, 0], POLY_UV[:, 1]
    return poly


# ---- transform ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", [("identity", np.identity(4)), ("similarity", ref.PLANTED), ("affine", AFFINE)])
def test_transform_is_the_restatement_to_the_bit(name, T):
    p = (np.random.default_rng(11).normal(size=(10_000, 3)) * [1.0, 30.0, 0.01]).astype(F32)
    d = _t(p)
    got = reg.transform(d, T)
    assert got.dtype == torch.float32 and got.shape == (10_000, 3) and torch.equal(d, _t(p))          # the input is not written
    assert got.cpu().numpy().tobytes() == ref.transform(p, T).tobytes()
    if name == "identity":
        assert got.cpu().numpy().tobytes() == p.tobytes()
    assert reg.transform(d[:0], T).shape == (0, 3)
    bad = p.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        reg.transform(_t(bad), T)


# ---- crop ---------------------------------------------------------------------------------------------------------------------------------------------
def _crop_points(axis):
    w, u, v = ref.AXES[axis]
    rng = np.random.default_rng(12 + w)
    p = rng.uniform(-1.3, 1.3, (5_000, 3)).astype(F32)
    p[:400, v] = rng.choice(POLY_UV[:, 1], 400).astype(F32)          # exactly at a vertex's v: the half-open rule
    p[400:500, u] = rng.choice(POLY_UV[:, 0], 100).astype(F32)       # exactly on a vertical edge's u
    p[500:600, w] = F32(-0.5)                                        # exactly axis_min and axis_max (closed), and one step outside
    p[600:700, w] = F32(0.75)
    p[700:750, w] = np.nextafter(F32(-0.5), F32(-1))
    p[750:800, w] = np.nextafter(F32(0.75), F32(1))
    return p


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_crop_masks_equal_the_restatement(axis):
    p, poly = _crop_points(axis), _polygon(axis)
    vol = reg.CropVolume(axis, -0.5, 0.75, poly)
    want = ref.crop(p, axis, -0.5, 0.75, poly)
    d = _t(p)
    got = reg.crop(d, vol)
    assert got.dtype == torch.bool and got.shape == (5_000,)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert 500 < want.sum() < 3_000 and want[:400].any() and not want[:400].all() and want[500:700].any() and not want[700:800].any()
    # through the fused T, and through transform followed by crop: the same mask, and the restatement's
    for T in (ref.PLANTED, AFFINE):
        fused = reg.crop(d, vol, T).cpu().numpy()
        np.testing.assert_array_equal(fused, reg.crop(reg.transform(d, T), vol).cpu().numpy())
        np.testing.assert_array_equal(fused, ref.crop(p, axis, -0.5, 0.75, poly, T=T))
        assert 300 < fused.sum() < 3_000
    np.testing.assert_array_equal(reg.crop(d, vol, np.identity(4)).cpu().numpy(), want)
    assert reg.crop(d[:0], vol).shape == (0,)


def test_crop_with_the_largest_polygon():
    a = np.linspace(0, 2 * np.pi, 1024, endpoint=False)
    r = 1.0 + 0.3 * np.sin(7 * a)
    poly = np.stack([r * np.cos(a), r * np.sin(a), np.zeros_like(a)], 1)
    p = np.random.default_rng(13).uniform(-1.4, 1.4, (3_000, 3)).astype(F32)
    got = reg.crop(_t(p), reg.CropVolume("Z", -1.0, 1.0, poly)).cpu().numpy()
    np.testing.assert_array_equal(got, ref.crop(p, "Z", -1.0, 1.0, poly))
    assert 300 < got.sum() < 2_000


# ---- voxel thinning -----------------------------------------------------------------------------------------------------------------------------------
def _voxel_cloud(case):
    rng = np.random.default_rng(14)
    if case == "one per voxel":
        return rng.uniform(-3, 1, (20_000, 3)).astype(F32), 0.147
    if case == "ten per voxel":
        return rng.uniform(-3, 1, (20_000, 3)).astype(F32), 0.32
    if case == "more than 1024 workgroups":
        return rng.uniform(-3, 1, (300_000, 3)).astype(F32), 0.05
    # v = 0.25: points on multiples of v / 2 (every second one on a voxel face: the grid's origin is lo - v / 2 = -3.125), 5 000 points in the one voxel
    # [-1.125, -0.875)^3 (the whole-wave path), and voxels of exactly 63 .. 129 points around the 64-point threshold
    v = 0.25
    grid = rng.integers(-24, 8, (15_000, 3)) * 0.125
    grid[0] = -3.0
    blob = rng.uniform(-1.1, -0.9, (5_000, 3))
    sized = [np.array([0.5 + 0.25 * j, 1.5, 0.5]) + rng.uniform(-0.05, 0.05, (n, 3)) for j, n in enumerate((63, 64, 65, 128, 129))]
    p = np.concatenate([grid, blob] + sized).astype(F32)
    rng.shuffle(p)
    return p, v


@pytest.mark.parametrize("case", ["one per voxel", "ten per voxel", "one voxel of 5000 and points on faces", "more than 1024 workgroups"])
def test_voxel_down_sample_against_the_restatement(case):
    p, v = _voxel_cloud(case)
    want, wkeys, counts, over = ref.voxel_down_sample(p, v)
    assert over == 0
    if case == "one per voxel":
        assert 1.0 < len(p) / len(want) < 2.5
    elif case == "ten per voxel":
        assert 8 < len(p) / len(want) < 14
    elif case.startswith("one voxel"):
        assert counts.max() >= 5_000 and set((63, 64, 65, 128, 129)) <= set(counts.tolist())
    d = _t(p)
    got, keys = reg.voxel_down_sample(d, v, return_keys=True)
    assert got.shape == (len(want), 3) and got.dtype == torch.float32          # the row count
    np.testing.assert_array_equal(keys.cpu().numpy(), wkeys)                  # ... and the key order
    g = got.cpu().numpy()
    ulp = np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    err = np.abs(g.astype(np.float64) - want)
    exact = int((g == want.astype(F32)).all(1).sum())
    print("\n[voxel %s] N %d -> M %d (largest voxel %d points); rows equal to the rounded f64 mean: %d of %d; largest error %.3f ulp"
          % (case, len(p), len(g), counts.max(), exact, len(g), float((err / ulp).max())))
    assert np.all(err <= ulp), float((err / ulp).max())
    small = counts <= _lib.PCREG_LONG_SEGMENT          # summed in index order, like the restatement: the same bits
    assert g[small].tobytes() == want[small].astype(F32).tobytes()
    for _ in range(2):          # three runs, identical bytes
        again = reg.voxel_down_sample(d, v)
        assert again.cpu().numpy().tobytes() == g.tobytes()
    assert torch.equal(d, _t(p))


def test_voxel_down_sample_edges():
    p = np.random.default_rng(15).uniform(-3, 1, (2_000, 3)).astype(F32)
    over = ref.voxel_down_sample(p, 1e-6)[3]
    assert 1_600 < over < 1_850          # a point fits only if all three coordinates lie within 2^21 voxels = 2.1 of the minimum: (2.1 / 4)^3 = 14 % of them do
    with pytest.raises(ValueError, match=r"voxel size 1e-06 is too small for the cloud's extent: %d point" % over):
        reg.voxel_down_sample(_t(p), 1e-6)
    empty = reg.voxel_down_sample(_t(p[:0]), 0.1)
    assert empty.shape == (0, 3) and empty.dtype == torch.float32 and empty.is_cuda
    out, keys = reg.voxel_down_sample(_t(p[:0]), 0.1, return_keys=True)
    assert out.shape == (0, 3) and keys.shape == (0,) and keys.dtype == torch.int64
    one = reg.voxel_down_sample(_t(p[:1]), 0.1).cpu().numpy()
    assert one.tobytes() == p[:1].tobytes()
    same = reg.voxel_down_sample(_t(np.repeat(p[:1], 1_000, 0)), 0.1).cpu().numpy()          # one voxel holds every point
    assert same.shape == (1, 3) and np.all(np.abs(same - p[:1]) <= np.spacing(np.abs(p[:1])))
    bad = p.copy()
    bad[5, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        reg.voxel_down_sample(_t(bad), 0.1)
    nc = _t(np.concatenate([p, p[:, :1]], 1))[:, :3]          # a non-contiguous view
    assert not nc.is_contiguous()
    assert reg.voxel_down_sample(nc, 0.2).cpu().numpy().tobytes() == reg.voxel_down_sample(_t(p), 0.2).cpu().numpy().tobytes()


# ---- the ICP scene ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """2 000 + 500 source points, their planted image with jittered duplicates, and what the restatement's ICP makes of them (computed once)."""
    src, tgt = ref.icp_scene(2_000, 500, seed=1)
    return {"src": src, "tgt": tgt, "ref": ref.icp(src, tgt, 0.5)}


def _tdist(T):
    return float(np.abs(np.asarray(T) - ref.PLANTED).max())


@pytest.mark.parametrize("case", ["one workgroup per 256", "more than 1024 workgroups"])
def test_moments_of_one_step(scene, case):
    src, tgt = scene["src"], scene["tgt"]
    if case != "one workgroup per 256":          # the grid-stride path: above 1024 x 256 queries
        rng = np.random.default_rng(16)
        src = (np.tile(src, (110, 1)).astype(np.float64) + 0.01 * rng.normal(size=(110 * len(src), 3))).astype(F32)
    T = ref.similarity(1.01, 1.0, (0.3, -0.5, 0.8), (0.02, -0.01, 0.02))          # part of the way: at max_dist 0.03 some points have no correspondence
    q = ref.transform(src, T)
    _, widx = mesh_eval_ref.nearest(q, tgt, 0.03)
    terms = ref.moment_terms(q, tgt, widx, ref.pivot_of(tgt))
    n = len(terms)
    assert 0.3 * len(src) < n < 0.98 * len(src)
    m, pivot, idx = reg.moments(_t(src), _t(tgt), 0.03, T)
    assert pivot.tobytes() == ref.pivot_of(tgt).tobytes()
    np.testing.assert_array_equal(idx.cpu().numpy(), widx)
    assert m.shape == (18,) and m[0] == n          # the integer
    want, scale = terms.sum(0), np.abs(terms).sum(0)
    bound = (n + 16) * 2.0 ** -52 * scale          # the order of an f64 sum of n terms, nothing else: the terms themselves are the restatement's to the bit
    err = np.abs(m[1:] - want)
    print("\n[moments %s] n %d of %d; largest error / bound %.3g" % (case, n, len(src), float((err / bound).max())))
    assert np.all(err <= bound), (err / bound).max()
    m2 = reg.moments(_t(src), _t(tgt), 0.03, T)[0]
    assert m2.tobytes() == m.tobytes()


def test_icp_recovers_the_planted_similarity(scene):
    r0 = scene["ref"]
    r = reg.icp(_t(scene["src"]), _t(scene["tgt"]), 0.5, max_iter=20)
    print("\n[icp] restatement: %d iterations, |T - planted| %.3g, rmse %.6g; device: %d iterations, |T - planted| %.3g, rmse %.6g, |T - T_ref| %.3g"
          % (r0["iterations"], _tdist(r0["transformation"]), r0["inlier_rmse"], r.iterations, _tdist(r.transformation), r.inlier_rmse,
             float(np.abs(r.transformation - r0["transformation"]).max())))
    assert 3 <= r0["iterations"] < 20
    assert r.iterations == r0["iterations"]
    assert _tdist(r.transformation) <= max(2 * _tdist(r0["transformation"]), 1e-9)
    assert r.n_correspondences == r0["n_correspondences"] and r.fitness == r0["fitness"] and abs(r.inlier_rmse - r0["inlier_rmse"]) <= 1e-9
    assert r.transformation.dtype == np.float64 and r.transformation[3].tolist() == [0, 0, 0, 1]
    again = reg.icp(_t(scene["src"]), _t(scene["tgt"]), 0.5, max_iter=20)
    assert again.transformation.tobytes() == r.transformation.tobytes() and again[1:] == r[1:]


def test_icp_edges(scene):
    src, tgt = _t(scene["src"]), _t(scene["tgt"])
    with pytest.raises(reg.RegistrationError, match="iteration 0: [012] correspondence"):
        reg.icp(src, tgt, 1e-7)
    with pytest.raises(reg.RegistrationError, match="iteration 0"):
        reg.icp(src, tgt[:0], 0.5)
    # max_iter = 0: init comes back, with the fitness and rmse measured there
    init = ref.similarity(1.0, 1.0, (0, 0, 1), (0.01, 0, 0))
    r = reg.icp(src, tgt, 0.5, init=init, max_iter=0)
    w = ref.icp(scene["src"], scene["tgt"], 0.5, init=init, max_iter=0)
    assert r.iterations == 0 and r.transformation.tobytes() == init.tobytes()
    assert r.n_correspondences == w["n_correspondences"] and r.fitness == w["fitness"] and abs(r.inlier_rmse - w["inlier_rmse"]) <= 1e-12
    # three updates, then on a side stream and from non-contiguous inputs: the same bits
    base = reg.icp(src, tgt, 0.5, max_iter=3)
    assert base.iterations == 3
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = reg.icp(src, tgt, 0.5, max_iter=3)
    s.synchronize()
    assert side.transformation.tobytes() == base.transformation.tobytes() and side.inlier_rmse == base.inlier_rmse
    wide_s = _t(np.concatenate([scene["src"], scene["src"][:, :2]], 1))[:, :3]
    skip_t = _t(np.repeat(scene["tgt"], 2, 0))[::2]
    assert not wide_s.is_contiguous() and not skip_t.is_contiguous()
    nc = reg.icp(wide_s, skip_t, 0.5, max_iter=3)
    assert nc.transformation.tobytes() == base.transformation.tobytes()
    bad = scene["src"].copy()
    bad[3, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        reg.icp(_t(bad), tgt, 0.5)


# ---- the TnT chain ------------------------------------------------------------------------------------------------------------------------------------
TNT_SEED, TAU = 2, 0.02
# the selection volume, in the ground truth's frame: the sheet and the wall without the corner beyond x + y = 1.6
TNT_VOLUME = ("Z", -0.7, 0.7, np.array([[-1.3, -1.3, 0], [1.3, -1.3, 0], [1.3, 0.3, 0], [0.3, 1.3, 0], [-1.3, 1.3, 0]], np.float64))


def test_evaluate_tnt_against_the_restatement_chain():
    pred, gt = ref.icp_scene(8_000, 2_000, seed=TNT_SEED)
    w = ref.evaluate_tnt(pred, gt, np.identity(4), TNT_VOLUME, TAU)
    # the condition on the inputs, on the restatement alone: the distances within 1e-5 tau of tau are at most 0.1 % of each cloud
    tau32 = float(F32(TAU))
    edge_p = int((np.abs(w["dist_pred"].astype(np.float64) - tau32) <= 1e-5 * TAU).sum())
    edge_r = int((np.abs(w["dist_gt"].astype(np.float64) - tau32) <= 1e-5 * TAU).sum())
    assert edge_p <= 1e-3 * w["n_pred"] and edge_r <= 1e-3 * w["n_gt"]
    assert 0.5 < w["precision"] <= 1 and 0.5 < w["recall"] <= 1 and len(w["rounds"]) == 3
    g = reg.evaluate_tnt(_t(pred), _t(gt), np.identity(4), reg.CropVolume(*TNT_VOLUME), TAU)
    print("\n[evaluate_tnt] restatement: P %.4f R %.4f F %.4f, n %d / %d of %d / %d, borderline %d / %d, iterations %s, |T - planted| %.3g; device: P %.4f R %.4f F %.4f, "
          "n %d / %d of %d / %d, iterations %s, |T - planted| %.3g"
          % (w["precision"], w["recall"], w["fscore"], w["n_precision"], w["n_recall"], w["n_pred"], w["n_gt"], edge_p, edge_r, [r["iterations"] for r in w["rounds"]],
             _tdist(w["transformation"]), g["precision"], g["recall"], g["fscore"], g["n_precision"], g["n_recall"], g["n_pred"], g["n_gt"],
             [r.iterations for r in g["rounds"]], _tdist(g["transformation"])))
    assert g["n_pred"] == w["n_pred"] and g["n_gt"] == w["n_gt"]          # the thinned cloud sizes
    assert 0 < g["n_gt_cropped"] < len(gt) and 0 < g["n_pred_cropped"] < len(pred)          # the volume cuts
    assert abs(g["n_precision"] - w["n_precision"]) <= edge_p and abs(g["n_recall"] - w["n_recall"]) <= edge_r
    assert _tdist(g["transformation"]) <= max(2 * _tdist(w["transformation"]), 1e-9)
    assert g["precision"] == g["n_precision"] / g["n_pred"] and g["recall"] == g["n_recall"] / g["n_gt"]
    assert abs(g["fscore"] - 2 * g["precision"] * g["recall"] / (g["precision"] + g["recall"])) <= 1e-15
    assert len(g["rounds"]) == 3 and all(isinstance(r, reg.ICPResult) for r in g["rounds"])
