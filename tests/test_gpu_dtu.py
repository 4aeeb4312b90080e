"""ibgs_amd.dtu on the MI355X against the host restatement of its contract (tests/dtu_ref.py: numpy, no code shared with the kernels), bit for bit, at the
smallest shapes at which the kernels can still go wrong: word seams, radii beyond the image, half-pixel ties, divisors of zero, culled corners."""
import types

import numpy as np
import pytest
import torch

from ibgs_amd import dtu, tsdf
from tests import dtu_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
RADII = (0, 1, 24, 40)
CULL_RADIUS = 6


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _mesh(v, f, c, n):
    return tsdf.TriangleMesh(_t(np.asarray(v, F32)), _t(np.asarray(f, np.int32)), _t(np.asarray(c, F32)), _t(np.asarray(n, F32)))


def _np(mesh):
    return tuple(t.cpu().numpy() for t in mesh)


# ---- shared inputs and their restated results, computed once and left unchanged ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def views():
    P, raw = ref.three_views(), ref.blob_masks()
    dilated = ref.dilate_all(raw, CULL_RADIUS)
    return types.SimpleNamespace(P=P, raw=raw, dilated=dilated, bits=ref.pack_bits(dilated))


@pytest.fixture(scope="module")
def grid(views):
    v, f, c, n = ref.grid_mesh_case()
    keep = ref.cull_vertices(v, views.P[:2], views.dilated[:2])
    return types.SimpleNamespace(v=v, f=f, c=c, n=n, keep=keep)


# ---- 1. dilation ---------------------------------------------------------------------------------------------------------------------------------------
def _patterns(H, W):
    """uint8 masks: marked pixels (values 1 and 255), a single centre pixel, a full mask, an empty one, noise."""
    rng = np.random.default_rng(H * 1000 + W)
    marked = np.zeros((H, W), np.uint8)
    for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, min(63, W - 1)), (H // 3, min(64, W - 1)), (H // 4, W - 1))):
        marked[y, x] = 255 if k % 2 else 1
    centre = np.zeros((H, W), np.uint8)
    centre[H // 2, W // 2] = 7
    noise = (rng.uniform(size=(H, W)) < 0.01).astype(np.uint8) * 255
    return np.stack([marked, centre, np.full((H, W), 1, np.uint8), np.zeros((H, W), np.uint8), noise])


@pytest.mark.parametrize("W", [40, 64, 65, 130])
@pytest.mark.parametrize("H", [30, 67])
def test_dilation_bit_for_bit(H, W):
    pats = _patterns(H, W)
    yy, xx = np.mgrid[:H, :W]
    for r in RADII:
        want = ref.dilate_all(pats, r)
        disc = (xx - W // 2) ** 2 + (yy - H // 2) ** 2 <= r * r          # the clipped disc, not through the restatement
        np.testing.assert_array_equal(want[1], disc)
        assert want[2].all() and not want[3].any() and (r == 0 or want[0].sum() > 7)
        words = ref.pack_bits(want)
        for n in (0, 1, 3, 5):
            src = _t(pats[:n])
            before = src.clone()
            got = dtu.dilate_masks(src, r)
            assert (got.H, got.W) == (H, W) and got.words.dtype == torch.int64 and tuple(got.words.shape) == (n, H, (W + 63) // 64)
            g = got.words.cpu().numpy()
            img, pad = ref.unpack_bits(g, W)
            assert not pad.any(), "pad bits set (H %d, W %d, r %d, n %d)" % (H, W, r, n)
            bad = np.argwhere(img != want[:n])
            assert len(bad) == 0, "H %d, W %d, r %d, n %d: %d pixel(s) differ, first (view, y, x) = %s" % (H, W, r, n, len(bad), bad[0].tolist())
            np.testing.assert_array_equal(g, words[:n])
            assert torch.equal(src, before)
        got_bool = dtu.dilate_masks(_t(pats != 0), r)          # bool input: the same bits
        np.testing.assert_array_equal(got_bool.words.cpu().numpy(), words)


def test_dilation_radius_beyond_one_word():
    """r > 64 takes the kernel's wider windows (two, three and four words to either side)."""
    H, W = 20, 330
    pats = _patterns(H, W)
    pats = (pats[0] | pats[4])[None]          # the marked pixels and the noise in one mask
    for r in (64, 65, 130, 255):
        got = dtu.dilate_masks(_t(pats), r).words.cpu().numpy()
        np.testing.assert_array_equal(got, ref.pack_bits(ref.dilate_all(pats, r)), err_msg="r %d" % r)


# ---- 2. vertex culling ---------------------------------------------------------------------------------------------------------------------------------
def test_cull_vertices_bit_for_bit(views):
    v, P, n_box, n_lattice = ref.cull_vertices_case()
    W, H = ref.VIEW_W, ref.VIEW_H
    passes, valids = zip(*(ref.view_passes(v, P[i], views.dilated[i]) for i in range(3)))
    passes, valids = np.array(passes), np.array(valids)
    want = passes.all(0)
    np.testing.assert_array_equal(want, ref.cull_vertices(v, P, views.dilated))
    rejected_by = (~passes).sum(0)
    shares = {"kept": want.mean(), "seen and kept": (want & valids.any(0)).mean(), "rejected by one view": (rejected_by == 1).mean(),
              "outside every view": (~valids.any(0)).mean()}
    print("\n[cull_vertices] V %d: %s" % (len(v), ", ".join("%s %.1f %%" % (k, 100 * s) for k, s in shares.items())))
    assert all(s >= 0.05 for s in shares.values()), shares
    # the lattice sits on exact half-pixels of view 0, where the chain and rint(u) part ways
    lat = slice(n_box, n_box + n_lattice)
    u, vv, den = ref.project(v[lat], P[0])
    assert np.all(u - np.floor(u) == 0.5) and np.all(vv - np.floor(vv) == 0.5) and np.all(den == 32)
    ok, ix, iy = ref.pixel_of(u, vv, W, H)
    assert (ix[ok] != np.rint(u[ok])).sum() > 100
    # behind the cameras, and the vertex whose divisor is zero in view 2
    assert (ref.project(v[lat.stop:-1], P[0])[2] < 0).sum() >= 300 and ref.project(v[-1:], P[2])[2][0] == 0 and not valids[2, -1]
    bits = dtu.MaskBits(_t(views.bits), H, W)
    tv, tp = _t(v), _t(P)
    before = (tv.clone(), tp.clone(), bits.words.clone())
    got = dtu.cull_vertices(tv, tp, bits)
    assert got.dtype == torch.bool and tuple(got.shape) == (len(v),)
    g = got.cpu().numpy()
    bad = np.flatnonzero(g != want)
    assert len(bad) == 0, "%d vertices differ, first %d: %s (lattice %d)" % (len(bad), bad[0], v[bad[0]].tolist(), ((bad >= lat.start) & (bad < lat.stop)).sum())
    assert torch.equal(tv, before[0]) and torch.equal(tp, before[1]) and torch.equal(bits.words, before[2])
    # the device's own dilation gives the same answer; single views; no view; no vertex
    np.testing.assert_array_equal(dtu.cull_vertices(tv, tp, dtu.dilate_masks(_t(views.raw), CULL_RADIUS)).cpu().numpy(), want)
    for i in range(3):
        one = dtu.cull_vertices(tv, tp[i:i + 1], dtu.MaskBits(bits.words[i:i + 1].contiguous(), H, W)).cpu().numpy()
        np.testing.assert_array_equal(one, passes[i], err_msg="view %d" % i)
    assert dtu.cull_vertices(tv, tp[:0], dtu.MaskBits(bits.words[:0], H, W)).all()
    assert tuple(dtu.cull_vertices(tv[:0], tp, bits).shape) == (0,)


# ---- 3. the culled mesh --------------------------------------------------------------------------------------------------------------------------------
SCALE, OFFSET = 1.7, (0.1, -3.3, 7.7)


def _check_mesh_equal(got, want_v, want_f, want_c, want_n):
    gv, gf, gc, gn = _np(got)
    assert gv.dtype == F32 and gf.dtype == np.int32 and gv.shape == want_v.shape and gf.shape == want_f.shape
    np.testing.assert_array_equal(gv.view(np.uint32), want_v.view(np.uint32))
    np.testing.assert_array_equal(gf, want_f)
    np.testing.assert_array_equal(gc.view(np.uint32), want_c.view(np.uint32))
    np.testing.assert_array_equal(gn.view(np.uint32), want_n.view(np.uint32))


def test_cull_mesh_bit_for_bit(views, grid):
    v, f, keep = grid.v, grid.f, grid.keep
    V = len(v)
    fk = keep[f].all(1)
    assert len(f) == 1986 and 0.3 < keep.mean() < 0.8 and 0.3 < fk.mean() < 0.8          # the grid spans the masks' border
    lone = V - 3
    assert keep[lone] and not keep[lone + 1] and not fk[(f == lone).any(1)].any()          # kept, and every face it had is gone
    assert f[1001, 0] == f[1001, 1] and fk[1001]          # the face that repeats an index survives
    want_v, want_f, (want_c, want_n) = ref.cull_mesh(v, f, keep, SCALE, OFFSET, attrs=(grid.c, grid.n))
    assert len(want_v) == keep.sum() and len(want_f) == fk.sum() and not (want_f == np.cumsum(keep)[lone] - 1).any()
    assert np.array_equal(want_v[np.cumsum(keep)[lone] - 1], v[lone] * F32(SCALE) + np.array(OFFSET, np.float64).astype(F32))
    m = _mesh(v, f, grid.c, grid.n)
    before = [t.clone() for t in m]
    P, raw = _t(views.P[:2]), _t(views.raw[:2])
    got = dtu.cull_mesh(m, P, raw, radius=CULL_RADIUS, scale=SCALE, offset=OFFSET)
    _check_mesh_equal(got, want_v, want_f, want_c, want_n)
    assert all(torch.equal(a, b) for a, b in zip(m, before))
    # already dilated masks give the same mesh
    bits = dtu.dilate_masks(raw, CULL_RADIUS)
    _check_mesh_equal(dtu.cull_mesh(m, P, bits, scale=SCALE, offset=OFFSET), want_v, want_f, want_c, want_n)
    # scale 1, offset 0: the kept rows themselves
    same = dtu.cull_mesh(m, P, bits)
    np.testing.assert_array_equal(same.vertices.cpu().numpy().view(np.uint32), v[keep].view(np.uint32))
    # no face
    none = dtu.cull_mesh(_mesh(v, np.zeros((0, 3), np.int32), grid.c, grid.n), P, bits, scale=SCALE, offset=OFFSET)
    assert tuple(none.faces.shape) == (0, 3) and none.faces.dtype == torch.int32
    np.testing.assert_array_equal(none.vertices.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
    # no view: everything stays; no vertex
    everything = dtu.cull_mesh(m, P[:0], raw[:0], radius=CULL_RADIUS)
    assert torch.equal(everything.vertices, m.vertices) and torch.equal(everything.faces, m.faces)
    z = np.zeros((0, 3), F32)
    empty = dtu.cull_mesh(_mesh(z, np.zeros((0, 3), np.int32), z, z), P, bits)
    assert tuple(empty.vertices.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3)


def test_cull_mesh_refuses_a_face_index_out_of_range(views, grid):
    P, raw = _t(views.P[:2]), _t(views.raw[:2])
    for bad in (len(grid.v), -1, 2 ** 31 - 1):
        f = grid.f.copy()
        f[700, 1] = bad
        m = _mesh(grid.v, f, grid.c, grid.n)
        before = [t.clone() for t in m]
        with pytest.raises(dtu.DTUError, match="1 triangle"):
            dtu.cull_mesh(m, P, raw, radius=CULL_RADIUS)
        assert all(torch.equal(a, b) for a, b in zip(m, before))


# ---- 4. the filters ------------------------------------------------------------------------------------------------------------------------------------
def test_filters_bit_for_bit():
    p, obs, bb, res, patch = ref.filter_case()
    want_in, want_obs = ref.obs_mask_filter(p, obs, bb, res, patch)
    lo, hi = ref.box_bounds(bb, patch)
    assert 0.2 < want_in.mean() < 0.8 and 0.05 < want_obs.mean() < want_in.mean()
    assert want_in[20000:20200].all() and not want_in[20200:20400].any()          # on lo: inside; on hi: outside
    assert not want_in[20600:20800].any() and want_in[20800:].all()          # one ulp below lo: outside; one ulp below hi: inside
    tie = p[20400:20600].astype(np.float64)
    g = (tie - bb[0].astype(np.float64)) / res
    assert (np.abs(g - np.floor(g) - 0.5) == 0).any(axis=1).all()
    tp, tobs = _t(p), _t(obs)
    before = (tp.clone(), tobs.clone())
    got = dtu.obs_mask_filter(tp, tobs, bb, res, patch)
    assert got.inbound.dtype == torch.bool and got.in_obs.dtype == torch.bool
    np.testing.assert_array_equal(got.inbound.cpu().numpy(), want_in)
    np.testing.assert_array_equal(got.in_obs.cpu().numpy(), want_obs)
    assert torch.equal(tp, before[0]) and torch.equal(tobs, before[1])
    as_bool = dtu.obs_mask_filter(tp, _t(obs != 0), torch.as_tensor(bb), res, patch)
    assert torch.equal(as_bool.in_obs, got.in_obs)
    default_patch = dtu.obs_mask_filter(tp, tobs, bb, res)          # patch = 60: everything is in bounds
    assert default_patch.inbound.all()
    np.testing.assert_array_equal(default_patch.in_obs.cpu().numpy(), ref.obs_mask_filter(p, obs, bb, res, 60.0)[1])
    empty = dtu.obs_mask_filter(tp[:0], tobs, bb, res, patch)
    assert tuple(empty.inbound.shape) == (0,) and tuple(empty.in_obs.shape) == (0,)
    for bad in (float("nan"), float("inf")):
        q = p[:100].copy()
        q[37, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            dtu.obs_mask_filter(_t(q), tobs, bb, res, patch)
        with pytest.raises(ValueError, match="non-finite"):
            dtu.above_plane(_t(q), [0, 0, 1, 0])


def test_above_plane_bit_for_bit():
    rng = np.random.default_rng(11)
    plane = np.array([0.25, -0.5, 1.0, -2.0])
    p = rng.uniform(-6, 6, (20_000, 3)).astype(F32)
    on = rng.integers(-8, 8, (500, 3)).astype(np.float64) / 4
    on[:, 2] = 2.0 - 0.25 * on[:, 0] + 0.5 * on[:, 1]          # exactly on the plane (all terms exact in binary)
    just = on.astype(F32)
    just[:, 2] = np.nextafter(just[:, 2], F32(np.inf))          # one ulp above it
    p = np.concatenate([p, on.astype(F32), just])
    want = ref.above_plane(p, plane)
    assert not want[20000:20500].any() and want[20500:].all() and 0.3 < want[:20000].mean() < 0.7          # the strict >
    got = dtu.above_plane(_t(p), plane)
    assert got.dtype == torch.bool
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(dtu.above_plane(_t(p), torch.as_tensor(plane)).cpu().numpy(), want)
    assert tuple(dtu.above_plane(_t(p[:0]), plane).shape) == (0,)


# ---- 5. the chain --------------------------------------------------------------------------------------------------------------------------------------
def _order(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randperm(n, generator=g, device="cuda").cpu().numpy()


@pytest.mark.parametrize("with_cull", [False, True])
def test_evaluate_dtu_against_the_restated_composition(views, grid, with_cull):
    gt, obs, bb, res, plane, density, max_dist, patch = ref.eval_case()
    v, f = grid.v, grid.f
    shift = (0.25, 0.0, 0.0)
    cull = None
    if with_cull:
        v, f, _ = ref.cull_mesh(grid.v, grid.f, grid.keep, 1.0, shift)
        cull = dtu.Cull(_t(views.P[:2]), _t(views.raw[:2]), CULL_RADIUS, 1.0, shift)
    seed = 3
    n_cloud = len(ref.sampled_cloud(v, f, density))
    want = ref.evaluate_dtu(v, f, gt, obs, bb, res, plane, density, max_dist, patch, _order(n_cloud, seed))
    # the case is about the search among the in-bound points: some thinned points are out of bounds, and searching all of them gives another answer
    assert want["n_inbound"] < want["n_thinned"] and want["n_in_obs"] < want["n_inbound"] and 0 < want["n_d2s"] <= want["n_in_obs"]
    assert want["all_thinned"]["n_s2d"] > want["n_s2d"] and abs(want["all_thinned"]["mean_s2d"] - want["mean_s2d"]) > 1e-3
    got = dtu.evaluate_dtu(_mesh(grid.v, grid.f, grid.c, grid.n), _t(gt), _t(obs), bb, res, plane, density=density, max_dist=max_dist, patch=patch, seed=seed,
                           cull=cull)
    print("\n[evaluate_dtu%s] %s" % (", culled" if with_cull else "", got))
    for k in ("n_sampled", "n_thinned", "n_inbound", "n_in_obs", "n_above", "n_d2s", "n_s2d"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k, n in (("mean_d2s", got["n_d2s"]), ("mean_s2d", got["n_s2d"])):
        assert abs(got[k] - want[k]) <= (n + 16) * 2.0 ** -52 * abs(want[k]), (k, got[k], want[k])          # the order of an f64 sum of n non-negative terms
    assert got["overall"] == (got["mean_d2s"] + got["mean_s2d"]) / 2
    if with_cull:
        assert got["n_vertices_culled"] == len(grid.v) - len(v) > 0 and got["n_faces_culled"] == len(grid.f) - len(f) > 0
        as_tuple = dtu.evaluate_dtu(_mesh(grid.v, grid.f, grid.c, grid.n), _t(gt), _t(obs), bb, res, plane, density=density, max_dist=max_dist, patch=patch,
                                    seed=seed, cull=tuple(cull))
        assert all(as_tuple[k] == got[k] for k in got if k.startswith("n_")) and abs(as_tuple["overall"] - got["overall"]) <= 1e-12 * got["overall"]
    else:
        assert "n_vertices_culled" not in got and "n_faces_culled" not in got
        assert set(got) == {"mean_d2s", "mean_s2d", "overall", "n_d2s", "n_s2d", "n_sampled", "n_thinned", "n_inbound", "n_in_obs", "n_above"}


# ---- 6. streams ----------------------------------------------------------------------------------------------------------------------------------------
def test_cull_mesh_on_a_non_default_stream_and_twice(views, grid):
    m = _mesh(grid.v, grid.f, grid.c, grid.n)
    P, raw = _t(views.P[:2]), _t(views.raw[:2])
    want = dtu.cull_mesh(m, P, raw, radius=CULL_RADIUS, scale=SCALE, offset=OFFSET)
    again = dtu.cull_mesh(m, P, raw, radius=CULL_RADIUS, scale=SCALE, offset=OFFSET)
    assert all(torch.equal(a, b) for a, b in zip(want, again))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = dtu.cull_mesh(m, P, raw, radius=CULL_RADIUS, scale=SCALE, offset=OFFSET)
        filt = dtu.obs_mask_filter(got.vertices, _t(ref.eval_case()[1]), ref.eval_case()[2], 0.25, 0.25)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, got)) and len(got.vertices) == grid.keep.sum()
    assert torch.equal(filt.inbound, dtu.obs_mask_filter(want.vertices, _t(ref.eval_case()[1]), ref.eval_case()[2], 0.25, 0.25).inbound)
