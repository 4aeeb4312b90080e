"""ibgs_amd.mesh_eval on the MI355X against the host restatement of its contract (tests/mesh_eval_ref.py: numpy + scipy, no code shared with the kernels),
against closed forms that do not go through the restatement (the analytic sphere of tests/mesh_ref.floater_frames), at scale, and at the contract's edges."""
import os
import time
import types

import numpy as np
import pytest
import torch

from ibgs_amd import mesh, mesh_eval, tsdf
from tests import mesh_eval_ref as ref
from tests import mesh_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _mesh(v, f):
    return types.SimpleNamespace(vertices=_t(np.asarray(v, F32)), faces=_t(np.asarray(f, np.int32)))


def _ms(fn, reps=3):
    """Median of `reps` hipEvent timings after one warm-up."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------------------
def _check_sampling(v, f, density, what, include_vertices=True):
    want, counts, _ = ref.sample_surface(v, f, density, include_vertices=include_vertices)
    m = _mesh(v, f)
    before = (m.vertices.clone(), m.faces.clone())
    got = mesh_eval.sample_surface(m, density, include_vertices=include_vertices).cpu().numpy()
    assert got.shape == want.shape and got.dtype == F32, (what, got.shape, want.shape)          # counts (order follows from the positions below)
    ulp = np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    exact = int((got == want.astype(F32)).all(axis=1).sum())
    print("\n[sampling %s] F %d -> %d points (%d triangles yield none, largest %d); rows equal to the rounded f64 value: %d of %d"
          % (what, len(f), len(got), int((counts == 0).sum()), int(counts.max(initial=0)), exact, len(got)))
    assert np.all(err <= ulp), (what, float((err / ulp).max()))
    assert torch.equal(m.vertices, before[0]) and torch.equal(m.faces, before[1])
    return got, counts


def test_sampling_random_and_degenerate_triangles():
    v, f = ref.random_mesh(3000, seed=3, scale=0.5)
    n = len(v)
    v = np.concatenate([v, np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 0, 1], [1e-4, 0, 1], [0, 0.987, 1], [5, 5, 5]], F32)])
    extra = np.array([[0, 0, 1], [2, 2, 2], [n, n + 1, n + 2], [n + 2, n + 1, n], [n + 3, n + 4, n + 5], [n + 6, n + 6, n + 6], [n, n + 6, n + 1]], np.int32)
    f = np.concatenate([f[:1500], extra, f[1500:]])          # repeated indices, collinear triples, a sliver with n1 = 0, one honest triangle among them
    got, counts = _check_sampling(v, f, 0.05, "random + degenerate")
    assert counts[1500:1506].tolist() == [0] * 6 and counts[1506] > 0 and counts.sum() > 50_000
    _check_sampling(v, f, 0.05, "without vertices", include_vertices=False)
    _check_sampling(v, f, 1e3, "nothing sampled")          # every n is 0: the vertices alone
    # a shared-vertex mesh (marching-cubes like), fine and coarse
    gv, gf = mesh_ref.grid(40, 30, 0.1)
    _check_sampling(gv, gf, 0.03, "grid")
    _check_sampling(gv, gf, 0.2, "grid, coarser than the mesh")


def test_sampling_one_huge_triangle_among_thousands_that_yield_none():
    tv, tf = ref.random_mesh(6000, seed=4, scale=1e-4)          # all far smaller than the density
    tv = np.concatenate([tv, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)])
    f = np.concatenate([tf[:3100], np.array([[len(tv) - 3, len(tv) - 2, len(tv) - 1]], np.int32), tf[3100:]])
    got, counts = _check_sampling(tv, f, 0.002, "load balance")
    assert counts[3100] == 500 * 499 // 2 > 10 ** 5 and (counts == 0).sum() >= 5000
    m = _mesh(tv, f)
    ms = _ms(lambda: mesh_eval.sample_surface(m, 0.002))
    print("[sampling load balance] %.3f ms per call (two read-backs included)" % ms)


def test_sampling_limits_raise_before_allocating():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    m = _mesh(v, [[0, 1, 2]])
    n = 3 + 500 * 499 // 2
    assert len(mesh_eval.sample_surface(m, 0.002, max_points=n)) == n
    with pytest.raises(ValueError, match=str(n)):
        mesh_eval.sample_surface(m, 0.002, max_points=n - 1)
    with pytest.raises(ValueError, match="density is too small"):          # 10^5 per side: over the per-triangle limit, counted, never walked
        mesh_eval.sample_surface(m, 1e-5)
    big = _mesh(v * 1000, [[0, 1, 2]])          # 3 x 10^8 samples from one triangle: counted (by the whole wave), refused, never allocated
    with pytest.raises(ValueError, match="max_points"):
        mesh_eval.sample_surface(big, 1000 / 30000.5, max_points=10 ** 6)
    for bad in (3, -1, 2 ** 31 - 1, -2 ** 31):
        with pytest.raises(mesh_eval.MeshEvalError, match="out of range"):
            mesh_eval.sample_surface(_mesh(v, [[0, 1, 2], [0, 1, bad]]), 0.1)
    e = mesh_eval.sample_surface(_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)), 0.1)
    assert e.shape == (0, 3)
    assert mesh_eval.sample_surface(_mesh(v, np.zeros((0, 3), np.int32)), 0.1).cpu().numpy().tobytes() == v.tobytes()


# ---- thinning -----------------------------------------------------------------------------------------------------------------------------------------
def _check_thin(p, r, order, what):
    want = ref.downsample(p, r, order)
    pt = _t(p)
    before = pt.clone()
    ot = None if order is None else _t(np.asarray(order, np.int64))
    runs = [mesh_eval.downsample(pt, r, order=ot).cpu().numpy() for _ in range(3)]
    assert runs[0].dtype == bool and runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes(), what
    diff = int((runs[0] != want).sum())
    print("\n[thinning %s] N %d radius %g: %d kept, %d differ from the restatement" % (what, len(p), r, int(runs[0].sum()), diff))
    assert diff == 0, what
    assert torch.equal(pt, before)
    return runs[0]


def test_thinning_orders_of_one_cloud():
    p = ref.surface_cloud(60_000, seed=6, noise=0.005)
    dup = np.arange(0, 6000, 3)
    p[dup] = p[dup + 1]          # duplicate points: the later of a pair goes
    rng = np.random.default_rng(7)
    masks = [_check_thin(p, 0.02, o, w) for o, w in ((rng.permutation(len(p)), "shuffled"), (None, "index order"), (np.argsort(p[:, 0], kind="stable"), "x-sorted"))]
    assert not np.array_equal(masks[0], masks[1]) and 2000 < masks[0].sum() < 30_000
    assert not np.any(masks[1][dup + 1])          # visited after its twin: removed by it, or by whatever removed the twin
    _check_thin(p, 0.0, None, "radius 0: duplicates only")
    _check_thin(p + F32(1000.0), 0.02, None, "far from the origin")


def test_thinning_sorted_collinear_chain():
    n, r = 4000, 0.01
    x = np.cumsum(np.random.default_rng(8).uniform(0.3, 0.6, n)) * r          # every point within r of the one before: the decisions travel along the chain
    p = np.stack([x, 0.5 * x, np.zeros(n)], 1).astype(F32)
    keep = _check_thin(p, r, None, "sorted collinear chain")
    assert keep[0] and n // 4 < keep.sum() < n // 2
    _check_thin(p[::-1].copy(), r, None, "chain, visited from the far end")
    _check_thin(p, r, np.random.default_rng(9).permutation(n), "chain, shuffled")


def test_thinning_edges():
    e = mesh_eval.downsample(torch.zeros(0, 3, device="cuda"), 0.1)
    assert e.shape == (0,) and e.dtype == torch.bool
    assert mesh_eval.downsample(torch.zeros(1, 3, device="cuda"), 0.1).tolist() == [True]
    assert mesh_eval.downsample(torch.zeros(5, 3, device="cuda"), 0.1).tolist() == [True, False, False, False, False]
    assert mesh_eval.downsample(torch.zeros(5, 3, device="cuda"), 0.1, order=_t(np.array([3, 1, 0, 2, 4]))).tolist() == [False, False, False, True, False]
    p = _t(ref.surface_cloud(100, 1))
    for bad in ([0] * 100, list(range(1, 101)), [-1] + list(range(1, 100))):
        with pytest.raises(ValueError, match="permutation"):
            mesh_eval.downsample(p, 0.1, order=_t(np.array(bad, np.int64)))
    q = p.clone()
    q[17, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        mesh_eval.downsample(q, 0.1)


# ---- nearest ------------------------------------------------------------------------------------------------------------------------------------------
def _check_nearest(q, t, md, what):
    wd, wi = ref.nearest(q, t, md)
    qt, tt = _t(q), _t(t)
    before = (qt.clone(), tt.clone())
    got = mesh_eval.nearest(qt, tt, md)
    gd, gi = got.dist.cpu().numpy(), got.index.cpu().numpy()
    assert gd.dtype == F32 and gi.dtype == np.int32
    nd, ni = int((gd.view(np.uint32) != wd.view(np.uint32)).sum()), int((gi != wi).sum())
    print("\n[nearest %s] Q %d N %d max_dist %g: %d without a neighbour, %d dist and %d index differ from the restatement"
          % (what, len(q), len(t), md, int((gi < 0).sum()), nd, ni))
    assert nd == 0 and ni == 0, what
    assert torch.equal(qt, before[0]) and torch.equal(tt, before[1])
    return gd, gi


def test_nearest_against_the_restatement():
    t = ref.surface_cloud(200_000, seed=11, noise=0.01)
    q = ref.surface_cloud(50_000, seed=12, noise=0.05)
    q[:5000, 2] += np.random.default_rng(13).uniform(0.02, 2.0, 5000).astype(F32)          # many beyond max_dist
    q[5000:5100] = t[:100]          # on a target
    gd, gi = _check_nearest(q, t, 0.1, "surface")
    assert (gi < 0).sum() > 1000 and np.all(gd[5000:5100] == 0)
    _check_nearest(q, t, 10.0, "surface, max_dist beyond the cloud")
    _check_nearest(q, t, 1e-3, "surface, max_dist below the spacing")
    _check_nearest(q + F32(4096.0), t + F32(4096.0), 0.1, "far from the origin")
    _check_nearest(q[:2000], t[:1], 0.5, "one target")
    _check_nearest(q[:2000], t[:9], 5.0, "nine targets")


def test_nearest_ties_go_to_the_smallest_index():
    g = np.stack(np.meshgrid(np.arange(24), np.arange(24), np.arange(24), indexing="ij"), -1).reshape(-1, 3).astype(F32)
    t = np.concatenate([g, g[::5]])[np.random.default_rng(14).permutation(len(g) + len(g[::5]))]          # a lattice with duplicates, shuffled
    rng = np.random.default_rng(15)
    q = np.concatenate([rng.integers(0, 23, (4000, 3)) + 0.5,          # cell centres: eight equidistant corners (and their duplicates)
                        rng.integers(0, 23, (2000, 3)) + np.array([0.5, 0.0, 0.0]),          # edge midpoints
                        rng.integers(0, 24, (2000, 3))]).astype(F32)          # on a lattice point
    gd, gi = _check_nearest(q, t, 2.0, "lattice ties")
    d2 = ref.d2_f32(q[:300, None], t[None])
    assert np.array_equal(gi[:300], np.argmin(d2, axis=1)) and np.all((d2 == d2.min(1, keepdims=True)).sum(1) >= 8)
    # max_dist exactly at the tie distance: d2 = 0.75 is not below 0.75
    _check_nearest(q[:4000], t, float(np.sqrt(0.75)), "cut-off at the tie distance")


def test_nearest_edges():
    q = _t(ref.surface_cloud(1000, 1))
    r = mesh_eval.nearest(q, torch.zeros(0, 3, device="cuda"), 1.0)
    assert torch.all(torch.isinf(r.dist)) and torch.all(r.index == -1) and r.dist.shape == (1000,)
    r = mesh_eval.nearest(torch.zeros(0, 3, device="cuda"), q, 1.0)
    assert r.dist.shape == (0,) and r.index.dtype == torch.int32
    r = mesh_eval.nearest(q, q, 0.0)          # nothing is nearer than 0
    assert torch.all(r.index == -1)
    bad = q.clone()
    bad[5, 0] = float("inf")
    for a, b in ((bad, q), (q, bad)):
        with pytest.raises(ValueError, match="non-finite"):
            mesh_eval.nearest(a, b, 1.0)


def test_nearest_does_not_wait_before_its_read_back():
    q, t = _t(ref.surface_cloud(20_000, 1)), _t(ref.surface_cloud(50_000, 2))
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    mesh_eval._nearest_async(q, t, 0.1, state)          # warm-up: the allocator has its blocks, the library is loaded
    torch.cuda.synchronize()
    a = torch.randn(8192, 8192, device="cuda")
    (a @ a).sum().item()
    hold = torch.cuda.Event()
    for _ in range(40):          # some hundred milliseconds of the stream, queued in well under one
        a @ a
    hold.record()
    dist, index = mesh_eval._nearest_async(q, t, 0.1, state)          # everything `nearest` does before its one read-back
    still_running = not hold.query()
    torch.cuda.synchronize()
    assert still_running, "nearest waited for the device before its read-back"
    want = mesh_eval.nearest(q, t, 0.1)
    assert torch.equal(dist, want.dist) and torch.equal(index, want.index)


def test_far_queries_cost_no_more_than_near_ones():
    n_side, Q = 1500, 200_000
    s = 1.0 / n_side          # spacing of the planar target; max_dist = 100 spacings, DTU's ratio
    rng = np.random.default_rng(16)
    g = (np.stack(np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-0.3, 0.3, (n_side * n_side, 2))) * s
    t = _t(np.concatenate([g, np.zeros((len(g), 1))], 1).astype(F32)[rng.permutation(len(g))])
    md = 100 * s
    xy = rng.uniform(0, 1, (Q, 2))
    near = _t(np.concatenate([xy, rng.uniform(-2 * s, 2 * s, (Q, 1))], 1).astype(F32))
    far = _t(np.concatenate([xy, rng.uniform(0.5 * md, 2.0 * md, (Q, 1)) * rng.choice([-1, 1], (Q, 1))], 1).astype(F32))
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    index = mesh_eval._Index(t, state)
    ms_near = _ms(lambda: index.query(near, md))
    ms_far = _ms(lambda: index.query(far, md))
    d_far, i_far = index.query(far, md)
    z = far[:, 2].abs()
    assert torch.all(i_far[z >= md * 1.001] == -1) and torch.all(i_far[z <= md * 0.99] >= 0)
    assert torch.all((d_far[z <= md * 0.99] >= z[z <= md * 0.99] * (1 - 1e-6)))
    assert state.cpu().tolist()[:4] == [0, 0, 0, 0]
    print("\n[far queries] N %d, Q %d, max_dist = 100 spacings: near %.3f ms, between 0.5 and 2 max_dist away %.3f ms, ratio %.2f" % (len(g), Q, ms_near, ms_far, ms_far / ms_near))
    assert ms_far / ms_near < 1e3


# ---- the metrics --------------------------------------------------------------------------------------------------------------------------------------
def test_chamfer_and_fscore_against_the_restatement():
    pred = ref.surface_cloud(40_000, seed=21, noise=0.01)
    gt = ref.surface_cloud(70_000, seed=22, noise=0.002)
    pred[:3000, 2] += 1.5          # outliers beyond max_dist
    rng = np.random.default_rng(23)
    pm, gm = rng.uniform(size=len(pred)) < 0.7, gt[:, 0] > -0.5
    for kw in (dict(), dict(pred_query_mask=pm, gt_query_mask=gm)):
        want = ref.chamfer(pred, gt, 0.3, **kw)
        got = mesh_eval.chamfer(_t(pred), _t(gt), 0.3, **{k: _t(v) for k, v in kw.items()})
        assert (got.n_d2s, got.n_s2d) == (want["n_d2s"], want["n_s2d"]) and got.n_d2s < got.n_pred_queries
        for a, b, n in ((got.mean_d2s, want["mean_d2s"], got.n_d2s), (got.mean_s2d, want["mean_s2d"], got.n_s2d)):
            assert abs(a - b) <= (n + 16) * 2.0 ** -52 * abs(b), (a, b)          # the order of an f64 sum of n non-negative terms
        assert got.overall == (got.mean_d2s + got.mean_s2d) / 2
        print("\n[chamfer] d2s %.9g (%d) s2d %.9g (%d) overall %.9g" % (got.mean_d2s, got.n_d2s, got.mean_s2d, got.n_s2d, got.overall))
    for tau in (0.004, 0.02):
        want = ref.fscore(pred, gt, tau)
        got = mesh_eval.fscore(_t(pred), _t(gt), tau)
        assert (got.n_precision, got.n_recall, got.n_pred, got.n_gt) == (want["n_precision"], want["n_recall"], len(pred), len(gt))
        assert (got.precision, got.recall, got.fscore) == (want["precision"], want["recall"], want["fscore"])
        print("[fscore] tau %g: precision %.6f recall %.6f F %.6f" % (tau, got.precision, got.recall, got.fscore))
    assert 0 < got.precision < 1 and 0 < got.recall <= 1
    # empty selections and empty sets
    none = torch.zeros(len(pred), dtype=torch.bool, device="cuda")
    c = mesh_eval.chamfer(_t(pred), _t(gt), 0.3, pred_query_mask=none)
    assert np.isnan(c.mean_d2s) and c.n_d2s == 0 and c.n_pred_queries == 0 and c.n_s2d > 0 and np.isnan(c.overall)
    c = mesh_eval.chamfer(torch.zeros(0, 3, device="cuda"), _t(gt), 0.3)
    assert np.isnan(c.mean_d2s) and np.isnan(c.mean_s2d) and (c.n_d2s, c.n_s2d) == (0, 0)
    f = mesh_eval.fscore(torch.zeros(0, 3, device="cuda"), _t(gt), 0.1)
    assert (f.precision, f.recall, f.fscore) == (0.0, 0.0, 0.0)
    f = mesh_eval.fscore(_t(pred + F32(50.0)), _t(gt), 0.1)          # nothing within tau: 0 / 0 is 0
    assert (f.precision, f.recall, f.fscore) == (0.0, 0.0, 0.0)


# ---- closed form, independent of the restatement ------------------------------------------------------------------------------------------------------
def _fibonacci_sphere(n, radius):
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    phi = np.pi * (1 + 5 ** 0.5) * k
    rho = np.sqrt(1 - z * z)
    return (radius * np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)).astype(F32)


def test_fused_sphere_against_its_analytic_surface():
    VOX, R = 0.02, 0.5
    vol = tsdf.TSDFVolume(VOX, 4 * VOX, block_capacity=1 << 13)
    for dep, col, M, k in mesh_ref.floater_frames():
        vol.integrate(_t(dep), *k, M, color=_t(col))
    raw = vol.extract_mesh()
    post = mesh.post_process_mesh(raw, 1)
    n_gt = 400_000
    gt = _t(_fibonacci_sphere(n_gt, R))
    # s: no point of the sphere is farther than s from a sample.  Each sample owns 4 pi R^2 / n of the sphere; the Fibonacci lattice's cells are near-square, of
    # side sqrt(4 pi R^2 / n), so the covering radius is about 0.71 of that side; s = one full side leaves 40 % of margin.
    s = float(np.sqrt(4 * np.pi * R * R / n_gt))
    density, max_dist = 0.01, 1.0
    cloud = mesh_eval.sample_surface(post, density)
    thinned = cloud[mesh_eval.downsample(cloud, density, order=torch.randperm(len(cloud), device="cuda"))]
    d = mesh_eval.nearest(thinned, gt, max_dist).dist.cpu().numpy().astype(np.float64)
    off = np.abs(np.linalg.norm(thinned.cpu().numpy().astype(np.float64), axis=1) - R)
    print("\n[sphere] post mesh F %d -> %d sampled, %d thinned; | |p| - R | max %.5f, d - | |p| - R | in [%.2e, %.2e], s = %.2e"
          % (len(post.faces), len(cloud), len(thinned), off.max(), (d - off).min(), (d - off).max(), s))
    assert np.all(d >= off - 1e-6) and np.all(d <= off + s)
    e_post = mesh_eval.evaluate_mesh(post, gt, density=density, max_dist=max_dist, tau=2 * VOX)
    e_raw = mesh_eval.evaluate_mesh(raw, gt, density=density, max_dist=max_dist, tau=2 * VOX)
    print("[sphere] post %s\n[sphere] raw  %s" % (e_post, e_raw))
    assert e_post["n_d2s"] == e_post["n_thinned"] and e_post["n_s2d"] == n_gt
    assert e_post["mean_d2s"] <= 0.52 * VOX + s and e_post["mean_s2d"] <= 0.52 * VOX + 2 * density          # the surface is within 0.52 voxels (tests/test_gpu_mesh.py)
    assert e_raw["mean_d2s"] > 2 * e_post["mean_d2s"] and e_raw["n_thinned"] > e_post["n_thinned"]          # the floaters sit 0.1 .. 0.4 off the sphere
    assert e_raw["mean_s2d"] <= 0.52 * VOX + 2 * density
    assert e_post["precision"] == 1.0 and e_post["recall"] == 1.0 and e_raw["precision"] < 0.99 and e_raw["recall"] == 1.0
    again = mesh_eval.evaluate_mesh(post, gt, density=density, max_dist=max_dist, tau=2 * VOX)
    assert again["n_thinned"] == e_post["n_thinned"] and again["n_d2s"] == e_post["n_d2s"]          # the seeded order: the same cloud
    other = mesh_eval.evaluate_mesh(post, gt, density=density, max_dist=max_dist, seed=1, pred_query_filter=lambda p: p[:, 2] > 0,
                                    gt_query_mask=gt[:, 2] > 0)
    assert 0.4 * e_post["n_thinned"] < other["n_d2s"] < 0.6 * e_post["n_thinned"] and other["n_s2d"] == int((gt[:, 2] > 0).sum())


# ---- scale --------------------------------------------------------------------------------------------------------------------------------------------
def test_scale():
    sizes = [(10 + k % 37, 12 + (7 * k) % 41) for k in range(1200)]
    h = 0.01
    v, f = mesh_ref.join([mesh_ref.grid(n, m, h, origin=(float(k % 40), float(k // 40), 0.0)) for k, (n, m) in enumerate(sizes)])
    v, f = mesh_ref.permute(v, f, seed=31)
    assert len(f) >= 1_900_000
    rng = np.random.default_rng(32)
    per = 2_200_000 // len(sizes) + 1
    gt = np.concatenate([np.concatenate([rng.uniform(0, 1, (per, 2)) * [(n - 1) * h, (m - 1) * h] + [k % 40, k // 40], np.zeros((per, 1))], 1)
                         for k, (n, m) in enumerate(sizes)]).astype(F32)
    assert len(gt) >= 2_000_000
    m, g = _mesh(v, f), _t(gt)
    density = 0.004
    t0 = time.perf_counter()
    e = mesh_eval.evaluate_mesh(m, g, density=density, max_dist=100 * density, tau=2 * density)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("\n[scale] F %d, gt %d, max_dist / density 100: evaluate_mesh %.3f s; %s" % (len(f), len(gt), dt, e))
    assert e["n_sampled"] > len(v) and len(v) // 4 < e["n_thinned"] < e["n_sampled"]
    assert e["n_d2s"] == e["n_thinned"] and e["n_s2d"] == len(gt)          # both clouds cover the same rectangles: nothing is beyond max_dist
    # a gt point is within one thinning radius of a kept point (maximality), up to the rectangles' rims; a kept point within a few gt spacings
    gt_spacing = h * np.sqrt(np.mean([(a - 1) * (b - 1) for a, b in sizes]) / per)
    assert e["mean_s2d"] <= 1.05 * density and e["mean_d2s"] <= 3 * gt_spacing and e["mean_d2s"] > 0
    # tau = 2 density: a gt point is within density + the sample spacing of a kept point; a kept point misses every gt point within tau with
    # probability exp(-pi (tau / gt spacing)^2) = 1.3 %
    assert e["recall"] > 0.99 and e["precision"] > 0.9
    assert dt < 120


# ---- contract edges -----------------------------------------------------------------------------------------------------------------------------------
def test_on_a_non_default_stream():
    v, f = ref.random_mesh(500, seed=41, scale=0.3, extent=1.0)
    gt = ref.surface_cloud(30_000, seed=42)
    m, g = _mesh(v, f), _t(gt)
    want_cloud = mesh_eval.sample_surface(m, 0.03)
    want_keep = mesh_eval.downsample(want_cloud, 0.03)
    want_nn = mesh_eval.nearest(want_cloud, g, 0.5)
    want_c = mesh_eval.chamfer(want_cloud, g, 0.5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cloud = mesh_eval.sample_surface(m, 0.03)
        keep = mesh_eval.downsample(cloud, 0.03)
        nn = mesh_eval.nearest(cloud, g, 0.5)
        c = mesh_eval.chamfer(cloud, g, 0.5)
        e = mesh_eval.evaluate_mesh(m, g, density=0.03, max_dist=0.5, tau=0.05)
    side.synchronize()
    assert torch.equal(cloud, want_cloud) and torch.equal(keep, want_keep) and torch.equal(nn.dist, want_nn.dist) and torch.equal(nn.index, want_nn.index)
    assert (c.n_d2s, c.n_s2d) == (want_c.n_d2s, want_c.n_s2d) and abs(c.mean_d2s - want_c.mean_d2s) <= 1e-12 * want_c.mean_d2s
    e2 = mesh_eval.evaluate_mesh(m, g, density=0.03, max_dist=0.5, tau=0.05)
    assert all(e[k] == e2[k] for k in ("n_d2s", "n_s2d", "n_sampled", "n_thinned", "precision", "recall", "fscore")) and e["n_sampled"] == len(cloud)
    assert abs(e["overall"] - e2["overall"]) <= 1e-12 * e2["overall"]


def test_non_contiguous_inputs():
    base = _t(np.concatenate([ref.surface_cloud(5000, 43), np.zeros((5000, 1), F32)], 1))
    p = base[:, :3]
    assert not p.is_contiguous()
    a = mesh_eval.nearest(p, p.contiguous()[::2], 0.2)
    b = mesh_eval.nearest(p.contiguous(), p.contiguous()[::2].contiguous(), 0.2)
    assert torch.equal(a.dist, b.dist) and torch.equal(a.index, b.index)
    assert torch.equal(mesh_eval.downsample(p, 0.05), mesh_eval.downsample(p.contiguous(), 0.05))
