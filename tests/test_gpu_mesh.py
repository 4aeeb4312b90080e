"""Mesh post-processing on the MI355X (ibgs_amd/mesh.py, csrc/mesh.hip) against the host restatement of its contract (tests/mesh_ref.py: numpy + scipy).
Integers are compared with assert_array_equal, the floats of an output mesh bit for bit with the input rows the restatement selects (they are copies);
the one tolerance is the cluster areas' (an f64 sum in another order).

  1  synthetic, adversarial indexing: disjoint grids, a three-triangle edge, degenerate triangles, an unreferenced vertex, everything permuted
  2  fused floaters: the analytic sphere + four small spheres through TSDFVolume -> extract_mesh -> post_process_mesh
  3  depth of the union forest: (a) a strip of 1 M triangles, whole and cut into 1000 pieces; (b) a fan of 200 000 triangles + 1000 that touch it at the
     apex only, timed against (a): a walk quadratic in a vertex's degree would be > 10^4 x off
  4  scale: 1.9 M faces in 1100 clusters
  5  determinism: cases 1 and 3a three times, byte-identical
  6  areas: relative error per cluster <= (n + 16) 2^-52, n = the cluster's triangles (two f64 sums of n non-negative terms in different orders differ by at
     most (n - 1) 2^-52 relative; the rest covers the roundings inside one triangle's area), checked in every comparison; closed forms in case 1
  7  edges of the contract: empty, one triangle, all degenerate, out-of-range indices (raise; the kernels bounds-check), inputs untouched, another stream"""
import numpy as np
import pytest
import torch

from ibgs_amd import mesh, tsdf
from tests import mesh_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _dev(v, f, c=None, n=None):
    if c is None:
        c, n = ref.attributes(v)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return tsdf.TriangleMesh(t(v), t(f), t(c), t(n))


def _np(m):
    return tuple(x.cpu().numpy() for x in (m.vertices, m.faces, m.colors, m.normals))


def _assert_areas(got, want, counts, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bound = (np.asarray(counts, np.float64) + 16) * EPS * np.abs(want)
    rel = err / np.maximum(np.abs(want), 1e-300)
    print("[areas %s] %d clusters, max relative error %.3e (worst cluster allows %.3e)" % (what, len(want), rel.max() if len(rel) else 0.0,
                                                                                       ((np.asarray(counts) + 16) * EPS).max() if len(rel) else 0.0))
    assert np.all(err <= bound)


def _check_clusters(m, v, f, what=""):
    got = mesh.cluster_connected_triangles(m)
    lab, counts, areas = ref.cluster(v, f)
    assert got.triangle_clusters.dtype == torch.int32 and got.cluster_n_triangles.dtype == torch.int32 and got.cluster_area.dtype == torch.float64
    np.testing.assert_array_equal(got.triangle_clusters.cpu().numpy(), lab)
    np.testing.assert_array_equal(got.cluster_n_triangles.cpu().numpy(), counts)
    _assert_areas(got.cluster_area.cpu().numpy(), areas, counts, what)
    return got, lab, counts, areas


def _check_post(m, arrays, lab, counts, k, min_triangles=50):
    v, f, c, n = arrays
    out = _np(mesh.post_process_mesh(m, k, min_triangles))
    rows, fo = ref.post_process(f, len(v), lab, counts, k, min_triangles)
    np.testing.assert_array_equal(out[1], fo)
    assert out[1].dtype == np.int32 and out[1].shape == (len(fo), 3)
    for a, src, name in ((out[0], v, "vertices"), (out[2], c, "colours"), (out[3], n, "normals")):
        assert a.dtype == np.float32 and a.shape == (len(rows), 3), name
        assert a.tobytes() == src[rows].tobytes(), name
    return out


def _check_clean(m, arrays, lab, counts, min_len):
    out = mesh.clean_mesh(m, min_len)
    np.testing.assert_array_equal(out.faces.cpu().numpy(), ref.clean(arrays[1], lab, counts, min_len))
    for a, src in zip((out.vertices, out.colors, out.normals), (arrays[0], arrays[2], arrays[3])):
        assert a.cpu().numpy().tobytes() == src.tobytes()          # vertices left as they are
    return out


def _untouched(m, arrays):
    for a, b in zip(_np(m), arrays):
        assert a.tobytes() == b.tobytes()


def _time_clustering(m, reps=3):
    mesh.cluster_connected_triangles(m)          # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); mesh.cluster_connected_triangles(m); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------------------

def test_synthetic_adversarial_indexing():
    v, f = ref.case1()
    c, n = ref.attributes(v)
    arrays = (v, f, c, n)
    m = _dev(*arrays)
    got, lab, counts, areas = _check_clusters(m, v, f, "case 1")
    assert len(counts) == 11 and sorted(counts.tolist(), reverse=True) == ref.CASE1_COUNTS
    # closed forms: a pure grid cluster of n triangles covers n / 2 squares of side h; the big grid carries its third-triangle-on-an-edge; the degenerate
    # pair has no area
    uv, uf = ref.case1(permuted=False)
    extra = float(ref.triangle_areas(uv, uf[-3:-2])[0])
    closed = np.array([cnt / 2 * ref.CASE1_H ** 2 for cnt in counts.tolist()])
    closed[np.argmax(counts)] = (counts.max() - 1) / 2 * ref.CASE1_H ** 2 + extra
    degenerate_pair = lab[np.flatnonzero((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]))]
    assert len(degenerate_pair) == 2 and degenerate_pair[0] == degenerate_pair[1] and counts[degenerate_pair[0]] == 2
    closed[degenerate_pair[0]] = 0.0
    _assert_areas(got.cluster_area.cpu().numpy(), closed, counts, "case 1, closed forms")
    for k in range(1, 12):
        out = _check_post(m, arrays, lab, counts, k)
        print("[case 1] cluster_to_keep %2d: V' %d F' %d" % (k, len(out[0]), len(out[1])))
        assert len(out[1]) == ref.CASE1_KEPT[min(k, 5)]
    with pytest.raises(ValueError, match="cluster"):
        mesh.post_process_mesh(m, 12)
    # the order of the removals: the degenerate pair survives the cluster filter at min_triangles = 1, keeps p, q, r alive and is then removed itself
    out = _check_post(m, arrays, lab, counts, 11, min_triangles=1)
    assert len(out[1]) == len(f) - 2 and len(out[0]) == len(v) - 1 and len(np.unique(out[1])) == len(out[0]) - 3
    assert len(_check_clean(m, arrays, lab, counts, 45).faces) == 9323 + 2 * 3042 + 522 + 50
    assert len(_check_clean(m, arrays, lab, counts, 1000).faces) == 9323 + 2 * 3042
    _untouched(m, arrays)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------------------

def _manifold_stats(f, V):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * V + e[:, 1]
    rkey = e[:, 1] * V + e[:, 0]
    _, cnt = np.unique(key, return_counts=True)
    return bool(np.all(cnt == 1)), bool(np.all(np.isin(rkey, key))), len(np.unique(np.minimum(key, rkey)))


def test_fused_floaters():
    VOX, R_S = 0.02, 0.5
    vol = tsdf.TSDFVolume(VOX, 4 * VOX, block_capacity=1 << 13)
    for dep, col, M, k in ref.floater_frames():
        vol.integrate(torch.as_tensor(dep, device="cuda"), *k, M, color=torch.as_tensor(col, device="cuda"))
    vol.check()
    raw = vol.extract_mesh()
    assert vol.mesh_overruns() == 0
    arrays = _np(raw)
    v, f = arrays[0], arrays[1]
    got, lab, counts, _ = _check_clusters(raw, v, f, "floaters")
    print("\n[floaters] V %d F %d, clusters %s" % (len(v), len(f), sorted(counts.tolist(), reverse=True)))
    assert len(counts) >= 5          # something to remove
    for k in range(1, len(counts) + 1):
        _check_post(raw, arrays, lab, counts, k)
    ov, of, oc, on = _check_post(raw, arrays, lab, counts, 1)
    once, paired, E = _manifold_stats(of, len(ov))
    assert once and paired                                 # every edge in exactly two faces, in opposite directions
    assert len(np.unique(of)) == len(ov)                   # every vertex referenced
    chi = len(ov) - E + len(of)
    d = np.abs(np.linalg.norm(ov.astype(np.float64), axis=1) - R_S) / VOX
    print("[floaters] cluster_to_keep 1: V' %d F' %d chi %d, | |x| - r | / v max %.4f" % (len(ov), len(of), chi, d.max()))
    assert chi == 2 and d.max() <= 0.52
    assert len(of) == counts.max()
    last = _check_post(raw, arrays, lab, counts, len(counts))          # the floor of 50: only the fragments under it go
    assert len(last[1]) == int(counts[counts >= 50].sum()) < len(f)
    _untouched(raw, arrays)


def test_both_mesh_files_of_render_geo_from_one_volume(tmp_path):
    """The recipe of ibgs_amd/tsdf.py's docstring: tsdf_fusion.ply and tsdf_fusion_post.ply."""
    from ibgs_amd import ply
    vol = tsdf.TSDFVolume(0.02, 0.08, block_capacity=1 << 13)
    for dep, col, M, k in ref.floater_frames(n_views=12):
        vol.integrate(torch.as_tensor(dep, device="cuda"), *k, M, color=torch.as_tensor(col, device="cuda"))
    raw = vol.extract_mesh()
    path, path_post = str(tmp_path / "tsdf_fusion.ply"), str(tmp_path / "tsdf_fusion_post.ply")
    ply.save_mesh(path, raw)
    ply.save_mesh(path_post, mesh.post_process_mesh(raw, 1))
    a, b = ply.load_mesh(path), ply.load_mesh(path_post)
    v, f = raw.vertices.cpu().numpy(), raw.faces.cpu().numpy()
    lab, counts, _ = ref.cluster(v, f)
    rows, fo = ref.post_process(f, len(v), lab, counts, 1)
    np.testing.assert_array_equal(a["faces"], f)
    np.testing.assert_array_equal(b["faces"], fo)
    assert b["vertices"].tobytes() == v[rows].tobytes() and 0 < len(fo) < len(f)
    np.testing.assert_array_equal(b["colors"], a["colors"][rows])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------------------

def test_union_forest_depth_and_high_degree_vertex():
    N = 1_000_000
    v, f = ref.permute(*ref.strip(N), seed=21)
    m = _dev(v, f)
    got = mesh.cluster_connected_triangles(m)
    assert got.cluster_n_triangles.cpu().tolist() == [N]
    assert int(got.triangle_clusters.abs().max()) == 0
    _assert_areas(got.cluster_area.cpu().numpy(), ref.triangle_areas(v, f).sum(keepdims=True), [N], "strip")
    ms_a = _time_clustering(m)

    cv, cf, lengths = ref.cut_strip(N, 1000, seed=22)
    cv, cf = ref.permute(cv, cf, seed=23)
    cm = _dev(cv, cf)
    cgot, lab, counts, _ = _check_clusters(cm, cv, cf, "cut strip")
    assert len(counts) == 1000 and sorted(counts.tolist()) == sorted(lengths.tolist()) and len(set(lengths.tolist())) > 500
    arrays = (cv, cf) + ref.attributes(cv)
    cm = _dev(*arrays)
    _check_post(cm, arrays, lab, counts, 300)

    # (b) the apex has the lowest index and degree 201 000
    fv, ff = ref.fan(200_000, 1000)
    rng = np.random.default_rng(24)
    ff = ff[rng.permutation(len(ff))]
    fm = _dev(fv, ff)
    fgot, flab, fcounts, _ = _check_clusters(fm, fv, ff, "fan")
    assert sorted(fcounts.tolist(), reverse=True) == [200_000] + [1] * 1000
    ms_b = _time_clustering(fm)
    print("\n[forest] clustering: strip of %d triangles %.3f ms; fan of 200 000 + 1000 loose triangles %.3f ms (ratio %.3f)" % (N, ms_a, ms_b, ms_b / ms_a))
    assert ms_b < 10 * ms_a


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------------------

def test_scale():
    sizes = [(10 + k % 37, 12 + (7 * k) % 41) for k in range(1100)]
    v, f = ref.join([ref.grid(n, m, 0.01, origin=(float(k % 40), float(k // 40), 0.0)) for k, (n, m) in enumerate(sizes)])
    v, f = ref.permute(v, f, seed=31)
    c, n = ref.attributes(v)
    arrays = (v, f, c, n)
    m = _dev(*arrays)
    got, lab, counts, _ = _check_clusters(m, v, f, "scale")
    print("\n[scale] V %d F %d clusters %d" % (len(v), len(f), len(counts)))
    assert len(f) >= 1_000_000 and len(counts) == 1100
    assert sorted(counts.tolist()) == sorted(2 * (a - 1) * (b - 1) for a, b in sizes)
    for k in (1, 137, 1100):
        _check_post(m, arrays, lab, counts, k)
    _check_post(m, arrays, lab, counts, 1100, min_triangles=1)
    _check_clean(m, arrays, lab, counts, 1000)
    _untouched(m, arrays)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------------------

def _everything(m, ks):
    g = mesh.cluster_connected_triangles(m)
    out = [g.triangle_clusters.cpu().numpy().tobytes(), g.cluster_n_triangles.cpu().numpy().tobytes()]
    for k in ks:
        out += [a.tobytes() for a in _np(mesh.post_process_mesh(m, k))]
    out += [a.tobytes() for a in _np(mesh.clean_mesh(m, 45))]
    return out


@pytest.mark.parametrize("case", ["case1", "strip"])
def test_bit_identical_from_run_to_run(case):
    if case == "case1":
        m, ks = _dev(*ref.case1()), (1, 2, 4, 7)
    else:
        m, ks = _dev(*ref.permute(*ref.strip(1_000_000), seed=21)), (1,)
    runs = [_everything(m, ks) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------------------

def test_empty_mesh():
    for V in (0, 5):
        v, f = np.zeros((V, 3), np.float32), np.zeros((0, 3), np.int32)
        m = _dev(v, f)
        g = mesh.cluster_connected_triangles(m)
        assert g.triangle_clusters.shape == (0,) and g.cluster_n_triangles.shape == (0,) and g.cluster_area.shape == (0,)
        assert g.cluster_area.dtype == torch.float64 and g.triangle_clusters.is_cuda
        out = mesh.post_process_mesh(m)
        assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.colors.shape) == (0, 3) and out.faces.dtype == torch.int32
        out = mesh.clean_mesh(m)
        assert tuple(out.vertices.shape) == (V, 3) and tuple(out.faces.shape) == (0, 3)


def test_one_triangle_and_all_degenerate():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5]], np.float32)
    f = np.array([[2, 0, 1]], np.int32)
    arrays = (v, f) + ref.attributes(v)
    m = _dev(*arrays)
    got, lab, counts, areas = _check_clusters(m, v, f, "one triangle")
    assert counts.tolist() == [1] and got.cluster_area.cpu().tolist() == [1.0]
    assert len(_check_post(m, arrays, lab, counts, 1)[1]) == 0                     # under the floor of 50
    out = _check_post(m, arrays, lab, counts, 1, min_triangles=1)
    assert out[1].tolist() == [[2, 0, 1]] and len(out[0]) == 3
    with pytest.raises(ValueError):
        mesh.post_process_mesh(m, 2)
    # all degenerate: (i, i, i + 1) and (i + 1, i, i + 1) share {i, i + 1}, the latter meets (i + 1, i + 1, i + 2) in {i + 1, i + 1}: one chain of 400;
    # 200 triangles (j, j, j) whose only edge {j, j} nobody shares: 200 clusters of one
    k = np.arange(200)
    f = np.concatenate([np.stack([k, k, k + 1], 1), np.stack([k + 1, k, k + 1], 1), np.stack([k + 300, k + 300, k + 300], 1)]).astype(np.int32)
    v = np.random.default_rng(1).normal(size=(600, 3)).astype(np.float32)
    f = f[np.random.default_rng(2).permutation(len(f))]
    arrays = (v, f) + ref.attributes(v)
    m = _dev(*arrays)
    got, lab, counts, areas = _check_clusters(m, v, f, "degenerate")
    assert sorted(counts.tolist(), reverse=True) == [400] + [1] * 200
    assert np.all(areas == 0) and got.cluster_area.abs().max().item() == 0
    for kk, mt in ((1, 50), (1, 1), (len(counts), 1)):
        out = _check_post(m, arrays, lab, counts, kk, mt)
        assert len(out[1]) == 0
    assert len(_check_post(m, arrays, lab, counts, len(counts), 1)[0]) == 401          # every referenced vertex stays, no face does
    _check_clean(m, arrays, lab, counts, 2)
    _untouched(m, arrays)


@pytest.mark.parametrize("bad", [1681, -1, 2 ** 31 - 1, -2 ** 31])
def test_out_of_range_face_index_raises(bad):
    v, f = ref.grid(41, 41, 0.1)          # 1681 vertices
    f = f.copy(); f[777, 1] = bad
    arrays = (v, f) + ref.attributes(v)
    m = _dev(*arrays)
    for fn in (mesh.cluster_connected_triangles, mesh.post_process_mesh, mesh.clean_mesh):
        with pytest.raises(mesh.MeshError, match="1 triangle"):
            fn(m)
    _untouched(m, arrays)


def test_on_a_non_default_stream():
    v, f = ref.case1()
    arrays = (v, f) + ref.attributes(v)
    m = _dev(*arrays)
    lab, counts, _ = ref.cluster(v, f)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = mesh.cluster_connected_triangles(m)
        out = mesh.post_process_mesh(m, 4)
    s.synchronize()
    np.testing.assert_array_equal(g.triangle_clusters.cpu().numpy(), lab)
    rows, fo = ref.post_process(f, len(v), lab, counts, 4)
    np.testing.assert_array_equal(out.faces.cpu().numpy(), fo)
    assert out.vertices.cpu().numpy().tobytes() == v[rows].tobytes()


def test_non_contiguous_inputs():
    v, f = ref.case1()
    c, n = ref.attributes(v)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    wide = lambda a: t(np.concatenate([a, a], 1))[:, :3]          # a strided view
    m = tsdf.TriangleMesh(wide(v), wide(f), wide(c), wide(n))
    assert not m.vertices.is_contiguous()
    lab, counts, _ = ref.cluster(v, f)
    _check_post(m, (v, f, c, n), lab, counts, 2)
