"""TSDF fusion and marching cubes on the MI355X (ibgs_amd/tsdf.py, csrc/tsdf.hip) against the numpy restatement of the contract (tests/tsdf_ref.py),
closed forms and the analytic surface scene.

  (a) integration parity on analytic depth maps (a sphere from 24 Fibonacci directions, a fronto-parallel plane from 5 views): allocated blocks,
      weights exact, tsdf / colour to 1e-6 (voxels whose pixel flips on a half-pixel tie may differ: at most 1e-4 of them)
  (b) the plane's closed form along the optical axis
  (c) the mesh against the restatement's marching cubes on the GPU's own volume: same V / F, faces identical in order
  (d) the sphere's mesh: a closed oriented 2-manifold of Euler characteristic 2 near the sphere, normals outward
  (e) bit-identical meshes twice, and with two hash capacities (different slot positions)
  (f) end to end: surface_discs rendered by renderer.render from 16 views, depth_for_fusion, integrate_view, extract_mesh
  (g) errors before any GPU work, capacity overflow and reset(), no host wait in integrate"""
import ctypes
import time

import numpy as np
import pytest
import torch

from ibgs_amd import _lib, tsdf
from tests import tsdf_ref as ref

pytestmark = pytest.mark.gpu

W, H, FX, CX, CY = 160, 120, 140.0, 80.0, 60.0
R_S, DIST, VOX = 0.5, 2.0, 0.02
TAU = 4 * VOX


def _table():
    out = (ctypes.c_int32 * 4096)()
    assert _lib.load().ibgs_tsdf_mc_table(out) == 0
    return np.array(out)


def _sphere_frames(n=24):
    frames = []
    for d in ref.fibonacci_directions(n):
        M = ref.look_at(DIST * d)
        dep, col = ref.sphere_view(M, W, H, FX, FX, CX, CY, R_S)
        frames.append((dep, col, M, (FX, FX, CX, CY)))
    return frames


def _plane_frames():
    p = ref.PLANE
    rng = np.random.default_rng(4)
    return [(d, rng.uniform(0, 1, (3, p["H"], p["W"])).astype(np.float32), M, (p["fx"], p["fy"], p["cx"], p["cy"])) for d, M in ref.plane_views()]


SCENES = {"sphere": (_sphere_frames, VOX), "plane": (_plane_frames, ref.PLANE["voxel"])}


def _gpu_volume(frames, voxel, cap=1 << 13):
    vol = tsdf.TSDFVolume(voxel, 4 * voxel, block_capacity=cap)
    for dep, col, M, k in frames:
        vol.integrate(torch.as_tensor(dep, device="cuda"), *k, M, color=torch.as_tensor(col, device="cuda"))
    return vol


def _ref_volume(frames, voxel):
    vol = ref.RefVolume(voxel, 4 * voxel)
    for dep, col, M, k in frames:
        vol.integrate(dep, *k, M, color=col)
    return vol


def _mesh_np(m):
    return tuple(x.cpu().numpy() for x in (m.vertices, m.faces, m.colors, m.normals))


@pytest.mark.parametrize("scene", ["sphere", "plane"])
def test_integration_parity(scene):
    make, voxel = SCENES[scene]
    frames = make()
    g = _gpu_volume(frames, voxel)
    g.check()
    r = _ref_volume(frames, voxel)
    gb, rb = g.blocks(), r.blocks()
    only_g, only_r = np.setdiff1d(gb["keys"], rb["keys"]), np.setdiff1d(rb["keys"], gb["keys"])
    print("\n[%s] blocks %d (restatement %d), only GPU %d, only restatement %d" % (scene, len(gb["keys"]), len(rb["keys"]), len(only_g), len(only_r)))
    assert len(only_g) == 0 and len(only_r) == 0          # (a cube test decided by a rounding tie could differ: none expected, none seen)
    assert g.ignored_points() == r.ignored == 0
    np.testing.assert_array_equal(gb["coords"], rb["coords"])
    np.testing.assert_array_equal(gb["weight"], rb["weight"])
    dt = np.abs(gb["tsdf"] - rb["tsdf"]); dc = np.abs(gb["color"] - rb["color"]).max(-1)
    off = (dt > 1e-6) | (dc > 1e-6)
    print("[%s] voxels %d, weighted %d, tsdf max diff %.2e, colour max diff %.2e, voxels beyond 1e-6: %d"
          % (scene, dt.size, int((gb["weight"] > 0).sum()), dt.max(), dc.max(), int(off.sum())))
    assert off.mean() <= 1e-4
    assert (gb["weight"] > 0).sum() > 10000


def test_plane_closed_form_on_the_optical_axis():
    p = ref.PLANE
    g = _gpu_volume(_plane_frames(), p["voxel"])
    t, w, X = ref.axis_voxels(g.blocks(), p["voxel"])
    want_t, want_w = ref.plane_closed_form(X)
    print("\n[plane axis] %d voxels, weights %s, max |tsdf - closed form| %.2e" % (len(t), sorted(set(w.tolist())), np.abs(t - want_t).max()))
    assert (w > 0).sum() >= 6 and w.max() == len(p["offsets"])
    np.testing.assert_array_equal(w, want_w)
    np.testing.assert_allclose(t, want_t, rtol=0, atol=1e-6)


@pytest.mark.parametrize("scene", ["sphere", "plane"])
def test_mesh_matches_the_restatement(scene):
    make, voxel = SCENES[scene]
    g = _gpu_volume(make(), voxel)
    v, f, c, n = _mesh_np(g.extract_mesh())
    assert g.mesh_overruns() == 0
    rv, rf, rc, rn = ref.marching_cubes(g.blocks(), voxel, _table())
    print("\n[%s mesh] V %d F %d (restatement %d %d)" % (scene, len(v), len(f), len(rv), len(rf)))
    assert (len(v), len(f)) == (len(rv), len(rf)) and len(f) > 1000
    np.testing.assert_array_equal(f, rf)
    for a, b, name in ((v, rv, "vertices"), (c, rc, "colours"), (n, rn, "normals")):
        d = np.abs(a - b).max()
        print("[%s mesh] %s max diff %.2e" % (scene, name, d))
        assert d <= 1e-6, name


def _manifold_stats(f, V):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * V + e[:, 1]
    rkey = e[:, 1] * V + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    directed_once = bool(np.all(cnt == 1))
    paired = bool(np.all(np.isin(rkey, key)))
    und = np.unique(np.minimum(key, rkey))
    return directed_once, paired, len(und)


def test_sphere_mesh_geometry():
    g = _gpu_volume(_sphere_frames(), VOX)
    v, f, c, n = _mesh_np(g.extract_mesh())
    once, paired, E = _manifold_stats(f, len(v))
    assert once and paired                                 # every edge in exactly two faces, in opposite directions
    assert len(np.unique(f)) == len(v)                     # no unreferenced vertex
    chi = len(v) - E + len(f)
    d = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - R_S) / VOX
    outward = ((n * v).sum(1) > 0).mean()
    print("\n[sphere mesh] V %d F %d E %d chi %d, | |x| - r | / v: mean %.4f max %.4f, outward normals %.5f, colour err max %.3f"
          % (len(v), len(f), E, chi, d.mean(), d.max(), outward, np.abs(c - (0.5 + 0.5 * v / R_S)).max()))
    assert chi == 2
    # measured (restatement = kernels): mean 0.087 v, max 0.507 v -- the projective (along-the-ray) sdf of grazing views and the pixel each voxel
    # snaps to bias the zero crossing on a curved surface; the plane's is exact to 0.01 v (test_tsdf_host)
    assert d.mean() <= 0.09 and d.max() <= 0.52
    assert outward >= 0.999
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5


def test_meshes_are_deterministic_across_runs_and_capacities():
    frames = _sphere_frames()
    a = _mesh_np(_gpu_volume(frames, VOX, cap=1 << 13).extract_mesh())
    b = _mesh_np(_gpu_volume(frames, VOX, cap=1 << 13).extract_mesh())
    c = _mesh_np(_gpu_volume(frames, VOX, cap=3000).extract_mesh())          # another slot count: other slot positions, other block indices
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() and x.tobytes() == z.tobytes()


def test_end_to_end_surface_scene():
    from ibgs_amd import renderer, simple_scene, synthetic as syn
    from tests import scenes
    dev = torch.device("cuda")
    Wr, Hr = 192, 144
    g = scenes.surface_discs(40000, seed=3)
    pc = simple_scene.SimpleGaussians(g, sh_degree=2, device=dev)
    cams = []
    for el in (25.0, 55.0):
        for k in range(8):
            cams.append(simple_scene.SimpleCamera(syn.make_camera(Wr, Hr, azimuth_deg=45.0 * k + (22.5 if el > 30 else 0.0), elevation_deg=el, radius=4.0),
                                                  uid=len(cams), device=dev))
    for c in cams:
        c.nearest_id = []
    scene = simple_scene.SimpleScene(cams, device=dev)
    pipe, args = simple_scene.default_pipe(), simple_scene.default_args()
    bg = torch.zeros(3, device=dev)
    voxel = 2 * scenes.GROUND_HALF / 128
    vol = tsdf.TSDFVolume(voxel, 4 * voxel, block_capacity=1 << 15)
    with torch.no_grad():
        for c in cams:
            out = renderer.render(c, pc, scene, pipe, args, bg, learnt_normal=True, nb_src_frames=3, buffer_length=4, render_geo=True,
                                  return_depth_normal=False)
            depth = tsdf.depth_for_fusion(out, c, max_depth=8.0, use_depth_filter=True)
            vol.integrate_view(c, depth, color=out["render"])
    vol.check()
    v, f, col, n = _mesh_np(vol.extract_mesh())
    assert vol.mesh_overruns() == 0 and len(f) > 10000
    x = v.astype(np.float64)
    d_sph = np.abs(np.linalg.norm(x, axis=1) - scenes.SPHERE_R)
    d_gnd = np.abs(x[:, 2] - float(scenes.GROUND_Z))
    contact = np.array([0.0, 0.0, float(scenes.GROUND_Z)])
    away = (np.abs(x[:, 0]) < scenes.GROUND_HALF - 4 * voxel) & (np.abs(x[:, 1]) < scenes.GROUND_HALF - 4 * voxel) \
        & (np.linalg.norm(x - contact, axis=1) > 0.3)
    d = np.minimum(d_sph, d_gnd)[away] / voxel
    print("\n[end to end] voxel %.4f, V %d F %d, vertices away from contact / edges %d, distance to sphere or ground / v: median %.3f p99 %.3f max %.3f"
          % (voxel, len(v), len(f), int(away.sum()), np.median(d), np.percentile(d, 99), d.max()))
    assert away.sum() > 0.5 * len(v)
    # measured: median 0.054 v, p99 0.24 v, max 0.44 v
    assert np.median(d) < 0.1 and np.percentile(d, 99) < 0.3 and d.max() < 0.6
    assert np.isfinite(col).all() and np.isfinite(n).all()


def test_errors_before_gpu_work():
    vol = tsdf.TSDFVolume(VOX, TAU, block_capacity=64)
    M = ref.look_at((0.0, 0.0, -2.0))
    d = torch.zeros(H, W, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        vol.integrate(d.cpu(), FX, FX, CX, CY, M)
    with pytest.raises(ValueError):
        vol.integrate(torch.zeros(2, H, W, device="cuda"), FX, FX, CX, CY, M)
    with pytest.raises(ValueError):
        vol.integrate(d.double(), FX, FX, CX, CY, M)
    with pytest.raises(ValueError):
        vol.integrate(d, FX, FX, CX, CY, M, color=torch.zeros(3, H, W + 1, device="cuda"))
    with pytest.raises(RuntimeError):
        vol.integrate(d, FX, FX, CX, CY, M, color=torch.zeros(3, H, W))
    with pytest.raises(ValueError):
        vol.integrate(d, FX, FX, CX, CY, np.identity(3))
    bad = M.copy(); bad[0, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        vol.integrate(d, FX, FX, CX, CY, bad)
    with pytest.raises(ValueError):
        vol.integrate(d, 0.0, FX, CX, CY, M)
    assert vol.num_blocks() == 0


def test_capacity_overflow_raises_and_reset_recovers():
    frames = _sphere_frames(4)
    need = len(_ref_volume(frames, VOX).coords)
    cap = need // 2          # 2 x cap hash slots hold every key: the count of the blocks that found no room is exact
    vol = _gpu_volume(frames, VOX, cap=cap)
    with pytest.raises(tsdf.TSDFVolumeError, match=r"overflow: %d block\(s\) found no room" % (need - cap)):
        vol.check()
    with pytest.raises(tsdf.TSDFVolumeError):
        vol.extract_mesh()
    small = _gpu_volume(frames, VOX, cap=16)          # 32 slots: the table fills, the count is a lower bound and says so
    with pytest.raises(tsdf.TSDFVolumeError, match=r"at least 16 block\(s\) found no room .*hash table filled") as e:
        small.check()
    print("\n[overflow] blocks needed %d; capacity %d: %d reported; capacity 16: %s" % (need, cap, need - cap, e.value))
    for v in (vol, small):
        v.reset()
        v.check()
        assert v.num_blocks() == 0
        dep = np.zeros((H, W), np.float32); dep[60, 80] = 2.0          # one pixel: at most 8 blocks
        v.integrate(torch.as_tensor(dep, device="cuda"), FX, FX, CX, CY, np.identity(4))
        v.check()
        assert 1 <= v.num_blocks() <= 8
        v.extract_mesh()
        assert v.mesh_overruns() == 0


def test_integrate_does_not_wait_for_the_device():
    frames = _sphere_frames(2)
    dep, col, M, k = frames[0]
    vol = tsdf.TSDFVolume(VOX, TAU, block_capacity=1 << 12)
    dd, cc = torch.as_tensor(dep, device="cuda"), torch.as_tensor(col, device="cuda")
    vol.integrate(dd, *k, M, color=cc)          # warm-up (code objects loaded)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); torch.cuda._sleep(10 ** 7); b.record(); b.synchronize()
    cycles = int(10 ** 7 * 1000.0 / max(a.elapsed_time(b), 1e-3))          # ~1 s of device time
    torch.cuda._sleep(cycles)
    t0 = time.perf_counter()
    vol.integrate(dd, *k, M, color=cc)
    host = time.perf_counter() - t0
    e = torch.cuda.Event(); e.record()
    pending = not e.query()
    torch.cuda.synchronize()
    print("\n[async] integrate returned after %.1f ms behind a ~1 s sleep kernel (still pending: %s)" % (1e3 * host, pending))
    assert pending and host < 0.25
    vol.check()
