"""CPU checks of the TSDF stage: the numpy restatement (tests/tsdf_ref.py) against a closed form, the PLY mesh writer, and depth_for_fusion against
a numpy restatement of render.py:228-272."""
import math
import os

import numpy as np
import pytest
import torch

from ibgs_amd import ply, simple_scene, synthetic as syn
from ibgs_amd import tsdf
from tests import tsdf_ref as ref


def test_restatement_plane_closed_form():
    p = ref.PLANE
    vol = ref.RefVolume(p["voxel"], 4 * p["voxel"])
    for depth, M in ref.plane_views():
        vol.integrate(depth, p["fx"], p["fy"], p["cx"], p["cy"], M)
    b = vol.blocks()
    t, w, X = ref.axis_voxels(b, p["voxel"])
    want_t, want_w = ref.plane_closed_form(X)
    assert (w > 0).sum() >= 6 and w.max() == len(p["offsets"])
    np.testing.assert_array_equal(w, want_w)
    np.testing.assert_allclose(t, want_t, rtol=0, atol=1e-6)
    # every voxel of the volume, not only the axis column
    I = b["coords"][:, None, :] * tsdf.BLOCK + ref.LOCAL[None]
    allX = (I.reshape(-1, 3).astype(np.float64) + 0.5) * p["voxel"]
    ct, cw = ref.plane_closed_form(allX)
    assert np.mean(cw == b["weight"].reshape(-1)) > 0.999
    same = cw == b["weight"].reshape(-1)
    assert np.abs(ct[same] - b["tsdf"].reshape(-1)[same]).max() < 2e-6          # (f32 z has ~6e-8 error, divided by tau = 0.08)
    # the allocated blocks are exactly those within tau of the plane (z blocks), across the back-projected footprint
    zb = np.unique(b["coords"][:, 2])
    B = 8 * p["voxel"]
    assert list(zb) == list(range(int(np.floor((p["z0"] - 4 * p["voxel"]) / B)), int(np.floor((p["z0"] + 4 * p["voxel"]) / B)) + 1))


def test_restatement_mesh_of_the_plane_is_flat_and_faces_the_cameras(built_lib):
    import ctypes
    p = ref.PLANE
    vol = ref.RefVolume(p["voxel"], 4 * p["voxel"])
    for depth, M in ref.plane_views():
        vol.integrate(depth, p["fx"], p["fy"], p["cx"], p["cy"], M)
    table = (ctypes.c_int32 * 4096)()
    built_lib.ibgs_tsdf_mc_table(table)
    v, f, c, n = ref.marching_cubes(vol.blocks(), p["voxel"], np.array(table))
    assert len(v) > 100 and len(f) > 100
    assert np.abs(v[:, 2] - p["z0"]).max() < 0.02 * p["voxel"]          # (the distance multiplier m varies per pixel: not exactly linear)
    assert np.all(n[:, 2] < -0.999)                                      # free space is towards the cameras (-z)
    assert len(np.unique(f)) == len(v)                                   # no unreferenced vertex


def test_ply_mesh_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    V, F = 57, 91
    mesh = tsdf.TriangleMesh(torch.as_tensor(rng.normal(size=(V, 3)).astype(np.float32)), torch.as_tensor(rng.integers(0, V, (F, 3)).astype(np.int32)),
                             torch.as_tensor(rng.uniform(-0.2, 1.2, (V, 3)).astype(np.float32)), torch.as_tensor(rng.normal(size=(V, 3)).astype(np.float32)))
    mesh.colors[0] = torch.tensor([0.5, 1.0, -0.1])          # 127.5 rounds up
    path = os.path.join(str(tmp_path), "m.ply")
    ply.save_mesh(path, mesh)
    raw = open(path, "rb").read()
    header = raw[:raw.index(b"end_header\n")].decode()
    assert "format binary_little_endian 1.0" in header and "element vertex %d" % V in header and "element face %d" % F in header
    assert "property uchar red" in header and "property list uchar int vertex_indices" in header and "property float nz" in header
    assert len(raw) == len(header) + len("end_header\n") + V * (6 * 4 + 3) + F * 13
    back = ply.load_mesh(path)
    np.testing.assert_array_equal(back["vertices"], mesh.vertices.numpy())
    np.testing.assert_array_equal(back["normals"], mesh.normals.numpy())
    np.testing.assert_array_equal(back["faces"], mesh.faces.numpy())
    want = np.floor(255 * np.clip(mesh.colors.numpy().astype(np.float64), 0, 1) + 0.5).astype(np.uint8)
    np.testing.assert_array_equal(back["colors"], want)
    assert list(back["colors"][0]) == [128, 255, 0]


def _fusion_restatement(depth, normal, cam, max_depth, use_filter, bounds):
    """render.py:228-272 + Open3D's depth_trunc in numpy (float32 where the reference computes in float32)."""
    d = depth.copy()
    H, W = d.shape
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    rays = np.stack([(u - cam.Cx) / cam.Fx, (v - cam.Cy) / cam.Fy, np.ones_like(u, dtype=np.float64)], -1).astype(np.float32)
    near = np.zeros_like(d, bool)
    if use_filter:
        vd = rays / np.maximum(np.linalg.norm(rays, axis=-1, keepdims=True), 1e-12)
        dn = normal.transpose(1, 2, 0)
        dn = dn / np.maximum(np.linalg.norm(dn, axis=-1, keepdims=True), 1e-12)
        ang = np.arccos(np.clip(np.abs((vd * dn).sum(-1)), 0, 1))
        thr = 80.0 / 180 * 3.14159
        near = np.abs(ang - thr) < 1e-5
        d[ang > thr] = 0
    if bounds is not None:
        pts = (rays * d[..., None]).reshape(-1, 3).astype(np.float64)
        pts = (pts - np.asarray(cam.T, np.float64)) @ np.asarray(cam.R, np.float64).T
        bad = np.zeros(len(pts), bool)
        for a in range(3):
            bad |= (pts[:, a] < bounds[a, 0]) | (pts[:, a] > bounds[a, 1])
        d[bad.reshape(H, W)] = 0
    d[d > max_depth] = 0
    return d, near


@pytest.mark.parametrize("use_filter,with_bounds", [(False, False), (True, False), (False, True), (True, True)])
def test_depth_for_fusion_matches_render_py(use_filter, with_bounds):
    W, H = 96, 64
    cam = simple_scene.SimpleCamera(syn.make_camera(W, H, azimuth_deg=30.0), device="cpu")
    rng = np.random.default_rng(5)
    depth = rng.uniform(2.0, 6.0, (H, W)).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.1] = 0
    normal = rng.normal(size=(3, H, W)).astype(np.float32)
    bounds = np.array([[-0.8, 0.9], [-1.0, 0.7], [-0.5, 1.2]]) if with_bounds else None
    pkg = {"median_intersected_depth": torch.as_tensor(depth)[None], "median_intersected_depth_normal": torch.as_tensor(normal)}
    got = tsdf.depth_for_fusion(pkg, cam, max_depth=5.0, use_depth_filter=use_filter, bounds=bounds).numpy()
    want, near = _fusion_restatement(depth, normal, cam, 5.0, use_filter, bounds)
    assert got.shape == (H, W) and got.dtype == np.float32
    differ = (got != want) & ~near
    # (the bounds test compares float32 points against float64 ones: a point within rounding of a box face may go either way)
    assert differ.sum() <= (3 if with_bounds else 0), differ.sum()
    assert (got == 0).mean() > 0.1 and (got > 0).mean() > 0.05
    if use_filter:
        assert ((want == 0) & (depth > 0) & (depth <= 5)).mean() > 0.02          # the filter did remove pixels
    assert float(pkg["median_intersected_depth"].min()) == 0.0 and float(pkg["median_intersected_depth"].max()) > 5          # input untouched


def test_volume_refuses_cpu_and_bad_arguments():
    with pytest.raises(RuntimeError, match="MI355X"):
        tsdf.TSDFVolume(0.01, 0.04, block_capacity=16, device="cpu")
    with pytest.raises(ValueError):
        tsdf.TSDFVolume(0.0, 0.04, block_capacity=16, device="cpu")
    with pytest.raises(ValueError):
        tsdf.TSDFVolume(0.01, math.nan, block_capacity=16, device="cpu")


def test_key_packing_round_trip():
    c = np.array([[0, 0, 0], [-1, 2, -3], [(1 << 20) - 1, -(1 << 20), 5]])
    k = tsdf.pack_keys(c)
    assert (k >= 0).all() and (k < (1 << 63) - 1).all()
    np.testing.assert_array_equal(tsdf.unpack_keys(k), c)
    # ascending packed key = ascending (z, y, x)
    assert np.all(np.diff(tsdf.pack_keys(np.array([[5, 0, 0], [0, 1, 0], [0, 0, 1]]))) > 0)
