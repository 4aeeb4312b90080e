"""The registration unit on a CPU-only box: the C ABI (include/ibgs_registration.h <-> _lib.PCREG_EXPORTS <-> the built library), the build registration, the
argument checks of ibgs_amd.registration (which run before any GPU work), read_crop_volume, and closed forms of the host restatement
(tests/registration_ref.py) and of the host-side similarity fit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, registration as reg
from tests import registration_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SQUARE = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float64)          # in the x-z plane: a crop along Y
ELL = np.array([[0, 0, 0], [2, 0, 0], [2, 1, 0], [1, 1, 0], [1, 2, 0], [0, 2, 0]], np.float64)          # a concave "L" in the x-y plane: a crop along Z


def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_registration.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_pcreg_[a-z_0-9]+)\s*\(", text)))
    assert len(names) == 8
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.PCREG_EXPORTS) == names
    defines = re.findall(r"#define\s+IBGS_(PCREG_[A-Z_]+)\s+(\d+)", text)
    assert len(defines) >= 9
    for name, val in defines:
        assert getattr(_lib, name) == int(val), name
    # the mesh-evaluation header is untouched
    assert len(_lib.MESH_EVAL_EXPORTS) == 9 and not any("pcreg" in n for n in _lib.MESH_EVAL_EXPORTS)


def test_kernels_attributed_to_the_registration_unit():
    src = open(os.path.join(ROOT, "ibgs_amd", "csrc", "registration.hip")).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)
    assert len(kernels) >= 8 and all(k.startswith("pcreg_") for k in kernels), kernels
    for k in kernels:
        assert _build.tu_of(k) == "registration", k
    assert ("pcreg_", "registration") in _build.KERNEL_TU[1:]
    assert "registration" in _build.SOURCES and "registration" in _build.UNIT_HEADERS and "registration" in _build.tu_shas()
    assert _build.EXTRA["registration"] == ["-ffp-contract=off"]
    assert not re.search(r"atomicAdd\s*\(\s*(?!state)", src), "only the integer state words are updated with atomics"


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_pcreg_required_scratch
    assert need(-1) == 0 and need(1 << 31) == 0 and need(0) > 1024 * 18 * 8 and need(10 ** 6) >= need(0) + 8 * 10 ** 6 and need((1 << 31) - 1) > 0
    err = lambda: built_lib.ibgs_last_error()
    eye = (ctypes.c_double * 16)(*np.identity(4).reshape(-1))
    bad = (ctypes.c_double * 16)(*np.identity(4).reshape(-1))
    bad[13] = 0.5
    nan = (ctypes.c_double * 16)(*np.identity(4).reshape(-1))
    nan[2] = float("nan")
    piv = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    assert built_lib.ibgs_pcreg_transform(None, -1, 128, eye, 128, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_pcreg_transform(None, 5, 128, None, 128, 128) < 0 and b"null T" in err()
    assert built_lib.ibgs_pcreg_transform(None, 5, 128, bad, 128, 128) < 0 and b"last row" in err()
    assert built_lib.ibgs_pcreg_transform(None, 5, 128, nan, 128, 128) < 0 and b"non-finite" in err()
    assert built_lib.ibgs_pcreg_transform(None, 5, None, eye, None, None) < 0 and b"null" in err()
    assert built_lib.ibgs_pcreg_crop(None, 5, 128, None, 3, 0.0, 1.0, 4, 128, 128, 128) < 0 and b"axis" in err()
    assert built_lib.ibgs_pcreg_crop(None, 5, 128, None, 1, 0.0, 1.0, 2, 128, 128, 128) < 0 and b"polygon" in err()
    assert built_lib.ibgs_pcreg_crop(None, 5, 128, None, 1, 0.0, 1.0, 1025, 128, 128, 128) < 0 and b"polygon" in err()
    assert built_lib.ibgs_pcreg_crop(None, 5, 128, None, 1, 1.0, 0.0, 4, 128, 128, 128) < 0 and b"axis_min" in err()
    assert built_lib.ibgs_pcreg_crop(None, 5, 128, bad, 1, 0.0, 1.0, 4, 128, 128, 128) < 0 and b"last row" in err()
    assert built_lib.ibgs_pcreg_crop(None, 5, None, None, 1, 0.0, 1.0, 4, None, None, None) < 0 and b"null" in err()
    assert built_lib.ibgs_pcreg_voxel_keys(None, 5, 128, 128, 0.0, 128, 128) < 0 and b"voxel" in err()
    assert built_lib.ibgs_pcreg_voxel_keys(None, 5, 128, 128, float("nan"), 128, 128) < 0 and b"voxel" in err()
    assert built_lib.ibgs_pcreg_voxel_keys(None, 5, None, None, 0.1, None, None) < 0 and b"null" in err()
    assert built_lib.ibgs_pcreg_bounds(None, 0, 128, 128, 1 << 20, 128, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_pcreg_bounds(None, 5, 128, 64, 1 << 20, 128, 128) < 0 and b"aligned" in err()
    assert built_lib.ibgs_pcreg_bounds(None, 5, 128, 128, 16, 128, 128) < 0 and b"needed" in err()
    assert built_lib.ibgs_pcreg_voxel_count(None, 5, 128, 128, 16, 128, 128) < 0 and b"needed" in err()
    assert built_lib.ibgs_pcreg_voxel_count(None, 0, 128, 128, 1 << 20, 128, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_pcreg_voxel_emit(None, 5, 128, 128, 128, 128, 1 << 20, 6, 128, None, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_pcreg_voxel_emit(None, 5, 128, None, 128, 128, 1 << 20, 5, 128, None, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_pcreg_moments(None, 0, 128, 128, 5, 128, piv, 128, 1 << 20, 128, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_pcreg_moments(None, 5, 128, 128, 5, 128, None, 128, 1 << 20, 128, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_pcreg_moments(None, 5, 128, 128, 5, 128, piv, 128, 16, 128, 128) < 0 and b"needed" in err()
    piv[1] = float("inf")
    assert built_lib.ibgs_pcreg_moments(None, 5, 128, 128, 5, 128, piv, 128, 1 << 20, 128, 128) < 0 and b"pivot" in err()


def _vol(**kw):
    d = dict(axis="Y", axis_min=-1.0, axis_max=1.0, polygon=SQUARE)
    d.update(kw)
    return reg.CropVolume(**d)


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    p, eye = torch.zeros(6, 3), np.identity(4)
    calls = {"transform": lambda: reg.transform(p, eye), "crop": lambda: reg.crop(p, _vol()), "crop T": lambda: reg.crop(p, _vol(), eye),
             "voxel_down_sample": lambda: reg.voxel_down_sample(p, 0.1), "moments": lambda: reg.moments(p, p, 1.0), "icp": lambda: reg.icp(p, p, 1.0),
             "evaluate_tnt": lambda: reg.evaluate_tnt(p, p, eye, _vol(), 0.01)}
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn()
    for bad in (torch.zeros(6, 3, dtype=torch.float64), torch.zeros(6, 4), torch.zeros(18), torch.zeros(2, 3, 3)):
        for fn in (lambda b: reg.transform(b, eye), lambda b: reg.crop(b, _vol()), lambda b: reg.voxel_down_sample(b, 0.1), lambda b: reg.icp(b, p, 1.0),
                   lambda b: reg.icp(p, b, 1.0), lambda b: reg.moments(b, p, 1.0), lambda b: reg.evaluate_tnt(b, p, eye, _vol(), 0.01),
                   lambda b: reg.evaluate_tnt(p, b, eye, _vol(), 0.01)):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (lambda: reg.transform(np.zeros((6, 3), F32), eye), lambda: reg.crop(p, (1, 2, 3)), lambda: reg.voxel_down_sample(p, "fine"),
               lambda: reg.icp(p, [[0, 0, 0]], 1.0)):
        with pytest.raises(TypeError):
            fn()
    # a T whose last row is not 0 0 0 1, or of another shape, or not finite
    persp = np.identity(4)
    persp[3, 0] = 1e-3
    scaled = np.identity(4)
    scaled[3, 3] = 2.0
    inf = np.identity(4)
    inf[0, 3] = np.inf
    for T in (persp, scaled, inf, np.identity(3), np.zeros((3, 4))):
        for fn in (lambda T: reg.transform(p, T), lambda T: reg.crop(p, _vol(), T), lambda T: reg.icp(p, p, 1.0, init=T), lambda T: reg.moments(p, p, 1.0, T),
                   lambda T: reg.evaluate_tnt(p, p, T, _vol(), 0.01)):
            with pytest.raises(ValueError):
                fn(T)
    # a bad polygon or volume
    for vol in (_vol(polygon=SQUARE[:2]), _vol(polygon=np.zeros((1025, 3))), _vol(polygon=SQUARE[:, :2]), _vol(polygon=np.full((4, 3), np.nan)), _vol(axis="W"),
                _vol(axis_min=1.0, axis_max=-1.0), _vol(axis_min=float("nan"))):
        for fn in (lambda v: reg.crop(p, v), lambda v: reg.evaluate_tnt(p, p, eye, v, 0.01)):
            with pytest.raises(ValueError):
                fn(vol)
    # a non-positive voxel size, tau or max_dist
    for x in (0.0, -1.0, float("nan"), float("inf")):
        for fn in (lambda x: reg.voxel_down_sample(p, x), lambda x: reg.icp(p, p, x), lambda x: reg.moments(p, p, x), lambda x: reg.evaluate_tnt(p, p, eye, _vol(), x)):
            with pytest.raises(ValueError):
                fn(x)
    for kw in (dict(max_iter=-1), dict(rel_fitness=-1.0), dict(rel_rmse=float("nan"))):
        with pytest.raises(ValueError):
            reg.icp(p, p, 1.0, **kw)
    for kw in (dict(voxel_rounds=((0.0, 80),)), dict(voxel_rounds=((1, -1),)), dict(uniform_round=0.0), dict(max_points=0)):
        with pytest.raises(ValueError):
            reg.evaluate_tnt(p, p, eye, _vol(), 0.01, **kw)


def test_read_crop_volume_round_trips(tmp_path):
    poly = np.array([[0.1, 7.0, -2.5], [3.25, 7.0, -2.0], [2.0, 7.0, 1.0 / 3.0], [-1.0, 7.0, 4.0]])
    path = str(tmp_path / "Scene.json")
    ref.write_crop_volume(path, "Y", -0.7071067811865476, 12.5, poly)
    vol = reg.read_crop_volume(path)
    assert vol.axis == "Y" and vol.axis_min == -0.7071067811865476 and vol.axis_max == 12.5
    assert vol.polygon.dtype == np.float64 and vol.polygon.tobytes() == poly.tobytes()
    w, lo, hi, uv = reg._check_volume(vol)
    assert (w, lo, hi) == (1, vol.axis_min, 12.5) and uv.tobytes() == np.ascontiguousarray(poly[:, [0, 2]]).tobytes()
    assert [reg._check_volume(vol._replace(axis=a))[0] for a in "XYZ"] == [0, 1, 2]
    assert reg._check_volume(vol._replace(axis="X"))[3].tobytes() == np.ascontiguousarray(poly[:, [1, 2]]).tobytes()
    ref.write_crop_volume(path, "Y", 0.0, 1.0, poly[:2])
    with pytest.raises(ValueError):
        reg.read_crop_volume(path)


def test_restatement_square_crop_is_a_box_test():
    rng = np.random.default_rng(0)
    p = rng.uniform(-1.5, 1.5, (4000, 3)).astype(F32)
    got = ref.crop(p, "Y", -0.5, 0.75, SQUARE)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    want = (y >= -0.5) & (y <= 0.75) & (np.abs(x) < 1) & (np.abs(z) < 1)
    np.testing.assert_array_equal(got, want)
    assert 100 < got.sum() < 3000
    # the axis bounds are closed, and the transform comes first
    edge = np.array([[0, -0.5, 0], [0, 0.75, 0], [0, np.nextafter(F32(0.75), F32(1)), 0]], F32)
    assert ref.crop(edge, "Y", -0.5, 0.75, SQUARE).tolist() == [True, True, False]
    shift = np.identity(4)
    shift[0, 3] = 2.0
    np.testing.assert_array_equal(ref.crop(p, "Y", -0.5, 0.75, SQUARE, T=shift), ref.crop(ref.transform(p, shift), "Y", -0.5, 0.75, SQUARE))
    assert ref.crop(p, "Y", -0.5, 0.75, SQUARE, T=shift).sum() < got.sum()


def test_restatement_concave_polygon():
    g = (np.arange(-2, 26) + 0.5) / 10.0
    p = np.stack(np.meshgrid(g, g, [0.5], indexing="ij"), -1).reshape(-1, 3).astype(F32)
    got = ref.crop(p, "Z", 0.0, 1.0, ELL)
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    want = (x > 0) & (y > 0) & (((x < 2) & (y < 1)) | ((x < 1) & (y < 2)))
    np.testing.assert_array_equal(got, want)
    assert got.sum() == 300          # area 3 at 100 points per unit square
    # the half-open rule at a vertex's v (an edge crosses when one end is below p[v] and the other at or above it): a level that holds vertices belongs to
    # the region below it -- y = 1 to the lower arm (its top edge is inside), y = 2 to the upper arm, y = 0 to nothing
    ray = np.array([[0.5, 1.0, 0.5], [1.5, 1.0, 0.5], [2.5, 1.0, 0.5], [0.5, 0.0, 0.5], [0.5, 2.0, 0.5], [1.5, 2.0, 0.5]], F32)
    assert ref.crop(ray, "Z", 0.0, 1.0, ELL).tolist() == [True, True, False, False, True, False]


def test_restatement_voxel_mean_of_a_lattice_gives_the_cell_centres():
    v = 0.25
    # 8 points per cell at the corners of a cube of side v / 4 around the lattice point c; the cloud's minimum is c0 - v / 8 on every axis, the grid's origin
    # c0 - 5 v / 8, so cell k spans [c_k - 5 v / 8, c_k + 3 v / 8) and holds exactly the cube around c_k ... all exact in binary
    cells = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    corners = np.stack(np.meshgrid([-1, 1], [-1, 1], [-1, 1], indexing="ij"), -1).reshape(-1, 3) * (v / 8)
    centres = -1.0 + v / 2 + cells * v
    p = (centres[:, None, :] + corners[None]).reshape(-1, 3).astype(F32)
    np.random.default_rng(1).shuffle(p)
    means, keys, counts, over = ref.voxel_down_sample(p, v)
    assert over == 0 and len(means) == 60 and np.all(counts == 8) and np.all(np.diff(keys) > 0)
    idx = np.stack([keys >> 42, (keys >> 21) & ref.MAX_INDEX, keys & ref.MAX_INDEX], 1)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    np.testing.assert_array_equal(idx, cells[order])
    np.testing.assert_array_equal(means, centres[order])
    assert ref.voxel_down_sample(np.zeros((0, 3), F32), v)[0].shape == (0, 3)
    assert ref.voxel_down_sample(np.array([[0, 0, 0], [1, 0, 0]], F32), 1e-7)[3] == 1


@pytest.mark.parametrize("fit", [reg.umeyama_points, ref.umeyama_points])
def test_umeyama_recovers_a_planted_similarity(fit):
    rng = np.random.default_rng(5)
    s = rng.normal(size=(200, 3)) * [1.0, 2.0, 0.5] + [10.0, -3.0, 4.0]
    for T in (ref.PLANTED, ref.similarity(0.37, 140.0, (1, 1, -2), (5, -8, 100)), np.identity(4)):
        t = s @ T[:3, :3].T + T[:3, 3]
        got = fit(s, t)
        assert np.abs(got - T).max() <= 1e-12 * max(1.0, np.abs(T).max()), np.abs(got - T).max()
        assert got[3].tolist() == [0, 0, 0, 1]
    # a reflected pair: the best proper rotation, never a reflection
    t = s * [1.0, 1.0, -1.0]
    got = fit(s, t)
    scale = np.cbrt(np.linalg.det(got[:3, :3]))
    assert scale > 0 and abs(np.linalg.det(got[:3, :3] / scale) - 1.0) < 1e-12
    np.testing.assert_allclose(got[:3, :3] @ got[:3, :3].T, scale * scale * np.identity(3), atol=1e-12)


def test_umeyama_from_moments_agrees_and_refuses_degenerate_input():
    rng = np.random.default_rng(6)
    s = rng.normal(size=(300, 3)).astype(F32)
    t = (s.astype(np.float64) @ ref.PLANTED[:3, :3].T + ref.PLANTED[:3, 3]).astype(F32)
    idx = np.arange(300)
    idx[::7] = -1
    for c in (np.zeros(3), ref.pivot_of(t), np.array([100.0, -50.0, 7.0])):
        m = ref.moments(s, t, idx, c)
        assert m[0] == (idx >= 0).sum()
        a, b = reg.umeyama(m, c), ref.umeyama(m, c)
        want = ref.umeyama_points(s[idx >= 0], t[idx >= 0])
        assert np.abs(a - b).max() <= 1e-13 and np.abs(a - want).max() <= 1e-9 * (1 + np.abs(c).max() ** 2)
    m = ref.moments(s, t, np.where(idx < 2, idx, -1), np.zeros(3))
    with pytest.raises(reg.RegistrationError, match="at least 3"):
        reg.umeyama(m, np.zeros(3))
    same = np.repeat(s[:1], 5, 0)
    with pytest.raises(reg.RegistrationError, match="no extent"):
        reg.umeyama(ref.moments(same, t[:5], np.arange(5), np.zeros(3)), np.zeros(3))
    with pytest.raises(ValueError):
        reg.umeyama(np.zeros(17))


def test_restatement_icp_converges_on_the_planted_scene():
    src, tgt = ref.icp_scene(2000, 500, seed=1)
    r = ref.icp(src, tgt, 0.5)
    assert 3 <= r["iterations"] < 20 and r["fitness"] == 1.0
    assert np.abs(r["transformation"] - ref.PLANTED).max() < 1e-6
    r0 = ref.icp(src, tgt, 0.5, max_iter=0)
    assert r0["iterations"] == 0 and np.array_equal(r0["transformation"], np.identity(4)) and r0["inlier_rmse"] > r["inlier_rmse"]


def test_product_code_imports_neither_scipy_nor_the_tests():
    src = open(os.path.join(ROOT, "ibgs_amd", "registration.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn|oracle|tests|open3d)\b", src, re.M)
