"""The DTU unit on a CPU-only box: the host restatement (tests/dtu_ref.py) against scipy's binary dilation and torch's CPU grid_sample, the C ABI
(include/ibgs_dtu.h <-> _lib.DTU_EXPORTS <-> the built library), the build registration, the argument checks of ibgs_amd.dtu (which run before any GPU
work), and read_obs_mask."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, dtu
from tests import dtu_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the restatement against the libraries the reference calls ---------------------------------------------------------------------------------------
def _marked(H, W, seed):
    """A sparse random mask with the pixels that matter set: the four corners, the last column of a word, the first of the next, the last of the row."""
    m = np.random.default_rng(seed).uniform(size=(H, W)) < 0.004
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, min(63, W - 1)), (H // 3, min(64, W - 1))):
        m[y, x] = True
    return m


@pytest.mark.parametrize("H,W,r", [(30, 40, 24), (67, 130, 24), (70, 100, 1), (33, 65, 0)])
def test_restated_dilation_is_scipys_binary_dilation_with_a_disc(H, W, r):
    ndi = pytest.importorskip("scipy.ndimage")
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disc = xx * xx + yy * yy <= r * r
    assert disc.sum() == len(ref.disc_offsets(r))
    for m in (_marked(H, W, 1), np.zeros((H, W), bool)):
        want = ndi.binary_dilation(m, structure=disc)          # (border_value = 0: zero outside the image)
        got = ref.dilate(m, r)
        np.testing.assert_array_equal(got, want)
        assert got.sum() >= m.sum() and (got.any() == m.any())
    # the bit layout round-trips and pads with zeros
    d = ref.dilate(_marked(H, W, 2), r)[None]
    img, pad = ref.unpack_bits(ref.pack_bits(d), W)
    np.testing.assert_array_equal(img, d)
    assert not pad.any() and ref.pack_bits(d).shape == (1, H, (W + 63) // 64)


def test_restated_sampling_chain_is_torchs_cpu_grid_sample():
    W, H = 130, 67
    rng = np.random.default_rng(3)
    n = 20_000
    u = rng.uniform(-5, W + 4, n).astype(F32)
    v = rng.uniform(-5, H + 4, n).astype(F32)
    # rows of exact half-pixels, and exact pixels
    u[:2000] = (rng.integers(-5, W + 4, 2000) + 0.5).astype(F32)
    v[1000:3000] = (rng.integers(-5, H + 4, 2000) + 0.5).astype(F32)
    u[3000:3500] = rng.integers(-2, W + 2, 500).astype(F32)
    image = np.arange(H * W, dtype=np.float64).reshape(H, W) + 1          # > 0 everywhere: 0 = the padding
    assert image.max() < 2 ** 24
    valid, ix, iy = ref.pixel_of(u, v, W, H)
    want = np.where(valid, image[iy, ix], 0.0)
    # the reference's own lines (evaluate_single_scene.py:77-83) on the CPU
    pix = torch.from_numpy(np.stack([u, v], 1))
    pix[:, 0] = (pix[:, 0] / (W - 1) - 0.5) * 2
    pix[:, 1] = (pix[:, 1] / (H - 1) - 0.5) * 2
    got = torch.nn.functional.grid_sample(torch.from_numpy(image.astype(F32))[None, None], pix[None, None], mode="nearest", padding_mode="zeros",
                                          align_corners=True)[0, 0, 0].numpy()
    inside = ((pix > -1.0) & (pix < 1.0)).all(dim=-1).numpy()
    np.testing.assert_array_equal(inside, valid)
    np.testing.assert_array_equal(got[valid], want[valid].astype(F32))
    assert 0.3 * n < valid.sum() < 0.95 * n
    # ... and the chain is not rint(u): the round trip moves some half-pixels to the other neighbour
    assert (ix[valid] != np.rint(u[valid])).any() and (iy[valid] != np.rint(v[valid])).any()
    assert ix[valid].min() == 0 and ix[valid].max() == W - 1 and iy[valid].min() == 0 and iy[valid].max() == H - 1


def test_restated_vertex_rule_on_a_hand_made_view():
    W, H = 130, 67
    P = ref.look_at((0, 0, -5), (0, 0, 0), (0, -1, 0), 100.0, W, H)
    d = np.zeros((H, W), bool)
    d[:, :65] = True
    pts = np.array([[0, 0, 0], [-0.5, 0, 0], [0.5, 0, 0], [100, 0, 0], [0, 0, -5 - 1e-6]], F32)
    u, v, den = ref.project(pts, P)
    assert abs(u[0] - 64.5) < 1e-3 and abs(v[0] - 33.0) < 1e-3
    passes, valid = ref.view_passes(pts, P, d)
    assert valid.tolist()[:4] == [True, True, True, False]
    assert passes[3] and passes[4] and not valid[4]          # outside the view, and at the camera's plane (c_2 + 1e-6 rounds to 0): the view does not reject
    assert passes[1] != passes[2]          # half a unit to either side of the mask's edge
    assert ref.cull_vertices(pts, np.zeros((0, 3, 4), F32), np.zeros((0, H, W), bool)).all()          # no view keeps everything


def test_restated_filters_closed_forms():
    obs = np.zeros((4, 3, 2), np.uint8)
    obs[1, 2, 0] = 1
    bb = np.array([[0, 0, 0], [6, 4, 2]], F32)
    p = np.array([[2, 4, 0], [2.99, 4.9, 0.9], [3.0, 4, 0], [1.0, 4, 0], [-1, 0, 0], [-1.0001, 0, 0], [8, 0, 0], [7.999, 0, 0]], F32)
    inbound, in_obs = ref.obs_mask_filter(p, obs, bb, res=2.0, patch=1.0)
    # g = rint(p / 2): x = 3.0 -> rint(1.5) = 2, x = 1.0 -> rint(0.5) = 0 (ties to even): both leave voxel 1
    assert in_obs.tolist() == [True, True, False, False, False, False, False, False]
    assert inbound.tolist() == [True, True, True, True, True, False, False, True]          # lo = -1 is inside, hi = 6 + 2 is not
    assert ref.above_plane(np.array([[0, 0, 1], [0, 0, 0], [0, 0, -1]], F32), [0, 0, 1, 0]).tolist() == [True, False, False]


# ---- the ABI and the build ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_dtu.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_dtu_[a-z_0-9]+)\s*\(", text)))
    assert len(names) == 8
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.DTU_EXPORTS) == names
    defines = re.findall(r"#define\s+IBGS_(DTU_[A-Z_]+)\s+(\d+)", text)
    assert len(defines) >= 8
    for name, val in defines:
        assert getattr(_lib, name) == int(val), name
    # the other geometry headers are untouched
    assert len(_lib.PCREG_EXPORTS) == 8 and len(_lib.MESH_EVAL_EXPORTS) == 9 and not any("dtu" in n for n in _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS)


def test_kernels_attributed_to_the_dtu_unit():
    src = open(os.path.join(ROOT, "ibgs_amd", "csrc", "dtu.hip")).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)
    assert len(kernels) >= 9 and all(k.startswith("dtu_") for k in kernels), kernels
    for k in kernels + ["dtu_emit_mesh_kernel", "dtu_scan_kernel"]:
        assert _build.tu_of(k) == "dtu", k
    order = [sub for sub, _ in _build.KERNEL_TU]
    assert order.index("dtu_") < order.index("mesh_") and order.index("dtu_") < order.index("scan_") and order[0] == "meval_"
    assert "dtu" in _build.SOURCES and "dtu" in _build.UNIT_HEADERS and "dtu" in _build.tu_shas()
    assert _build.EXTRA["dtu"] == ["-ffp-contract=off"]
    assert not re.search(r"atomicAdd\s*\(\s*(?!state)", src), "only the integer state words are updated with atomics"
    assert "cumsum" not in open(os.path.join(ROOT, "ibgs_amd", "dtu.py")).read()


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need_d, need_c = built_lib.ibgs_dtu_required_dilate_scratch, built_lib.ibgs_dtu_required_cull_scratch
    assert need_d(49, 1200, 1600) >= 49 * 1200 * 25 * 8 and need_d(0, 2, 2) > 0 and need_d(1, 1, 40) == 0 and need_d(1, 40, 1) == 0 and need_d(-1, 2, 2) == 0
    assert need_d(1 << 20, 65536, 65536) == 0 and need_d(1, 65537, 2) == 0
    assert need_c(-1, 0) == 0 and need_c(0, 1 << 30) == 0 and need_c(1 << 31, 0) == 0 and need_c(0, 0) > 0 and need_c(10 ** 6, 2 * 10 ** 6) >= 12 * 10 ** 6
    err = lambda: built_lib.ibgs_last_error()
    f3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    d3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    d4 = (ctypes.c_double * 4)(0.0, 0.0, 1.0, 0.0)
    assert built_lib.ibgs_dtu_dilate(None, 1, 30, 40, 256, 128, 128, 1 << 20, 128) < 0 and b"radius" in err()
    assert built_lib.ibgs_dtu_dilate(None, 1, 30, 40, -1, 128, 128, 1 << 20, 128) < 0 and b"radius" in err()
    assert built_lib.ibgs_dtu_dilate(None, 1, 30, 1, 24, 128, 128, 1 << 20, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_dtu_dilate(None, 1, 30, 40, 24, None, 128, 1 << 20, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_dtu_dilate(None, 1, 30, 40, 24, 128, 64, 1 << 20, 128) < 0 and b"aligned" in err()
    assert built_lib.ibgs_dtu_dilate(None, 1, 30, 40, 24, 128, 128, 16, 128) < 0 and b"needed" in err()
    assert built_lib.ibgs_dtu_dilate(None, 0, 30, 40, 24, None, None, 0, None) == 0          # no view: nothing to do
    assert built_lib.ibgs_dtu_cull_vertices(None, -1, 128, 1, 128, 30, 40, 128, 128, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_dtu_cull_vertices(None, 5, 128, 1, 128, 30, 1, 128, 128, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_dtu_cull_vertices(None, 5, 128, 1, None, 30, 40, 128, 128, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_dtu_cull_count(None, 5, 1 << 30, 128, 128, 128, 1 << 20, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_dtu_cull_count(None, 5, 5, None, 128, 128, 1 << 20, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_dtu_cull_count(None, 5, 5, 128, 128, 128, 16, 128) < 0 and b"needed" in err()
    assert built_lib.ibgs_dtu_cull_emit(None, 5, 5, 128, 128, None, None, 128, 1 << 20, 1.0, f3, 6, 0, 128, 128, None, None, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_dtu_cull_emit(None, 5, 5, 128, 128, None, None, 128, 1 << 20, 1.0, None, 5, 5, 128, 128, None, None, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_dtu_cull_emit(None, 5, 5, 128, 128, None, None, 128, 1 << 20, 1.0, f3, 5, 5, 128, 128, 128, None, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_dtu_obs_filter(None, 5, 128, 128, 0, 3, 3, f3, f3, d3, 1.0, 128, 128, 128) < 0 and b"shape" in err()
    assert built_lib.ibgs_dtu_obs_filter(None, 5, 128, 128, 3, 3, 3, f3, f3, d3, 0.0, 128, 128, 128) < 0 and b"res" in err()
    assert built_lib.ibgs_dtu_obs_filter(None, 5, 128, 128, 3, 3, 3, f3, f3, d3, float("nan"), 128, 128, 128) < 0 and b"res" in err()
    assert built_lib.ibgs_dtu_obs_filter(None, 5, 128, 128, 3, 3, 3, None, f3, d3, 1.0, 128, 128, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_dtu_obs_filter(None, 5, None, 128, 3, 3, 3, f3, f3, d3, 1.0, 128, 128, 128) < 0 and b"null" in err()
    assert built_lib.ibgs_dtu_above_plane(None, 5, 128, None, 128, 128) < 0 and b"null plane" in err()
    assert built_lib.ibgs_dtu_above_plane(None, 5, None, d4, 128, 128) < 0 and b"null" in err()
    d4[1] = float("inf")
    assert built_lib.ibgs_dtu_above_plane(None, 5, 128, d4, 128, 128) < 0 and b"non-finite" in err()


def _cpu_mesh(V=6, F=2):
    z = torch.zeros(V, 3)
    return types.SimpleNamespace(vertices=z, faces=torch.zeros(F, 3, dtype=torch.int32), colors=z.clone(), normals=z.clone())


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    p, masks, proj = torch.zeros(6, 3), torch.zeros(2, 30, 40, dtype=torch.uint8), torch.zeros(2, 3, 4)
    bits = dtu.MaskBits(torch.zeros(2, 30, 1, dtype=torch.int64), 30, 40)
    obs, bb, plane = torch.zeros(4, 3, 2, dtype=torch.uint8), np.array([[0, 0, 0], [1, 1, 1]], F32), [0, 0, 1, 0]
    m = _cpu_mesh()
    calls = {"dilate_masks": lambda: dtu.dilate_masks(masks), "dilate_masks bool": lambda: dtu.dilate_masks(masks.bool(), 3),
             "cull_vertices": lambda: dtu.cull_vertices(p, proj, bits), "cull_mesh": lambda: dtu.cull_mesh(m, proj, masks),
             "cull_mesh bits": lambda: dtu.cull_mesh(m, proj, bits), "obs_mask_filter": lambda: dtu.obs_mask_filter(p, obs, bb, 1.0),
             "above_plane": lambda: dtu.above_plane(p, plane), "evaluate_dtu": lambda: dtu.evaluate_dtu(m, p, obs, bb, 1.0, plane),
             "evaluate_dtu cull": lambda: dtu.evaluate_dtu(m, p, obs, bb, 1.0, plane, cull=dtu.Cull(proj, masks))}
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn()
    # wrong dtypes and shapes
    for bad in (torch.zeros(2, 30, 40), torch.zeros(30, 40, dtype=torch.uint8), torch.zeros(2, 30, 40, dtype=torch.int32), torch.zeros(2, 30, 1, dtype=torch.uint8),
                torch.zeros(2, 1, 40, dtype=torch.uint8)):
        for fn in (lambda b: dtu.dilate_masks(b), lambda b: dtu.cull_mesh(m, proj, b)):
            with pytest.raises(ValueError):
                fn(bad)
    for bad in (torch.zeros(6, 3, dtype=torch.float64), torch.zeros(6, 4), torch.zeros(18)):
        for fn in (lambda b: dtu.cull_vertices(b, proj, bits), lambda b: dtu.obs_mask_filter(b, obs, bb, 1.0), lambda b: dtu.above_plane(b, plane),
                   lambda b: dtu.evaluate_dtu(m, b, obs, bb, 1.0, plane)):
            with pytest.raises(ValueError):
                fn(bad)
    for bad in (torch.zeros(2, 4, 4), torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(3, 4)):
        for fn in (lambda b: dtu.cull_vertices(p, b, bits), lambda b: dtu.cull_mesh(m, b, masks)):
            with pytest.raises(ValueError):
                fn(bad)
    # n differs between the projections and the masks
    for fn in (lambda: dtu.cull_vertices(p, torch.zeros(3, 3, 4), bits), lambda: dtu.cull_mesh(m, torch.zeros(3, 3, 4), masks),
               lambda: dtu.cull_mesh(m, torch.zeros(1, 3, 4), bits), lambda: dtu.evaluate_dtu(m, p, obs, bb, 1.0, plane, cull=(torch.zeros(3, 3, 4), masks, 24, 1.0, (0, 0, 0)))):
        with pytest.raises(ValueError, match="view"):
            fn()
    # the radius and the image's limits
    for r in (256, -1, 2.5):
        for fn in (lambda r: dtu.dilate_masks(masks, r), lambda r: dtu.cull_mesh(m, proj, masks, radius=r)):
            with pytest.raises(ValueError, match="radius"):
                fn(r)
    with pytest.raises(TypeError):
        dtu.dilate_masks(masks, "wide")
    with pytest.raises(ValueError, match="W"):
        dtu.dilate_masks(torch.zeros(2, 30, 1, dtype=torch.uint8))
    # mask bits that do not fit their H, W
    for mb in (dtu.MaskBits(torch.zeros(2, 30, 2, dtype=torch.int64), 30, 40), dtu.MaskBits(torch.zeros(2, 30, 1, dtype=torch.int32), 30, 40),
               dtu.MaskBits(torch.zeros(2, 30, 1, dtype=torch.int64), 30, 1)):
        with pytest.raises(ValueError):
            dtu.cull_vertices(p, proj, mb)
    for fn in (lambda: dtu.dilate_masks(np.zeros((2, 30, 40), np.uint8)), lambda: dtu.cull_vertices(p, proj, masks), lambda: dtu.cull_vertices(p, [[0]], bits),
               lambda: dtu.cull_mesh((1, 2), proj, masks), lambda: dtu.obs_mask_filter(p, np.zeros((2, 2, 2)), bb, 1.0), lambda: dtu.above_plane(p, "flat"),
               lambda: dtu.evaluate_dtu(m, p, obs, bb, 1.0, plane, cull=5)):
        with pytest.raises(TypeError):
            fn()
    # the box, the plane, the move
    for kw in (dict(bb=np.zeros((3, 2))), dict(bb=np.full((2, 3), np.nan)), dict(res=0.0), dict(res=float("nan")), dict(patch=-1.0),
               dict(obs_mask=torch.zeros(4, 3, dtype=torch.uint8)), dict(obs_mask=torch.zeros(4, 3, 2))):
        a = dict(obs_mask=obs, bb=bb, res=1.0, patch=60.0)
        a.update(kw)
        with pytest.raises(ValueError):
            dtu.obs_mask_filter(p, a["obs_mask"], a["bb"], a["res"], a["patch"])
        with pytest.raises(ValueError):
            dtu.evaluate_dtu(m, p, a["obs_mask"], a["bb"], a["res"], plane, patch=a["patch"])
    for bad in ([0, 0, 1], [0, 0, 1, float("inf")]):
        with pytest.raises(ValueError):
            dtu.above_plane(p, bad)
    for kw in (dict(scale=float("nan")), dict(offset=(0, 0)), dict(offset=(0, 0, float("inf")))):
        with pytest.raises(ValueError):
            dtu.cull_mesh(m, proj, masks, **kw)
    for kw in (dict(density=0.0), dict(max_dist=-1.0)):
        with pytest.raises(ValueError):
            dtu.evaluate_dtu(m, p, obs, bb, 1.0, plane, **kw)


def test_read_obs_mask_round_trips(tmp_path):
    sio = pytest.importorskip("scipy.io")
    rng = np.random.default_rng(4)
    obs = (rng.uniform(size=(12, 9, 7)) < 0.5).astype(np.uint8)
    bb = np.array([[-1.5, 2.25, 3.0], [10.5, 11.0, 9.125]], F32)
    plane = np.array([0.1, -0.2, 0.97, 612.3456789012345])
    sio.savemat(str(tmp_path / "ObsMask1_10.mat"), {"ObsMask": obs.astype(bool), "BB": bb, "Res": np.array([[0.7]])})
    sio.savemat(str(tmp_path / "Plane1.mat"), {"P": plane.reshape(4, 1)})
    got_obs, got_bb, got_res, got_plane = dtu.read_obs_mask(str(tmp_path / "ObsMask1_10.mat"), str(tmp_path / "Plane1.mat"))
    assert got_obs.dtype == np.uint8 and got_obs.tobytes() == obs.tobytes() and got_obs.shape == obs.shape
    assert got_bb.dtype == F32 and got_bb.tobytes() == bb.tobytes() and got_res == 0.7
    assert got_plane.dtype == np.float64 and got_plane.tobytes() == plane.tobytes()
    sio.savemat(str(tmp_path / "Empty.mat"), {"BB": bb})
    with pytest.raises(ValueError, match="ObsMask"):
        dtu.read_obs_mask(str(tmp_path / "Empty.mat"), str(tmp_path / "Plane1.mat"))


def test_product_code_imports_neither_scipy_nor_the_tests():
    src = open(os.path.join(ROOT, "ibgs_amd", "dtu.py")).read()
    assert not re.search(r"^(import|from)\s+(scipy|sklearn|oracle|tests|cv2|skimage|trimesh)\b", src, re.M)          # (scipy.io: inside read_obs_mask only)
    assert re.search(r"^\s+from scipy\.io import loadmat", src, re.M)
