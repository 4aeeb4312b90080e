"""The mesh-evaluation unit on a CPU-only box: the host restatement of its contract (tests/mesh_eval_ref.py) against what the reference's own code computed
(tests/golden/mesh_eval.npz, frozen by tests/golden/make_mesh_eval_fixture.py), the kd-tree restatement against the literal one, the C ABI
(include/ibgs_mesh_eval.h <-> _lib.MESH_EVAL_EXPORTS <-> the built library) and the argument checks of ibgs_amd.mesh_eval, which run before any GPU work."""
import os
import re
import types

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, mesh_eval
from tests import mesh_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_BAND, FLOOR_BAND, SUM_BAND = 1e-5, 1e-9, 1e-9          # the band condition (see the fixture generator)
D2_RTOL = 4 * 2.0 ** -24          # rounding of the f32 d2 formula: three subtractions, three products, two sums, each 2^-24


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "mesh_eval.npz"))


def test_fixture_is_small(fx):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mesh_eval.npz")) <= 600 * 1024


def test_band_condition_holds_on_the_fixture(fx):
    assert fx["pair_margin"] >= PAIR_BAND and fx["floor_margin"] >= FLOOR_BAND and fx["sum_margin"] >= SUM_BAND
    # ... and recomputed here from the stored inputs
    _, _, m = ref.sample_surface(fx["vertices"], fx["faces"], float(fx["density"]))
    assert m["floor_margin"] >= FLOOR_BAND and m["sum_margin"] >= SUM_BAND
    assert ref.pair_margin(fx["sample_points"].astype(np.float32), float(fx["density"])) >= PAIR_BAND


def test_sampling_restates_the_reference(fx):
    pts, counts, _ = ref.sample_surface(fx["vertices"], fx["faces"], float(fx["density"]))
    np.testing.assert_array_equal(counts, fx["sample_counts"])
    assert pts.shape == fx["sample_points"].shape and counts.sum() > 1000 and (counts == 0).sum() >= 3
    scale = np.abs(fx["sample_points"]).max()
    assert np.abs(pts - fx["sample_points"]).max() <= 8 * 2.0 ** -52 * scale          # f64 round-off of two products and two sums
    np.testing.assert_array_equal(pts[:len(fx["vertices"])], fx["vertices"].astype(np.float64))


@pytest.mark.parametrize("thin", [ref.downsample, ref.downsample_brute])
def test_thinning_restates_the_sklearn_loop(fx, thin):
    cloud, r = fx["sample_points"].astype(np.float32), float(fx["density"])
    np.testing.assert_array_equal(thin(cloud, r, fx["order"]), fx["keep"])
    np.testing.assert_array_equal(thin(cloud, r), fx["keep_index_order"])
    assert 0 < fx["keep"].sum() < len(cloud) and np.any(fx["keep"] != fx["keep_index_order"])


@pytest.mark.parametrize("nn", [ref.nearest, ref.nearest_brute])
def test_nearest_restates_the_kd_tree(fx, nn):
    cloud, gt, md = fx["sample_points"].astype(np.float32)[fx["keep"]], fx["gt"], float(fx["max_dist"])
    for q, t, dist, idx in ((cloud, gt, fx["dist_d2s"], fx["index_d2s"]), (gt, cloud, fx["dist_s2d"], fx["index_s2d"])):
        d, i = nn(q, t, md)
        near = dist < md * (1 - 1e-6)
        assert near.sum() > 100 and np.all(np.isinf(d[dist > md * (1 + 1e-6)]))
        # d = sqrt(d2): half the relative error of d2, plus the root's own rounding
        rel = np.abs(d[near].astype(np.float64) - dist[near]) / dist[near]
        assert rel.max() <= D2_RTOL, rel.max()
        same = i[near] == idx[near]          # where the indices differ the two candidates are equally near to within the same bound
        other = np.sqrt(((q[near][~same].astype(np.float64) - t[idx[near][~same]].astype(np.float64)) ** 2).sum(1))
        assert np.all(np.abs(other - dist[near][~same]) <= D2_RTOL * dist[near][~same])
    c = ref.chamfer(cloud, gt, md, nn=nn)
    assert abs(c["mean_d2s"] - float(fx["mean_d2s"])) <= D2_RTOL * float(fx["mean_d2s"])
    assert abs(c["mean_s2d"] - float(fx["mean_s2d"])) <= D2_RTOL * float(fx["mean_s2d"])
    assert c["n_d2s"] == int((fx["dist_d2s"] < md).sum()) and c["n_s2d"] == int((fx["dist_s2d"] < md).sum())


def test_the_two_restatements_agree_on_small_clouds():
    rng = np.random.default_rng(2)
    for seed, n, r in ((1, 700, 0.08), (2, 1500, 0.05), (3, 400, 0.3)):
        p = ref.surface_cloud(n, seed, noise=0.02)
        dup = np.arange(0, n - 1, 7)
        p[dup] = p[dup + 1]          # duplicates
        for order in (None, rng.permutation(n), np.argsort(p[:, 0], kind="stable")):
            a, b = ref.downsample(p, r, order), ref.downsample_brute(p, r, order)
            np.testing.assert_array_equal(a, b)
            kept = p[a]          # independent and maximal
            d2 = ref.d2_f32(kept[:, None], kept[None])
            np.fill_diagonal(d2, np.inf)
            assert np.all(d2 > np.float32(r) * np.float32(r))
            assert np.all(ref.d2_f32(p[~a][:, None], kept[None]).min(1) <= np.float32(r) * np.float32(r))
        q = ref.surface_cloud(500, seed + 10, noise=0.3)
        q[:50] += 5.0          # beyond max_dist
        q[50:60] = p[:10]          # on a target (and on its duplicate)
        for md in (0.05, 0.5, 10.0):
            d1, i1 = ref.nearest(q, p, md)
            d2_, i2 = ref.nearest_brute(q, p, md)
            assert d1.tobytes() == d2_.tobytes()
            np.testing.assert_array_equal(i1, i2)
            if md <= 0.5:
                assert np.all(np.isinf(d1[:50])) and np.all(i1[:50] == -1)
    d, i = ref.nearest(q, np.zeros((0, 3), np.float32), 1.0)
    assert np.all(np.isinf(d)) and np.all(i == -1)
    c = ref.chamfer(np.zeros((0, 3), np.float32), p, 1.0)
    assert np.isnan(c["mean_d2s"]) and np.isnan(c["mean_s2d"]) and c["n_d2s"] == 0 and c["n_s2d"] == 0
    assert ref.fscore(np.zeros((0, 3), np.float32), p, 0.1)["fscore"] == 0.0


def test_sampling_closed_forms():
    # a right triangle with legs L: thr = density, n1 = n2 = n = floor(L / density); a + b < 1 <=> i + j + 1 < n: n (n - 1) / 2 samples
    for L, dens in ((1.0, 0.3), (2.0, 0.3), (1.0, 0.07)):
        v = np.array([[0, 0, 0], [L, 0, 0], [0, L, 0]], np.float32)
        pts, counts, _ = ref.sample_surface(v, np.array([[0, 1, 2]], np.int32), dens, include_vertices=False)
        n = int(np.floor(np.float64(np.float32(L)) / dens))
        assert counts[0] == n * (n - 1) // 2 == len(pts)
        assert np.all(pts[:, 2] == 0) and np.all(pts[:, 0] + pts[:, 1] < L) and np.all(np.diff(pts[:, 0]) >= 0)          # i-major


def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_mesh_eval.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_meval_[a-z_0-9]+)\s*\(", text)))
    assert len(names) == 9
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.MESH_EVAL_EXPORTS) == names
    defines = re.findall(r"#define\s+IBGS_(MEVAL_[A-Z_]+)\s+(\d+)", text)
    assert len(defines) >= 10
    for name, val in defines:
        assert getattr(_lib, name) == int(val), name


def test_kernels_attributed_to_the_mesh_eval_unit():
    src = open(os.path.join(ROOT, "ibgs_amd", "csrc", "mesh_eval.hip")).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)
    assert len(kernels) >= 8 and all(k.startswith("meval_") for k in kernels), kernels
    for k in kernels:
        assert _build.tu_of(k) == "mesh_eval", k
    assert _build.tu_of("meval_cell_count") == "mesh_eval" and _build.KERNEL_TU[0] == ("meval_", "mesh_eval")
    assert "mesh_eval" in _build.SOURCES and "mesh_eval" in _build.UNIT_HEADERS and "mesh_eval" in _build.tu_shas()
    assert "-ffp-contract=off" in _build.EXTRA["mesh_eval"]
    assert _build.tu_of("mesh_label_kernel") == "mesh" and _build.tu_of("cell_count_kernel") == "binning"


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need_s, need_t = built_lib.ibgs_meval_required_sample_scratch, built_lib.ibgs_meval_required_tree
    assert need_s(0) > 0 and need_s(10 ** 6) >= 4 * 10 ** 6 and need_s(-1) == 0 and need_s(1 << 30) == 0
    assert need_t(0) == 0 and need_t(-3) == 0 and need_t(1 << 31) == 0 and need_t(1) > 0
    assert 16 * 10 ** 6 < need_t(10 ** 6) < 24 * 10 ** 6 and need_t((1 << 31) - 1) > 0
    err = lambda: built_lib.ibgs_last_error()
    assert built_lib.ibgs_meval_sample_count(None, 3, -1, None, None, 0.2, None, 0, None, None) < 0 and b"out of range" in err()
    assert built_lib.ibgs_meval_sample_count(None, 3, 1, 128, 128, 0.0, 128, 1 << 20, 128, 128) < 0 and b"density" in err()
    assert built_lib.ibgs_meval_sample_count(None, 3, 1, None, None, 0.2, None, 0, None, None) < 0 and b"null" in err()
    assert built_lib.ibgs_meval_sample_count(None, 3, 1, 128, 128, 0.2, 64, 1 << 20, 128, 128) < 0 and b"aligned" in err()
    assert built_lib.ibgs_meval_sample_emit(None, 3, 1, 128, 128, 0.2, 128, 16, 0, None, 128) < 0 and b"needed" in err()
    assert built_lib.ibgs_meval_build(None, 0, 128, 128, None, 128, 1 << 20, 128) < 0 and b"out of range" in err()
    assert built_lib.ibgs_meval_build(None, 10, 128, 128, None, 128, 16, 128) < 0 and b"needed" in err()
    assert built_lib.ibgs_meval_thin_rounds(None, 10, 128, 1 << 20, -1.0, 128, 1, 128) < 0 and b"radius" in err()
    assert built_lib.ibgs_meval_thin_rounds(None, 10, 128, 1 << 20, 1.0, 128, 0, 128) < 0 and b"rounds" in err()
    assert built_lib.ibgs_meval_nearest(None, 5, 128, None, 10, 128, 1 << 20, float("nan"), 128, 128, 128) < 0 and b"max_dist" in err()
    assert built_lib.ibgs_meval_nearest(None, 5, None, None, 10, 128, 1 << 20, 1.0, None, None, None) < 0 and b"null" in err()
    assert built_lib.ibgs_meval_keys(None, 5, None, None, None, None) < 0 and built_lib.ibgs_meval_reduce(None, 5, None, 1.0, None, None) < 0


def _cpu_mesh(V=5, F=3):
    return types.SimpleNamespace(vertices=torch.zeros(V, 3), faces=torch.zeros(F, 3, dtype=torch.int32))


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    p = torch.zeros(6, 3)
    calls = {"sample_surface": lambda: mesh_eval.sample_surface(_cpu_mesh(), 0.2), "downsample": lambda: mesh_eval.downsample(p, 0.2),
             "nearest": lambda: mesh_eval.nearest(p, p, 1.0), "chamfer": lambda: mesh_eval.chamfer(p, p, 1.0), "fscore": lambda: mesh_eval.fscore(p, p, 0.1),
             "evaluate_mesh": lambda: mesh_eval.evaluate_mesh(_cpu_mesh(), p)}
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn()
    for bad in (torch.zeros(6, 3, dtype=torch.float64), torch.zeros(6, 4), torch.zeros(18), torch.zeros(2, 3, 3)):
        for fn in (lambda b: mesh_eval.downsample(b, 0.2), lambda b: mesh_eval.nearest(b, p, 1.0), lambda b: mesh_eval.nearest(p, b, 1.0),
                   lambda b: mesh_eval.chamfer(b, p, 1.0), lambda b: mesh_eval.chamfer(p, b, 1.0), lambda b: mesh_eval.fscore(b, p, 0.1),
                   lambda b: mesh_eval.evaluate_mesh(_cpu_mesh(), b)):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (lambda: mesh_eval.downsample(np.zeros((6, 3), np.float32), 0.2), lambda: mesh_eval.nearest(p, [[0, 0, 0]], 1.0),
               lambda: mesh_eval.sample_surface((1, 2), 0.2), lambda: mesh_eval.sample_surface(types.SimpleNamespace(vertices=np.zeros((3, 3)), faces=p), 0.2),
               lambda: mesh_eval.downsample(p, "wide")):
        with pytest.raises(TypeError):
            fn()
    ok = _cpu_mesh()
    for bad in (types.SimpleNamespace(vertices=ok.vertices, faces=torch.zeros(3, 3, dtype=torch.int64)),
                types.SimpleNamespace(vertices=ok.vertices, faces=torch.zeros(3, 4, dtype=torch.int32)),
                types.SimpleNamespace(vertices=torch.zeros(5, 3, dtype=torch.float64), faces=ok.faces),
                types.SimpleNamespace(vertices=torch.zeros(15), faces=ok.faces)):
        with pytest.raises(ValueError):
            mesh_eval.sample_surface(bad, 0.2)
    for kw in (dict(density=0.0), dict(density=-1.0), dict(density=float("nan")), dict(density=float("inf")), dict(density=0.2, max_points=-1)):
        with pytest.raises(ValueError):
            mesh_eval.sample_surface(ok, **kw)
    for fn in (lambda: mesh_eval.downsample(p, -0.1), lambda: mesh_eval.downsample(p, float("inf")), lambda: mesh_eval.nearest(p, p, -1.0),
               lambda: mesh_eval.nearest(p, p, float("nan")), lambda: mesh_eval.chamfer(p, p, -2.0), lambda: mesh_eval.fscore(p, p, 0.0),
               lambda: mesh_eval.evaluate_mesh(ok, p, max_dist=-1.0), lambda: mesh_eval.evaluate_mesh(ok, p, tau=0.0)):
        with pytest.raises(ValueError):
            fn()


def test_product_code_imports_neither_scipy_nor_the_tests():
    src = open(os.path.join(ROOT, "ibgs_amd", "mesh_eval.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn|oracle|tests)\b", src, re.M)
