"""The mesh post-processing unit on a CPU-only box: the two host restatements of its contract (tests/mesh_ref.py) against each other and against
closed forms, the C ABI (include/ibgs_mesh.h <-> _lib.MESH_EXPORTS <-> the built library), the argument checks of ibgs_amd.mesh, which run before any
GPU work, and a PLY round trip of a filtered mesh."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, mesh, ply, tsdf
from tests import mesh_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixtures():
    v3, f3 = ref.fan(3000, 40)
    return {"case1": ref.case1(), "case1_unpermuted": ref.case1(permuted=False), "fan": ref.permute(v3, f3, 2), "strip": ref.permute(*ref.strip(4000), 3)}


def _floater_mesh():
    """Case 2 on the host: the numpy TSDF restatement + the library's marching-cubes table."""
    from tests import tsdf_ref
    vol = tsdf_ref.RefVolume(0.02, 0.08)
    for dep, col, M, k in ref.floater_frames():
        vol.integrate(dep, *k, M, color=col)
    tab = (ctypes.c_int32 * 4096)()
    assert _lib.load().ibgs_tsdf_mc_table(tab) == 0
    v, f, c, n = tsdf_ref.marching_cubes(vol.blocks(), 0.02, np.array(tab))
    return v, f


@pytest.mark.parametrize("name", ["case1", "case1_unpermuted", "fan", "strip"])
def test_the_two_restatements_agree(name):
    v, f = _fixtures()[name]
    a, b = ref.cluster(v, f), ref.cluster_bfs(v, f)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_allclose(a[2], b[2], rtol=1e-12, atol=0)
    assert a[1].sum() == len(f) and np.all(np.diff(np.unique(a[0], return_index=True)[1]) > 0)          # numbered by first appearance


def test_case1_counts_and_survivors():
    v, f = ref.case1()
    lab, counts, _ = ref.cluster(v, f)
    assert len(f) == 16065 and sorted(counts.tolist(), reverse=True) == ref.CASE1_COUNTS
    for k in range(1, 12):
        rows, fo = ref.post_process(f, len(v), lab, counts, k)
        assert len(fo) == ref.CASE1_KEPT[min(k, 5)], k
        assert len(np.unique(fo)) == len(rows)          # (no degenerate survivor here: every kept vertex is referenced)
    with pytest.raises(ValueError):
        ref.post_process(f, len(v), lab, counts, 12)
    # min_triangles = 1: the degenerate pair survives the cluster filter, keeps its three vertices and then loses both triangles
    rows, fo = ref.post_process(f, len(v), lab, counts, 11, min_triangles=1)
    assert len(fo) == 16065 - 2 and len(rows) == len(v) - 1 and len(np.unique(fo)) == len(rows) - 3
    assert len(ref.clean(f, lab, counts, 45)) == 9323 + 2 * 3042 + 522 + 50 and len(ref.clean(f, lab, counts, 1000)) == 9323 + 2 * 3042


def test_fused_floaters_on_the_host():
    v, f = _floater_mesh()
    lab, counts, _ = ref.cluster(v, f)
    lab2, counts2, _ = ref.cluster_bfs(v, f)
    np.testing.assert_array_equal(lab, lab2)
    np.testing.assert_array_equal(counts, counts2)
    assert (len(v), len(f)) == (13480, 26913) and sorted(counts.tolist(), reverse=True) == [24052, 1160, 780, 545, 360, 8, 8]
    rows, fo = ref.post_process(f, len(v), lab, counts, 1)
    assert (len(rows), len(fo)) == (12028, 24052)          # the sphere-only mesh of tests/test_gpu_tsdf.py
    e = np.sort(np.concatenate([fo[:, [0, 1]], fo[:, [1, 2]], fo[:, [2, 0]]]).astype(np.int64), axis=1)
    assert len(rows) - len(np.unique(e[:, 0] * len(rows) + e[:, 1])) + len(fo) == 2
    d = np.abs(np.linalg.norm(v[rows].astype(np.float64), axis=1) - 0.5) / 0.02
    assert d.max() <= 0.52
    assert len(ref.post_process(f, len(v), lab, counts, 7)[1]) == 26913 - 16


def test_closed_forms_of_disjoint_grids():
    sizes, h = [(7, 3), (2, 2), (12, 9), (3, 30), (2, 5)], 0.125
    v, f = ref.join([ref.grid(n, m, h, origin=(10.0 * k, 0, 0)) for k, (n, m) in enumerate(sizes)])
    for cl in (ref.cluster, ref.cluster_bfs):
        lab, counts, areas = cl(v, f)
        assert counts.tolist() == [2 * (n - 1) * (m - 1) for n, m in sizes]
        np.testing.assert_allclose(areas, [(n - 1) * (m - 1) * h * h for n, m in sizes], rtol=1e-13)
        assert np.all(np.diff(lab) >= 0)


def test_strips_and_fans():
    v, f, lengths = ref.cut_strip(5000, 25, seed=1)
    assert ref.cluster(v, f)[1].tolist() == lengths.tolist()
    v, f = ref.fan(500, 30)
    lab, counts, _ = ref.cluster(v, f)
    assert counts.tolist() == [500] + [1] * 30          # a shared vertex does not connect


def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_mesh.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_mesh_[a-z_0-9]+)\s*\(", text)))
    assert len(names) == 5
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.MESH_EXPORTS) == names
    assert built_lib.ibgs_mesh_sizeof_mesh() == ctypes.sizeof(_lib.Mesh)
    for name, val in re.findall(r"#define\s+IBGS_(MESH_[A-Z_]+)\s+(\d+)", text):
        assert getattr(_lib, name) == int(val), name


def test_kernels_attributed_to_the_mesh_unit():
    src = open(os.path.join(ROOT, "ibgs_amd", "csrc", "mesh.hip")).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)
    assert len(kernels) >= 6 and all(k.startswith("mesh_") for k in kernels), kernels
    for k in kernels:
        assert _build.tu_of(k) == "mesh", k
    assert "mesh" in _build.SOURCES and "mesh" in _build.UNIT_HEADERS and "mesh" in _build.tu_shas()
    assert _build.tu_of("tsdf_mc_emit_kernel") == "tsdf"


def test_scratch_size_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_mesh_required_scratch
    assert need(0, 0) > 0 and need(1000, 2000) > 2000 * 6 * 16
    assert need(10 ** 6, 2 * 10 ** 6) >= need(10 ** 6, 10 ** 6) >= need(10, 10 ** 6)
    assert need(-1, 5) == 0 and need(5, -1) == 0 and need(1 << 31, 5) == 0 and need(5, 1 << 30) == 0
    assert need((1 << 31) - 1, (1 << 30) - 1) > 0
    m = _lib.Mesh()
    assert built_lib.ibgs_mesh_cluster(None, None, None, None, None) < 0
    m.V, m.F = 4, -1
    assert built_lib.ibgs_mesh_cluster(None, ctypes.byref(m), None, None, None) < 0
    assert b"out of range" in built_lib.ibgs_last_error()
    m.F = 2
    assert built_lib.ibgs_mesh_cluster(None, ctypes.byref(m), None, None, None) < 0
    assert b"null" in built_lib.ibgs_last_error()
    m.vertices = m.faces = m.state = 128
    m.scratch, m.scratch_bytes = 64, 1 << 30          # (never dereferenced: the alignment check fails first)
    assert built_lib.ibgs_mesh_filter_count(None, ctypes.byref(m), None, None, 1, 0) < 0
    assert b"aligned" in built_lib.ibgs_last_error()
    m.scratch, m.scratch_bytes = 128, 16
    assert built_lib.ibgs_mesh_filter_emit(None, ctypes.byref(m), 0, 0, 0, None, 0, None, None) < 0
    assert b"needed" in built_lib.ibgs_last_error()


def _cpu_mesh(V=5, F=3):
    return tsdf.TriangleMesh(torch.zeros(V, 3), torch.zeros(F, 3, dtype=torch.int32), torch.zeros(V, 3), torch.zeros(V, 3))


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    for fn in (mesh.cluster_connected_triangles, mesh.post_process_mesh, mesh.clean_mesh):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(_cpu_mesh())
        with pytest.raises(TypeError):
            fn((1, 2, 3))
        with pytest.raises(TypeError):
            fn(_cpu_mesh()._replace(faces=np.zeros((3, 3), np.int32)))
    ok = _cpu_mesh()
    for bad in (ok._replace(faces=torch.zeros(3, 3, dtype=torch.int64)), ok._replace(faces=torch.zeros(3, 4, dtype=torch.int32)),
                ok._replace(vertices=torch.zeros(5, 3, dtype=torch.float64)), ok._replace(vertices=torch.zeros(15)),
                ok._replace(colors=torch.zeros(4, 3)), ok._replace(normals=torch.zeros(6, 3))):
        for fn in (mesh.cluster_connected_triangles, mesh.post_process_mesh, mesh.clean_mesh):
            with pytest.raises(ValueError):
                fn(bad)
    for k in (0, -3):
        with pytest.raises(ValueError, match="cluster_to_keep"):
            mesh.post_process_mesh(ok, cluster_to_keep=k)


def test_product_code_imports_neither_scipy_nor_the_tests():
    src = open(os.path.join(ROOT, "ibgs_amd", "mesh.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|oracle|tests)\b", src, re.M)


def test_ply_round_trip_of_a_filtered_mesh(tmp_path):
    v, f = ref.case1()
    c, n = ref.attributes(v)
    n = np.nan_to_num(n)
    lab, counts, _ = ref.cluster(v, f)
    rows, fo = ref.post_process(f, len(v), lab, counts, 4)
    out = tsdf.TriangleMesh(torch.as_tensor(v[rows]), torch.as_tensor(fo), torch.as_tensor(c[rows]), torch.as_tensor(n[rows]))
    path = str(tmp_path / "post.ply")
    ply.save_mesh(path, out)
    back = ply.load_mesh(path)
    np.testing.assert_array_equal(back["faces"], fo)
    assert back["vertices"].tobytes() == v[rows].tobytes() and back["normals"].tobytes() == n[rows].tobytes()
    np.testing.assert_array_equal(back["colors"], np.floor(255.0 * c[rows].astype(np.float64) + 0.5).astype(np.uint8))
    assert len(back["faces"]) == ref.CASE1_KEPT[4] and back["faces"].max() == len(rows) - 1
