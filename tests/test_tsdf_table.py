"""The TSDF unit's C ABI on a CPU-only box (no compute: the library only loads) and its marching-cubes table, checked over all 256 cases:
empty extremes, closed sheets (every interior triangle edge shared by exactly two triangles in opposite directions), crack-free faces (the
boundary segments on a cube face depend on that face's four signs alone, and the opposite face of the neighbouring cell draws them reversed)
and orientation towards the non-negative corners."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from ibgs_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])


def edge_corners(e):
    a, k = divmod(e, 4)
    b, c = [x for x in range(3) if x != a]
    off = [0, 0, 0]
    off[b] = k & 1
    off[c] = k >> 1
    c0 = off[0] | off[1] << 1 | off[2] << 2
    return c0, c0 | (1 << a)


def edge_faces(e):
    """The two cube faces (axis, side) an edge lies on."""
    c0, c1 = edge_corners(e)
    return {(ax, int(CORNERS[c0][ax])) for ax in range(3) if CORNERS[c0][ax] == CORNERS[c1][ax]}


@pytest.fixture(scope="module")
def table(built_lib):
    out = (ctypes.c_int32 * (256 * 16))()
    assert built_lib.ibgs_tsdf_mc_table(out) == 0
    t = np.array(out, np.int64).reshape(256, 16)
    return [[tuple(int(x) for x in t[c, 3 * i:3 * i + 3]) for i in range(5) if t[c, 3 * i] >= 0] for c in range(256)], t


def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_tsdf.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_tsdf_[a-z_0-9]+)\s*\(", text)))
    assert len(names) == 7
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.TSDF_EXPORTS) == names
    assert built_lib.ibgs_tsdf_sizeof_volume() == ctypes.sizeof(_lib.TsdfVolume)
    assert built_lib.ibgs_tsdf_sizeof_view() == ctypes.sizeof(_lib.TsdfView)
    assert built_lib.ibgs_tsdf_sizeof_mesh_scratch() == ctypes.sizeof(_lib.TsdfMeshScratch)


def test_kernels_attributed_to_the_tsdf_unit():
    src = open(os.path.join(ROOT, "ibgs_amd", "csrc", "tsdf.hip")).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)
    assert len(kernels) == 5 and all(k.startswith("tsdf_") for k in kernels), kernels
    for k in kernels:
        assert _build.tu_of(k) == "tsdf", k
    assert "tsdf" in _build.SOURCES and _build.EXTRA["tsdf"] == ["-ffp-contract=off"]
    assert _build.tu_of("tsdf_mc_scan_kernel") == "tsdf"          # not scan_sort through "scan_"


def test_validation_before_any_gpu_work(built_lib):
    vol, view = _lib.TsdfVolume(), _lib.TsdfView()
    assert built_lib.ibgs_tsdf_integrate(None, None, ctypes.byref(view), None, None, 0) < 0
    assert built_lib.ibgs_tsdf_integrate(None, ctypes.byref(vol), ctypes.byref(view), None, None, 0) < 0
    assert b"voxel_length" in built_lib.ibgs_last_error()
    vol.voxel_length, vol.sdf_trunc, vol.capacity, vol.slot_bits = 0.01, 0.04, 16, 5
    for f in ("slot_key", "slot_block", "slot_mark", "active", "block_key", "tsdf", "weight", "color", "state"):
        setattr(vol, f, 64)          # (never dereferenced: the view check fails first)
    view.W, view.H, view.fx, view.fy = 8, 8, 10.0, 10.0
    view.world_to_camera[0] = float("nan")
    assert built_lib.ibgs_tsdf_integrate(None, ctypes.byref(vol), ctypes.byref(view), ctypes.c_void_p(64), None, 0) < 0
    assert b"pose" in built_lib.ibgs_last_error()
    assert built_lib.ibgs_tsdf_mesh_emit(None, ctypes.byref(vol), None, 0, 0, None, None, None, None) < 0


def test_extreme_cases_empty(table):
    tris, _ = table
    assert tris[0] == [] and tris[255] == []
    assert all(len(t) >= 1 for t in tris[1:255])


def test_triangles_use_exactly_the_crossing_edges(table):
    tris, raw = table
    for case in range(256):
        neg = [(case >> c) & 1 for c in range(8)]
        crossing = {e for e in range(12) if neg[edge_corners(e)[0]] != neg[edge_corners(e)[1]]}
        used = {e for t in tris[case] for e in t}
        assert used == crossing, case
        assert all(len(set(t)) == 3 for t in tris[case]), case
        assert np.all(raw[case, 3 * len(tris[case]):] == -1), case


def test_interior_edges_shared_twice_in_opposite_directions(table):
    tris, _ = table
    for case in range(256):
        directed = [(t[i], t[(i + 1) % 3]) for t in tris[case] for i in range(3)]
        for a, b in directed:
            if edge_faces(a) & edge_faces(b):
                continue          # both ends on one cube face: a boundary segment or a diagonal lying on the face
            assert directed.count((a, b)) == 1 and directed.count((b, a)) == 1, (case, a, b)
        for a, b in set(directed):          # a diagonal on a face is interior too: it must come back reversed
            if directed.count((a, b)) + directed.count((b, a)) > 1:
                assert directed.count((a, b)) == 1 and directed.count((b, a)) == 1, (case, a, b)


def boundary_segments(tri_list):
    """Directed triangle edges whose reverse is absent (the sheet's boundary on the cube's faces)."""
    directed = [(t[i], t[(i + 1) % 3]) for t in tri_list for i in range(3)]
    return {(a, b) for a, b in directed if (b, a) not in directed}


def face_pattern(case, axis, side):
    fc = [c for c in range(8) if CORNERS[c][axis] == side]
    return tuple((case >> c) & 1 for c in fc)


def test_face_segments_depend_on_the_face_pattern_alone(table):
    tris, _ = table
    segs_of = {}
    for case in range(256):
        bnd = boundary_segments(tris[case])
        for a, b in bnd:
            assert edge_faces(a) & edge_faces(b), (case, a, b)          # every boundary segment lies on a face
        for axis, side in itertools.product(range(3), range(2)):
            on = frozenset((a, b) for a, b in bnd if (axis, side) in (edge_faces(a) & edge_faces(b)))
            key = (axis, side, face_pattern(case, axis, side))
            assert segs_of.setdefault(key, on) == on, (case, axis, side)
    # 16 patterns per face, each seen; the neighbour across a face draws the same segments reversed
    for axis in range(3):
        assert len([k for k in segs_of if k[:2] == (axis, 0)]) == 16
        for pattern in itertools.product(range(2), repeat=4):
            lo, hi = segs_of[(axis, 0, pattern)], segs_of[(axis, 1, pattern)]

            def to_low(e):          # the edge of face (axis, 1) as the edge of the neighbour's face (axis, 0)
                c0, c1 = edge_corners(e)
                c0 &= ~(1 << axis); c1 &= ~(1 << axis)
                return next(f for f in range(12) if set(edge_corners(f)) == {c0, c1})

            assert {(to_low(b), to_low(a)) for a, b in hi} == set(lo), (axis, pattern)


def test_orientation_towards_the_non_negative_corners(table):
    tris, _ = table
    mid = lambda e: 0.5 * (CORNERS[edge_corners(e)[0]] + CORNERS[edge_corners(e)[1]])
    for case in range(256):
        for t in tris[case]:
            p = [mid(e) for e in t]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            assert np.linalg.norm(n) > 0, (case, t)
            for e in t:
                c0, c1 = edge_corners(e)
                pos, neg = (c1, c0) if (case >> c0) & 1 else (c0, c1)
                assert np.dot(n, CORNERS[pos] - CORNERS[neg]) >= 0, (case, t, e)
            s = sum(np.dot(n, CORNERS[c1] - CORNERS[c0]) * (1 if (case >> c0) & 1 else -1) for c0, c1 in map(edge_corners, t))
            assert s > 0, (case, t)


def test_table_is_what_the_generator_derives(table):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    _, raw = table
    np.testing.assert_array_equal(np.array(gen.table()), raw)
