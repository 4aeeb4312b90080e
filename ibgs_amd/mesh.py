"""Triangle-mesh post-processing on the MI355X: the reference's `post_process_mesh(mesh, num_cluster)` and `clean_mesh(mesh, min_len)`
(render.py:34-66), which run Open3D's host-side `cluster_connected_triangles`, `remove_triangles_by_mask`, `remove_unreferenced_vertices` and
`remove_degenerate_triangles` and cannot be run where Open3D has no build.  With tsdf.TSDFVolume this gives both mesh files of `render.py --render_geo`:

    raw = volume.extract_mesh()
    ply.save_mesh(path, raw)                                             # tsdf_fusion.ply
    ply.save_mesh(path_post, mesh.post_process_mesh(raw, num_cluster))   # tsdf_fusion_post.ply

The contract is this project's own statement of those routines ("Mesh post-processing"; header of ibgs_amd/csrc/mesh.hip);
tests/mesh_ref.py restates it twice.  Any indexed mesh is accepted, not only marching-cubes output: unreferenced vertices, edges shared by any number of
triangles, vertices of any degree, triangles that repeat an index.  Labels, counts and output meshes are a pure function of the input (bit-identical from
run to run); `cluster_area` is summed with f64 atomics and may differ in its last bits.

HIP only (C ABI include/ibgs_mesh.h): CPU tensors are refused, every argument is checked before any GPU work, every kernel runs on torch's current stream.
Each call reads a few counters back (it waits for the stream): the docstrings say which."""
import ctypes
from typing import NamedTuple

import torch

from . import _device, _lib
from .tsdf import TriangleMesh

MAX_FACES = (1 << 30) - 1
MAX_VERTICES = (1 << 31) - 1


class TriangleClusters(NamedTuple):
    triangle_clusters: torch.Tensor          # (F,) int32: cluster of every triangle, clusters numbered by ascending smallest triangle index
    cluster_n_triangles: torch.Tensor        # (C,) int32
    cluster_area: torch.Tensor               # (C,) f64: sum of 0.5 |(p1 - p0) x (p2 - p0)|, evaluated in f64 from the f32 vertices


class MeshError(RuntimeError):
    pass


def _check(mesh):
    """(V, F, device) of a valid device mesh; raises before anything touches the GPU."""
    try:
        v, f, c, n = mesh.vertices, mesh.faces, mesh.colors, mesh.normals
    except AttributeError:
        raise TypeError("mesh must be a tsdf.TriangleMesh (vertices, faces, colors, normals), got %s" % type(mesh).__name__) from None
    for name, t in (("vertices", v), ("faces", f), ("colors", c), ("normals", n)):
        if not torch.is_tensor(t):
            raise TypeError("mesh.%s must be a tensor, got %s" % (name, type(t).__name__))
    for name, t in (("vertices", v), ("colors", c), ("normals", n)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("mesh.%s must be (V, 3) float32, got %s %s" % (name, tuple(t.shape), t.dtype))
    if f.dtype != torch.int32 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("mesh.faces must be (F, 3) int32, got %s %s" % (tuple(f.shape), f.dtype))
    V, F = int(v.shape[0]), int(f.shape[0])
    if c.shape[0] != V or n.shape[0] != V:
        raise ValueError("mesh.colors / mesh.normals must have one row per vertex (%d), got %d / %d" % (V, c.shape[0], n.shape[0]))
    if F > MAX_FACES or V > MAX_VERTICES:
        raise ValueError("mesh too large: V %d, F %d (limits: V < 2^31, F < 2^30)" % (V, F))
    for name, t in (("vertices", v), ("faces", f), ("colors", c), ("normals", n)):
        _device.refuse_cpu("mesh", "mesh." + name, t)
    if any(t.device != v.device for t in (f, c, n)):
        raise ValueError("the mesh's tensors are on different devices")
    return V, F, v.device


class _Run:
    """One mesh's C struct with its scratch and state (fresh per call: the library keeps nothing)."""

    def __init__(self, mesh, V, F, dev):
        self.lib = _lib.load()
        self.V, self.F, self.dev = V, F, dev
        self.vertices, self.faces = mesh.vertices.contiguous(), mesh.faces.contiguous()
        nbytes = self.lib.ibgs_mesh_required_scratch(V, F)
        if nbytes == 0:
            raise ValueError("mesh too large: V %d, F %d" % (V, F))
        self.scratch, self.state = _device.scratch(dev, nbytes), _device.zeros_state(dev, _lib.MESH_STATE_WORDS)
        m = _lib.Mesh()
        m.V, m.F, m.vertices, m.faces = V, F, self.vertices.data_ptr(), self.faces.data_ptr()
        m.scratch, m.scratch_bytes, m.state = self.scratch.data_ptr(), nbytes, self.state.data_ptr()
        self.c = m

    def call(self, name, *args):
        _device.call(self.dev, name, ctypes.byref(self.c), *args)

    def counters(self):
        s = self.state.cpu().tolist()          # (waits for the stream)
        if s[_lib.MESH_BAD_FACES]:
            raise MeshError("mesh.faces holds %d triangle(s) with a vertex index outside [0, %d)" % (s[_lib.MESH_BAD_FACES], self.V))
        if s[_lib.MESH_TABLE_FULL] or s[_lib.MESH_OVERRUN]:
            raise MeshError("mesh library fault: %d edge(s) found no table slot, %d emit(s) out of range" % (s[_lib.MESH_TABLE_FULL], s[_lib.MESH_OVERRUN]))
        return s

    def cluster(self):
        """labels (F,), counts and areas (F,: the first C are meaningful), C.  Reads the state back once."""
        with torch.cuda.device(self.dev):
            labels = torch.empty(self.F, dtype=torch.int32, device=self.dev)
            counts = torch.empty(self.F, dtype=torch.int32, device=self.dev)
            areas = torch.empty(self.F, dtype=torch.float64, device=self.dev)
        self.call("ibgs_mesh_cluster", labels.data_ptr(), counts.data_ptr(), areas.data_ptr())
        C = self.counters()[_lib.MESH_CLUSTERS]
        return labels, counts[:C], areas[:C], C

    def filter(self, mesh, labels, keep_cluster, C, flags):
        """(faces', [vertices', colors', normals'] or None).  Reads V', F' back once, then the state once more after the emit."""
        self.call("ibgs_mesh_filter_count", labels.data_ptr(), keep_cluster.data_ptr(), C, flags)
        s = self.counters()
        V2, F2 = s[_lib.MESH_VERTICES_OUT], s[_lib.MESH_FACES_OUT]
        keep_v = bool(flags & _lib.MESH_KEEP_VERTICES)
        with torch.cuda.device(self.dev):
            faces = torch.empty(F2, 3, dtype=torch.int32, device=self.dev)
            src = [] if keep_v else [self.vertices, mesh.colors.contiguous(), mesh.normals.contiguous()]
            dst = [torch.empty(V2, 3, dtype=torch.float32, device=self.dev) for _ in src]
        ptrs = lambda ts: (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
        self.call("ibgs_mesh_filter_emit", flags, V2, F2, faces.data_ptr(), len(src), ptrs(src), ptrs(dst))
        self.counters()          # (an emit outside the outputs would be a library fault: raise rather than hand out a partial mesh)
        return faces, (None if keep_v else dst)


def _empty(dev):
    z = lambda dt: torch.empty(0, 3, dtype=dt, device=dev)
    return TriangleMesh(z(torch.float32), z(torch.int32), z(torch.float32), z(torch.float32))


def cluster_connected_triangles(mesh):
    """Connected components of the triangles of a device mesh under "share an edge" (Open3D's `TriangleMesh.cluster_connected_triangles`).

    An edge is an unordered pair of vertex indices, taken literally; sharing only a vertex does not connect.  Clusters are numbered in ascending order of their
    smallest triangle index.  -> TriangleClusters(triangle_clusters (F,) int32, cluster_n_triangles (C,) int32, cluster_area (C,) f64), on the device.
    One host read-back: the counters that carry C (and the count of out-of-range face indices, which raises MeshError)."""
    V, F, dev = _check(mesh)
    if F == 0:
        return TriangleClusters(torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                                torch.empty(0, dtype=torch.float64, device=dev))
    labels, counts, areas, _ = _Run(mesh, V, F, dev).cluster()
    return TriangleClusters(labels, counts.clone(), areas.clone())          # (clones: the views would keep two F-long buffers alive)


def post_process_mesh(mesh, cluster_to_keep=1, min_triangles=50):
    """render.py's `post_process_mesh(mesh, cluster_to_keep)`: keep the triangles of every cluster with at least
    n = max(cluster_to_keep-th largest cluster size, min_triangles) triangles (ties keep more than cluster_to_keep clusters), drop the vertices no survivor
    refers to and re-index the faces, then drop the survivors that repeat a vertex index.  Order is kept; positions, colours and normals are copied bit for
    bit (normals are not recomputed).  -> a new tsdf.TriangleMesh on the device; the input is left untouched.

    ValueError for cluster_to_keep < 1 and for cluster_to_keep > number of clusters (the reference's IndexError); an empty mesh returns an empty mesh.
    Host read-backs: the counters after clustering (C), after the filter's count pass (V', F': they size the outputs) and after the emit."""
    cluster_to_keep, min_triangles = int(cluster_to_keep), int(min_triangles)
    if cluster_to_keep < 1:
        raise ValueError("cluster_to_keep must be >= 1, got %d" % cluster_to_keep)
    V, F, dev = _check(mesh)
    if F == 0:
        return _empty(dev)
    run = _Run(mesh, V, F, dev)
    labels, counts, _, C = run.cluster()
    if cluster_to_keep > C:
        raise ValueError("cluster_to_keep = %d, but the mesh has %d cluster(s)" % (cluster_to_keep, C))
    with torch.cuda.device(dev):
        kth = torch.topk(counts, cluster_to_keep).values[-1]          # (stays on the device)
        keep = (counts >= torch.clamp(kth, min=min_triangles)).to(torch.uint8)
    faces, (vert, col, nrm) = run.filter(mesh, labels, keep, C, 0)
    return TriangleMesh(vert, faces, col, nrm)


def clean_mesh(mesh, min_len=1000):
    """render.py's `clean_mesh(mesh, min_len)`: the triangles of clusters with fewer than min_len triangles removed; vertices, colours and normals are
    left as they are (the returned mesh shares those tensors with the input), degenerate triangles stay.  Host read-backs: as post_process_mesh."""
    V, F, dev = _check(mesh)
    min_len = int(min_len)
    if F == 0:
        return TriangleMesh(mesh.vertices, mesh.faces, mesh.colors, mesh.normals)
    run = _Run(mesh, V, F, dev)
    labels, counts, _, C = run.cluster()
    with torch.cuda.device(dev):
        keep = (counts >= min_len).to(torch.uint8)
    faces, _ = run.filter(mesh, labels, keep, C, _lib.MESH_KEEP_VERTICES | _lib.MESH_KEEP_DEGENERATE)
    return TriangleMesh(mesh.vertices, faces, mesh.colors, mesh.normals)
