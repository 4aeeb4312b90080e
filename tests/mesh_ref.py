"""Host restatements of the mesh post-processing contract ("Mesh post-processing"; ibgs_amd/csrc/mesh.hip) and the meshes the
tests run it on.  Two independent algorithms, neither shares code with the kernels:

  cluster()       numpy + scipy: edges -> triangle adjacency (every triangle of an edge linked to the edge's first) -> scipy.sparse.csgraph
                  .connected_components -> renumbered by smallest triangle index -> counts, f64 areas
  cluster_bfs()   literal, for small meshes: dict of edges, adjacency sets, breadth-first search seeded from the lowest unvisited triangle

and the filters (post_process, clean) in plain numpy indexing.  This is numpy + scipy, not Open3D."""
from collections import deque

import numpy as np


# ---- restatement 1: numpy + scipy -----------------------------------------------------------------------------------------------------------------

def triangle_areas(vertices, faces):
    p = np.asarray(vertices, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return 0.5 * np.sqrt((n * n).sum(1))


def cluster(vertices, faces):
    """-> (triangle_clusters (F,) int32, cluster_n_triangles (C,) int32, cluster_area (C,) f64)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    if F == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    V = int(max(len(vertices), f.max() + 1))
    pairs = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = pairs.min(1) * V + pairs.max(1)
    tri = np.tile(np.arange(F), 3)
    order = np.argsort(key, kind="stable")
    key, tri = key[order], tri[order]
    start = np.r_[True, key[1:] != key[:-1]]
    first = tri[np.flatnonzero(start)[np.cumsum(start) - 1]]          # the first triangle of every entry's edge
    g = coo_matrix((np.ones(len(tri), np.int8), (tri, first)), shape=(F, F))
    _, lab = connected_components(g, directed=False)
    _, first_tri = np.unique(lab, return_index=True)                  # smallest triangle of every component
    rank = np.empty(len(first_tri), np.int64)
    rank[np.argsort(first_tri)] = np.arange(len(first_tri))
    lab = rank[lab]
    counts = np.bincount(lab)
    areas = np.bincount(lab, weights=triangle_areas(vertices, f))
    return lab.astype(np.int32), counts.astype(np.int32), areas.astype(np.float64)


# ---- restatement 2: the literal one ---------------------------------------------------------------------------------------------------------------

def cluster_bfs(vertices, faces):
    f = [tuple(int(x) for x in t) for t in np.asarray(faces).reshape(-1, 3)]
    by_edge = {}
    for t, (a, b, c) in enumerate(f):
        for p, q in ((a, b), (b, c), (c, a)):
            by_edge.setdefault((min(p, q), max(p, q)), []).append(t)
    adj = [set() for _ in f]
    for ts in by_edge.values():
        for t in ts:
            adj[t].update(ts)
    lab = [-1] * len(f)
    counts = []
    for seed in range(len(f)):
        if lab[seed] >= 0:
            continue
        c = len(counts)
        lab[seed] = c
        n, q = 0, deque([seed])
        while q:
            t = q.popleft()
            n += 1
            for u in adj[t]:
                if lab[u] < 0:
                    lab[u] = c
                    q.append(u)
        counts.append(n)
    lab = np.array(lab, np.int32).reshape(-1)
    ar = triangle_areas(vertices, np.asarray(faces).reshape(-1, 3)) if len(f) else np.zeros(0)
    areas = np.array([ar[lab == c].sum() for c in range(len(counts))], np.float64)
    return lab, np.array(counts, np.int32), areas


# ---- the filters ------------------------------------------------------------------------------------------------------------------------------------

def post_process(faces, n_vertices, labels, counts, cluster_to_keep=1, min_triangles=50):
    """-> (vertex_rows, faces_out): the input rows of the surviving vertices, in order, and the re-indexed surviving faces."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if cluster_to_keep < 1 or (len(f) and cluster_to_keep > len(counts)):
        raise ValueError("cluster_to_keep")
    if len(f) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int32)
    n = max(int(np.sort(counts)[-cluster_to_keep]), min_triangles)
    f = f[counts[labels] >= n]                                     # remove_triangles_by_mask
    used = np.zeros(n_vertices, bool)
    used[f.reshape(-1)] = True                                     # remove_unreferenced_vertices
    new_index = np.cumsum(used) - 1
    f = new_index[f]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]          # remove_degenerate_triangles
    return np.flatnonzero(used), f.astype(np.int32)


def clean(faces, labels, counts, min_len=1000):
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    return f[counts[labels] >= min_len] if len(f) else f


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------------------

def grid(n, m, h=1.0, origin=(0.0, 0.0, 0.0)):
    """n x m vertices spaced h, 2 (n - 1)(m - 1) triangles, area (n - 1)(m - 1) h^2."""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    v = np.stack([i.ravel() * h, j.ravel() * h, np.zeros(n * m)], 1) + np.asarray(origin, np.float64)
    a = (i[:-1, :-1] * m + j[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([a, a + m, a + 1], 1), np.stack([a + 1, a + m, a + m + 1], 1)], 1).reshape(-1, 3)
    return v.astype(np.float32), f.astype(np.int32)


def join(parts):
    """Disjoint union of (vertices, faces) meshes."""
    vs, fs, off = [], [], 0
    for v, f in parts:
        vs.append(v); fs.append(f + off); off += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def permute(v, f, seed):
    """The same mesh with vertex ids, triangle order and each triangle's starting corner randomly permuted."""
    rng = np.random.default_rng(seed)
    pv, pf = rng.permutation(len(v)), rng.permutation(len(f))
    inv = np.empty(len(v), np.int64); inv[pv] = np.arange(len(v))          # old id -> new id
    f = inv[f][pf]
    r = rng.integers(0, 3, len(f))
    f = np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], 1)
    return v[pv], f.astype(np.int32)


CASE1_GRIDS = [(60, 80), (40, 40), (40, 40), (6, 6), (6, 5), (5, 5), (3, 3), (2, 2), (2, 2), (30, 10)]
CASE1_H = 0.25
# checked with both restatements: 11 clusters; cluster_to_keep -> surviving faces of 16065
CASE1_COUNTS = [9323, 3042, 3042, 522, 50, 40, 32, 8, 2, 2, 2]
CASE1_KEPT = {1: 9323, 2: 15407, 3: 15407, 4: 15929, 5: 15979}


def case1(seed=11, permuted=True):
    """Disjoint grids, a third triangle on one edge of the first grid, two degenerate triangles (p, p, q) and (p, p, r) that share only {p, p}, one
    unreferenced vertex."""
    parts = [grid(n, m, CASE1_H, origin=(100.0 * k, 0.0, 0.0)) for k, (n, m) in enumerate(CASE1_GRIDS)]
    v, f = join(parts)
    V = len(v)
    extra_v = np.array([[0.1, 0.1, 1.0], [500.0, 500.0, 0.0], [501.0, 500.0, 0.0], [500.0, 501.0, 0.0], [900.0, 900.0, 900.0]], np.float32)
    apex, p, q, r = V, V + 1, V + 2, V + 3          # (V + 4: the unreferenced vertex)
    extra_f = np.array([[f[0, 1], f[0, 2], apex],          # (the first quad's diagonal: its third triangle)
                         [p, p, q], [p, p, r]], np.int32)
    v, f = np.concatenate([v, extra_v]), np.concatenate([f, extra_f])
    return permute(v, f, seed) if permuted else (v, f)


def attributes(v, seed=5):
    """Colours and normals with every bit pattern class a copy must preserve (random payloads; a NaN and a -0 among them)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, v.shape).astype(np.float32)
    n = rng.normal(size=v.shape).astype(np.float32)
    if len(v) > 2:
        n[0, 0] = -0.0; n[1, 1] = np.nan
    return c, n


def strip(n_tri):
    """A triangle strip: triangle t = (t, t + 1, t + 2) (orientation alternating), each adjacent to the next."""
    t = np.arange(n_tri)
    f = np.stack([t, t + 1, t + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    k = np.arange(n_tri + 2)
    v = np.stack([0.5 * k, (k & 1).astype(np.float64), np.zeros(len(k))], 1).astype(np.float32)
    return v, f.astype(np.int32)


def cut_strip(n_tri, pieces, seed):
    """`pieces` separate strips of unequal lengths summing to n_tri (no shared vertices) -> (vertices, faces, lengths)."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n_tri), pieces - 1, replace=False))
    lengths = np.diff(np.r_[0, cuts, n_tri])
    parts = []
    for k, L in enumerate(lengths):
        v, f = strip(int(L))
        parts.append((v + np.array([0.0, 3.0 * k, 0.0], np.float32), f))
    v, f = join(parts)
    return v, f, lengths


def fan(n_tri, n_loose):
    """n_tri triangles (0, i, i + 1) around vertex 0 (one cluster), then n_loose triangles (0, a, b) with private a, b: they touch the fan, and each other,
    at vertex 0 only (n_loose clusters of one)."""
    i = np.arange(1, n_tri + 1)
    f_fan = np.stack([np.zeros(n_tri, np.int64), i, i + 1], 1)
    base = n_tri + 2
    j = np.arange(n_loose)
    f_loose = np.stack([np.zeros(n_loose, np.int64), base + 2 * j, base + 2 * j + 1], 1)
    nv = base + 2 * n_loose
    ang = np.linspace(0.0, 40.0 * np.pi, nv)
    rad = 1.0 + np.arange(nv) * 1e-5
    v = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.arange(nv) * 1e-6], 1)
    v[0] = 0.0
    return v.astype(np.float32), np.concatenate([f_fan, f_loose]).astype(np.int32)


# ---- the analytic sphere with four fused floaters (tests/test_gpu_tsdf.py's scene + four small spheres) -----------------------------------------------

FLOATERS = [((0.80, 0.0, 0.0), 0.10), ((0.0, -0.78, 0.15), 0.08), ((-0.3, 0.3, 0.75), 0.06), ((0.0, 0.0, -0.74), 0.04)]


def floater_frames(W=160, H=120, fx=140.0, cx=80.0, cy=60.0, radius=0.5, dist=2.0, n_views=24):
    """[(depth, colour, world_to_camera, (fx, fy, cx, cy))]: the big sphere and the floaters composited per pixel by nearest depth."""
    from tests import tsdf_ref as ref
    frames = []
    for d in ref.fibonacci_directions(n_views):
        M = ref.look_at(dist * d)
        dep, col = ref.sphere_view(M, W, H, fx, fx, cx, cy, radius)
        for center, r in FLOATERS:
            d2, c2 = ref.sphere_view(M, W, H, fx, fx, cx, cy, r, center=center)
            nearer = (d2 > 0) & ((dep == 0) | (d2 < dep))
            dep = np.where(nearer, d2, dep)
            col = np.where(nearer[None], c2, col)
        frames.append((dep.astype(np.float32), col.astype(np.float32), M, (fx, fx, cx, cy)))
    return frames
