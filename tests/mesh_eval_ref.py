"""Host restatement of the mesh-evaluation contract ("Mesh evaluation"; header of ibgs_amd/csrc/mesh_eval.hip) in numpy + scipy.
It shares no code with the kernels or with ibgs_amd/mesh_eval.py.  Each stage is stated twice: once with a kd-tree to find candidates (any size), once
literally (brute force, small inputs); the decisions are always taken with the contract's own f32 formula."""
import numpy as np
from scipy.spatial import cKDTree

F32 = np.float32


# ---- surface sampling ------------------------------------------------------------------------------------------------------------------------------
def triangle_grid(vertices, faces, density):
    """Per triangle (n1, n2) as int64 (0, 0 for a triangle that yields nothing) and the f64 (p0, v1, v2); |v|/thr too (for the band check)."""
    v = np.asarray(vertices, F32).astype(np.float64)
    p0, p1, p2 = (v[np.asarray(faces)[:, k]] for k in range(3))
    v1, v2 = p1 - p0, p2 - p0
    norm = lambda a: np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    l1, l2 = norm(v1), norm(v2)
    c = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2], v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], 1)
    area2 = norm(c)
    ok = area2 > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        thr = float(density) * np.sqrt(l1 * l2 / area2)
        r1, r2 = l1 / thr, l2 / thr
    r1, r2 = np.where(ok, r1, 0.0), np.where(ok, r2, 0.0)
    n1, n2 = np.floor(r1).astype(np.int64), np.floor(r2).astype(np.int64)
    none = (n1 == 0) | (n2 == 0)
    n1[none] = 0
    n2[none] = 0
    return n1, n2, p0, v1, v2, r1, r2


def sample_triangle(n1, n2, p0, v1, v2):
    """The f64 samples of one triangle, i-major, and the smallest |a + b - 1| met (for the band check)."""
    if n1 == 0 or n2 == 0:
        return np.zeros((0, 3)), np.inf
    a = (np.arange(n1 + 1, dtype=np.float64) + 0.5) / float(n1)
    b = (np.arange(n2 + 1, dtype=np.float64) + 0.5) / float(n2)
    s = a[:, None] + b[None, :]
    ii, jj = np.nonzero(s < 1.0)          # (row-major = i-major)
    q = (v1[None, :] * a[ii, None] + v2[None, :] * b[jj, None]) + p0[None, :]
    return q, float(np.abs(s - 1.0).min())


def sample_surface(vertices, faces, density, include_vertices=True):
    """-> (points (N, 3) f64 before the one rounding to f32, counts per triangle (F,) int64, margins dict)."""
    n1, n2, p0, v1, v2, r1, r2 = triangle_grid(vertices, faces, density)
    parts, counts, band = [], np.zeros(len(n1), np.int64), np.inf
    for t in range(len(n1)):
        q, m = sample_triangle(int(n1[t]), int(n2[t]), p0[t], v1[t], v2[t])
        parts.append(q)
        counts[t] = len(q)
        band = min(band, m)
    pts = np.concatenate(([np.asarray(vertices, F32).astype(np.float64)] if include_vertices else []) + parts) if parts or include_vertices else np.zeros((0, 3))
    r = np.concatenate([r1, r2])
    r = r[np.isfinite(r) & (r > 0)]
    floor_margin = float(np.abs(r - np.round(r)).min()) if len(r) else np.inf
    return pts, counts, {"floor_margin": floor_margin, "sum_margin": band}


# ---- the f32 distance ------------------------------------------------------------------------------------------------------------------------------
def d2_f32(q, t):
    """(dx dx + dy dy) + dz dz in f32, broadcasting; q, t: (..., 3) f32."""
    d = np.asarray(q, F32) - np.asarray(t, F32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _flat_pairs(lists):
    n = np.fromiter((len(l) for l in lists), np.int64, len(lists))
    return np.repeat(np.arange(len(lists)), n), (np.concatenate([np.asarray(l, np.int64) for l in lists]) if n.sum() else np.zeros(0, np.int64))


# ---- thinning --------------------------------------------------------------------------------------------------------------------------------------
def _thin(n, rank, src, dst):
    """The loop of eval.py:86-94 over the directed pairs (src, dst) of the radius graph."""
    order = np.argsort(rank, kind="stable")
    start = np.searchsorted(src, np.arange(n + 1))          # (src is ascending)
    mask = np.ones(n, bool)
    for i in order:
        if mask[i]:
            mask[dst[start[i]:start[i + 1]]] = False
            mask[i] = True
    return mask


def rank_of(n, order):
    rank = np.arange(n)
    if order is not None:
        rank = np.empty(n, np.int64)
        rank[np.asarray(order)] = np.arange(n)
    return rank


def downsample(points, radius, order=None):
    """Keep mask; neighbours from a kd-tree at radius (1 + 1e-4), each pair then decided by d2 <= r r in f32."""
    p = np.ascontiguousarray(points, F32)
    n = len(p)
    if n == 0:
        return np.zeros(0, bool)
    r = F32(radius)
    lists = cKDTree(p.astype(np.float64)).query_ball_point(p.astype(np.float64), float(radius) * (1 + 1e-4) + 1e-30)
    src, dst = _flat_pairs(lists)
    near = d2_f32(p[src], p[dst]) <= r * r
    return _thin(n, rank_of(n, order), src[near], dst[near])


def downsample_brute(points, radius, order=None):
    """The rule read literally: visit the points by rank; keep one iff no kept point before it has d2 <= r r."""
    p = np.ascontiguousarray(points, F32)
    r2 = F32(radius) * F32(radius)
    keep = np.zeros(len(p), bool)
    kept = []
    for i in np.argsort(rank_of(len(p), order), kind="stable"):
        if not kept or not np.any(d2_f32(p[i], p[kept]) <= r2):
            keep[i] = True
            kept.append(i)
    return keep


# ---- nearest ---------------------------------------------------------------------------------------------------------------------------------------
def _finish(best, idx, max_dist):
    md = F32(max_dist)
    found = (idx >= 0) & (best < md * md)
    dist = np.where(found, np.sqrt(best.astype(np.float64)).astype(F32), F32(np.inf)).astype(F32)          # f64 root rounded = the correctly rounded f32 root
    return dist, np.where(found, idx, -1).astype(np.int32)


def nearest(query, target, max_dist):
    """(dist f32, index int32).  The kd-tree gives the f64 nearest distance d64; every target within d64 (1 + 1e-4) is re-scored with the f32 formula (the f32
    d2 is within 4 x 2^-24 relative of the exact one, so the f32 minimum and all its ties are among them); the smallest index among the minima wins."""
    q, t = np.ascontiguousarray(query, F32), np.ascontiguousarray(target, F32)
    best, idx = np.full(len(q), np.inf, F32), np.full(len(q), -1, np.int64)
    if len(q) and len(t):
        tree = cKDTree(t.astype(np.float64))
        d64, _ = tree.query(q.astype(np.float64), k=1, distance_upper_bound=float(max_dist) * (1 + 1e-3) + 1e-30)
        has = np.flatnonzero(np.isfinite(d64))
        if len(has):
            qi, ti = _flat_pairs(tree.query_ball_point(q[has].astype(np.float64), d64[has] * (1 + 1e-4) + 1e-30))
            qi = has[qi]
            d2 = d2_f32(q[qi], t[ti])
            o = np.lexsort((ti, d2, qi))          # per query: ascending d2, then ascending index
            first = o[np.concatenate([[True], qi[o][1:] != qi[o][:-1]])]
            best[qi[first]], idx[qi[first]] = d2[first], ti[first]
    return _finish(best, idx, max_dist)


def nearest_brute(query, target, max_dist):
    q, t = np.ascontiguousarray(query, F32), np.ascontiguousarray(target, F32)
    best, idx = np.full(len(q), np.inf, F32), np.full(len(q), -1, np.int64)
    if len(t):
        for i in range(len(q)):
            d2 = d2_f32(q[i], t)
            idx[i] = int(np.argmin(d2))          # (the first of equal minima)
            best[i] = d2[idx[i]]
    return _finish(best, idx, max_dist)


# ---- the metrics -----------------------------------------------------------------------------------------------------------------------------------
def mean_below(dist, threshold):
    """(f64 mean or NaN, count) of the dist < threshold (f32 compare)."""
    sel = np.asarray(dist, F32) < F32(threshold)
    n = int(sel.sum())
    return (float(np.asarray(dist, F32)[sel].astype(np.float64).sum() / n) if n else float("nan")), n


def chamfer(pred, gt, max_dist, pred_query_mask=None, gt_query_mask=None, nn=nearest):
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    pq = pred if pred_query_mask is None else pred[np.asarray(pred_query_mask)]
    gq = gt if gt_query_mask is None else gt[np.asarray(gt_query_mask)]
    a, na = mean_below(nn(pq, gt, max_dist)[0], max_dist)
    b, nb = mean_below(nn(gq, pred, max_dist)[0], max_dist)
    return {"mean_d2s": a, "mean_s2d": b, "overall": (a + b) / 2, "n_d2s": na, "n_s2d": nb}


def fscore(pred, gt, tau, nn=nearest):
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    if len(pred) == 0 or len(gt) == 0:
        return {"precision": 0.0, "recall": 0.0, "fscore": 0.0, "n_precision": 0, "n_recall": 0}
    a = int((nn(pred, gt, 2 * tau)[0] < F32(tau)).sum())
    b = int((nn(gt, pred, 2 * tau)[0] < F32(tau)).sum())
    p, r = a / len(pred), b / len(gt)
    return {"precision": p, "recall": r, "fscore": (2 * r * p / (r + p)) if r + p > 0 else 0.0, "n_precision": a, "n_recall": b}


# ---- test inputs -----------------------------------------------------------------------------------------------------------------------------------
def random_mesh(n_tri, seed, scale=1.0, extent=4.0):
    """n_tri independent triangles (3 n_tri vertices) of mixed sizes."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, (n_tri, 1, 3))
    size = scale * np.exp(rng.uniform(np.log(0.02), np.log(1.0), (n_tri, 1, 1)))
    v = (c + size * rng.normal(size=(n_tri, 3, 3))).reshape(-1, 3).astype(F32)
    return v, np.arange(3 * n_tri, dtype=np.int32).reshape(-1, 3)


def surface_cloud(n, seed, noise=0.01):
    """n points near a wavy sheet: the kind of cloud a sampled mesh is."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n, 2))
    z = 0.3 * np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1]) + noise * rng.normal(size=n)
    return np.concatenate([xy, z[:, None]], 1).astype(F32)


def pair_margin(points, radius):
    """Smallest | d - radius | / radius over the pairs near the radius, d in f64 (the band condition of the thinning)."""
    p = np.asarray(points, F32).astype(np.float64)
    tree = cKDTree(p)
    pairs = tree.query_pairs(float(radius) * 1.01, output_type="ndarray")
    if not len(pairs):
        return np.inf
    d = np.linalg.norm(p[pairs[:, 0]] - p[pairs[:, 1]], axis=1)
    return float(np.abs(d - float(radius)).min() / float(radius))
