"""Host restatement of the registration contract ("Registration"; header of ibgs_amd/csrc/registration.hip) in numpy.  It shares no
code with the kernels or with ibgs_amd/registration.py; the nearest search is tests/mesh_eval_ref.py's."""
import json

import numpy as np

from tests import mesh_eval_ref

F32 = np.float32
AXES = {"X": (0, 1, 2), "Y": (1, 0, 2), "Z": (2, 0, 1)}          # orthogonal_axis -> (w; u, v)
MAX_INDEX = (1 << 21) - 1


# ---- transform -------------------------------------------------------------------------------------------------------------------------------------
def transform(points, T):
    """x' = ((T00 x + T01 y) + T02 z) + T03 in f64 from the f32 coordinates, rounded once."""
    p = np.asarray(points, F32).astype(np.float64)
    T = np.asarray(T, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(F32)


# ---- crop ------------------------------------------------------------------------------------------------------------------------------------------
def write_crop_volume(path, axis, axis_min, axis_max, polygon):
    """A TnT-style crop file, as Open3D writes a SelectionPolygonVolume."""
    with open(path, "w") as f:
        json.dump({"axis_max": float(axis_max), "axis_min": float(axis_min), "bounding_polygon": [[float(c) for c in v] for v in polygon],
                   "class_name": "SelectionPolygonVolume", "orthogonal_axis": axis, "version_major": 1, "version_minor": 0}, f)


def crop(points, axis, axis_min, axis_max, polygon, T=None):
    """Keep mask.  polygon: (n, 3) f64.  The crossing rule edge by edge, vectorised over the points, every operation in f64 in the contract's order."""
    p = np.asarray(points, F32) if T is None else transform(points, T)
    p = p.astype(np.float64)
    w, u, v = AXES[axis]
    poly = np.asarray(polygon, np.float64)
    n = len(poly)
    left = np.zeros(len(p), np.int64)
    pu, pv = p[:, u], p[:, v]
    for i in range(n):
        j = (i + 1) % n
        ui, vi, uj, vj = poly[i, u], poly[i, v], poly[j, u], poly[j, v]
        crosses = ((vi < pv) & (vj >= pv)) | ((vj < pv) & (vi >= pv))
        if vj != vi:
            node = ui + (pv - vi) / (vj - vi) * (uj - ui)
            left += crosses & (node < pu)
    return (float(axis_min) <= p[:, w]) & (p[:, w] <= float(axis_max)) & (left % 2 == 1)


# ---- voxel thinning --------------------------------------------------------------------------------------------------------------------------------
def voxel_index(points, voxel):
    p = np.asarray(points, F32)
    origin = p.min(0).astype(np.float64) - float(voxel) / 2
    return np.floor((p.astype(np.float64) - origin) / float(voxel)).astype(np.int64)


def voxel_down_sample(points, voxel):
    """-> (means (M, 3) f64 before the one rounding to f32, keys (M,) int64 ascending, counts (M,), points beyond the 21-bit grid).  Sums in point-index order."""
    p = np.asarray(points, F32)
    if len(p) == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    idx = voxel_index(p, voxel)
    over = int((idx > MAX_INDEX).any(1).sum())
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    keys, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    sums = np.zeros((len(keys), 3))
    np.add.at(sums, inv.reshape(-1), p.astype(np.float64))          # (unbuffered: one addition after the other, in index order)
    return sums / counts[:, None].astype(np.float64), keys, counts, over


# ---- moments and the similarity fit ----------------------------------------------------------------------------------------------------------------
def moment_terms(query, target, index, pivot):
    """(n, 17) f64: per correspondence the terms of sum(s - c) [3], sum(t - c) [3], sum (s - c)(t - c)^T [9, row = s], sum |s - c|^2, sum d^2."""
    index = np.asarray(index)
    has = index >= 0
    s = np.asarray(query, F32)[has].astype(np.float64)
    t = np.asarray(target, F32)[index[has]].astype(np.float64)
    c = np.asarray(pivot, np.float64)
    sc, tc, d = s - c, t - c, s - t
    outer = (sc[:, :, None] * tc[:, None, :]).reshape(len(s), 9)
    ss = (sc[:, 0] * sc[:, 0] + sc[:, 1] * sc[:, 1]) + sc[:, 2] * sc[:, 2]
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.concatenate([sc, tc, outer, ss[:, None], dd[:, None]], 1)


def moments(query, target, index, pivot, reverse=False):
    """The 18 numbers, summed one term after the other in index order (reverse: from the last correspondence to the first)."""
    terms = moment_terms(query, target, index, pivot)
    if reverse:
        terms = terms[::-1]
    total = np.cumsum(terms, axis=0)[-1] if len(terms) else np.zeros(17)          # (cumsum adds sequentially)
    return np.concatenate([[float(len(terms))], total])


def umeyama(m, pivot):
    """Eigen's umeyama with scaling from the raw moments about the pivot."""
    n = m[0]
    if n < 3:
        raise ValueError("fewer than 3 correspondences")
    mean_s, mean_t = m[1:4] / n, m[4:7] / n
    cov_ts = np.array([[m[7 + 3 * a + b] / n - mean_t[b] * mean_s[a] for a in range(3)] for b in range(3)])          # row t, column s
    var_s = m[16] / n - (mean_s[0] ** 2 + mean_s[1] ** 2 + mean_s[2] ** 2)
    if not var_s > 0:
        raise ValueError("no extent")
    U, D, Vt = np.linalg.svd(cov_ts)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    scale = np.trace(np.diag(D) @ S) / var_s
    T = np.identity(4)
    T[:3, :3] = scale * R
    T[:3, 3] = (np.asarray(pivot) + mean_t) - scale * R @ (np.asarray(pivot) + mean_s)
    return T


def umeyama_points(src, dst):
    s, t = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, mt = s.mean(0), t.mean(0)
    cov = (t - mt).T @ (s - ms) / len(s)
    var_s = ((s - ms) ** 2).sum() / len(s)
    U, D, Vt = np.linalg.svd(cov)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    scale = np.trace(np.diag(D) @ S) / var_s
    T = np.identity(4)
    T[:3, :3] = scale * R
    T[:3, 3] = mt - scale * R @ ms
    return T


def pivot_of(target):
    t = np.asarray(target, F32)
    return (t.min(0).astype(np.float64) + t.max(0).astype(np.float64)) / 2


def icp(source, target, max_dist, init=None, max_iter=20, rel_fitness=1e-6, rel_rmse=1e-6, reverse=False):
    """-> dict(transformation, fitness, inlier_rmse, iterations, n_correspondences)."""
    source, target = np.asarray(source, F32), np.asarray(target, F32)
    T = np.identity(4) if init is None else np.array(init, np.float64)
    c = pivot_of(target)
    prev, k = None, 0
    while True:
        q = transform(source, T)
        _, idx = mesh_eval_ref.nearest(q, target, max_dist)
        m = moments(q, target, idx, c, reverse=reverse)
        n = int(m[0])
        if n < 3:
            raise ValueError("iteration %d: %d correspondences" % (k, n))
        fitness, rmse = n / len(source), float(np.sqrt(m[17] / n))
        if (prev is not None and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse) or k == max_iter:
            return {"transformation": T, "fitness": fitness, "inlier_rmse": rmse, "iterations": k, "n_correspondences": n}
        prev = (fitness, rmse)
        T = umeyama(m, c) @ T
        k += 1


# ---- the TnT chain ---------------------------------------------------------------------------------------------------------------------------------
def _vds(points, voxel):
    return voxel_down_sample(points, voxel)[0].astype(F32)


def _uniform(cloud, max_points):
    n = len(cloud)
    return cloud[::int(round(n / float(max_points)))] if n > max_points else cloud


def evaluate_tnt(pred, gt, init_trans, volume, tau, voxel_rounds=((1, 80), (0.5, 20)), uniform_round=2, max_iter=20, max_points=4_000_000):
    """volume: (axis, axis_min, axis_max, polygon).  -> dict with the thinned clouds and their nearest distances too (for the borderline count)."""
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    T = np.array(init_trans, np.float64)
    moved = lambda T: transform(pred[crop(pred, *volume, T=T)], T)
    gt_crop = gt[crop(gt, *volume)]
    rounds = []
    for a, b in voxel_rounds:
        r = icp(_vds(moved(T), a * tau), _vds(gt_crop, a * tau), b * tau, max_iter=max_iter)
        T = r["transformation"] @ T
        rounds.append(r)
    if uniform_round is not None:
        r = icp(_uniform(moved(T), max_points), _uniform(gt_crop, max_points), uniform_round * tau, max_iter=max_iter)
        T = r["transformation"] @ T
        rounds.append(r)
    s, t = _vds(moved(T), tau / 2), _vds(gt_crop, tau / 2)
    d_st, d_ts = mesh_eval_ref.nearest(s, t, 2 * tau)[0], mesh_eval_ref.nearest(t, s, 2 * tau)[0]
    a, b = int((d_st < F32(tau)).sum()), int((d_ts < F32(tau)).sum())
    p, r = (a / len(s), b / len(t)) if len(s) and len(t) else (0.0, 0.0)
    return {"precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0, "n_precision": a, "n_recall": b, "n_pred": len(s), "n_gt": len(t),
            "transformation": T, "rounds": rounds, "dist_pred": d_st, "dist_gt": d_ts}


# ---- test inputs -----------------------------------------------------------------------------------------------------------------------------------
def similarity(scale, angle_deg, axis, t):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(angle_deg)
    T = np.identity(4)
    T[:3, :3] = scale * (np.identity(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K)
    T[:3, 3] = t
    return T


PLANTED = similarity(1.02, 2.0, (0.3, -0.5, 0.8), (0.03, -0.02, 0.025))


def icp_scene(n_sheet, n_wall, seed):
    """Source: n_sheet points on z = 0.3 sin 3x cos 2y + 0.2 x y over [-1, 1]^2 and n_wall points on the wall x = 1 (f32).  Target: the source under PLANTED,
    rounded to f32, and a third as many again jittered duplicates (sigma 0.002).  -> (source, target)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n_sheet, 2))
    sheet = np.concatenate([xy, (0.3 * np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1]) + 0.2 * xy[:, 0] * xy[:, 1])[:, None]], 1)
    wall = np.concatenate([np.ones((n_wall, 1)), rng.uniform(-1, 1, (n_wall, 1)), rng.uniform(-0.5, 0.5, (n_wall, 1))], 1)
    src = np.concatenate([sheet, wall]).astype(F32)
    exact = (src.astype(np.float64) @ PLANTED[:3, :3].T + PLANTED[:3, 3]).astype(F32)
    dup = rng.choice(len(src), len(src) // 3, replace=False)
    jit = (exact[dup].astype(np.float64) + 0.002 * rng.normal(size=(len(dup), 3))).astype(F32)
    return src, np.concatenate([exact, jit])
