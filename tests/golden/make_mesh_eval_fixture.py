"""Generator of tests/golden/mesh_eval.npz (BUILD CONTAINER ONLY; the suites read the .npz and never the reference).

Runs the reference's own evaluation code on small inputs and stores inputs and results only:
  * `sample_single_tri` is imported from /root/reference/scripts/eval_dtu/eval.py (with `open3d` registered as an empty module: the function does not use
    it) and driven per triangle the way eval.py:54-71 drives it;
  * the thinning is sklearn's NearestNeighbors(algorithm='kd_tree').radius_neighbors and the loop of eval.py:86-94;
  * the distances are the same engine's kneighbors (eval.py:119-120).

The contract decides in f32 where the reference decides in f64, so the inputs are chosen (by seed) such that the reference alone is unambiguous -- no pair
within 1e-5 radius of the radius, no |v| / thr within 1e-9 of an integer, no a + b within 1e-9 of 1 -- and the margins are stored for the test to re-assert.

    python tests/golden/make_mesh_eval_fixture.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import sklearn.neighbors as skln

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import mesh_eval_ref as ref  # noqa: E402  (input generators and the margin helpers only)

REF_EVAL = "/root/reference/scripts/eval_dtu/eval.py"
PAIR_BAND, FLOOR_BAND, SUM_BAND = 1e-5, 1e-9, 1e-9


def reference_sample_single_tri():
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    spec = importlib.util.spec_from_file_location("ref_eval_dtu", REF_EVAL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # (everything else in the file sits under `if __name__ == '__main__'`)
    return mod.sample_single_tri


def reference_sampling(vertices, faces, density, sample_single_tri):
    """The reference's function, triangle by triangle, on the arguments eval.py builds for it: (n1, n2, v1 (1, 3), v2 (1, 3), p0 (3,)) in f64."""
    n1, n2, p0, v1, v2, _, _ = ref.triangle_grid(vertices, faces, density)
    parts = [sample_single_tri((float(n1[t]), float(n2[t]), v1[t:t + 1], v2[t:t + 1], p0[t])) for t in range(len(faces))]
    counts = np.array([len(q) for q in parts], np.int64)
    return np.concatenate([vertices.astype(np.float64)] + parts, axis=0), counts


def _engine(points, radius):
    return skln.NearestNeighbors(n_neighbors=1, radius=radius, algorithm="kd_tree", n_jobs=-1).fit(points)


def reference_thinning(points, radius):
    """sklearn's radius lists, walked in index order: a point still standing when visited knocks out its neighbours."""
    lists = _engine(points, radius).radius_neighbors(points, radius=radius, return_distance=False)
    keep = np.ones(len(points), bool)
    for i, near in enumerate(lists):
        if keep[i]:
            keep[near] = False
            keep[i] = True
    return keep


def reference_distances(query, target, radius):
    dist, idx = _engine(target, radius).kneighbors(query, n_neighbors=1, return_distance=True)
    return dist[:, 0], idx[:, 0]


def main():
    sample_single_tri = reference_sample_single_tri()
    density = 0.05
    for seed in range(100):
        v, f = ref.random_mesh(400, seed=100 + seed, scale=0.5, extent=1.0)
        # the band condition, triangle by triangle: a triangle with n1 = n2 has a + b = 1 on its diagonal and is left out
        n1, n2, p0, v1, v2, r1, r2 = ref.triangle_grid(v, f, density)
        good = [t for t in range(len(f)) if ref.sample_triangle(int(n1[t]), int(n2[t]), p0[t], v1[t], v2[t])[1] >= SUM_BAND
                and min(abs(r - round(r)) for r in (r1[t], r2[t])) >= FLOOR_BAND][:160]
        v, f = v.reshape(-1, 3, 3)[good].reshape(-1, 3), np.arange(3 * len(good), dtype=np.int32).reshape(-1, 3)
        # degenerate rows: a repeated vertex, a collinear triple, a sliver with n1 = 0
        v = np.concatenate([v, np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 0, 1], [1e-3, 0, 1], [0, 0.987, 1]], np.float32)])
        n = len(v) - 6
        f = np.concatenate([f, np.array([[0, 0, 1], [n, n + 1, n + 2], [n + 3, n + 4, n + 5]], np.int32)])
        pts64, counts = reference_sampling(v, f, density, sample_single_tri)
        _, _, margins = ref.sample_surface(v, f, density)
        cloud = pts64.astype(np.float32)
        order = np.random.default_rng(seed).permutation(len(cloud))
        pair = ref.pair_margin(cloud, density)
        if margins["floor_margin"] < FLOOR_BAND or margins["sum_margin"] < SUM_BAND or pair < PAIR_BAND:
            continue
        break
    else:
        raise SystemExit("no seed satisfies the band condition")
    shuffled = cloud[order].astype(np.float64)
    mask_shuffled = reference_thinning(shuffled, density)          # in visiting order
    mask = np.zeros(len(cloud), bool)
    mask[order] = mask_shuffled
    mask_index_order = reference_thinning(cloud.astype(np.float64), density)
    gt = ref.surface_cloud(6000, seed=5, noise=0.02)
    gt[:, :2] *= 1.2
    thinned = cloud[mask]
    max_dist = 0.6
    d_d2s, i_d2s = reference_distances(thinned.astype(np.float64), gt.astype(np.float64), density)
    d_s2d, i_s2d = reference_distances(gt.astype(np.float64), thinned.astype(np.float64), density)
    out = dict(vertices=v, faces=f, density=np.float64(density), sample_points=pts64, sample_counts=counts, order=order.astype(np.int64), keep=mask,
               keep_index_order=mask_index_order, gt=gt, max_dist=np.float64(max_dist), dist_d2s=d_d2s, index_d2s=i_d2s.astype(np.int64),
               dist_s2d=d_s2d, index_s2d=i_s2d.astype(np.int64),
               mean_d2s=np.float64(d_d2s[d_d2s < max_dist].mean()), mean_s2d=np.float64(d_s2d[d_s2d < max_dist].mean()),
               floor_margin=np.float64(margins["floor_margin"]), sum_margin=np.float64(margins["sum_margin"]), pair_margin=np.float64(pair),
               seed=np.int64(seed))
    path = os.path.join(HERE, "mesh_eval.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; seed %d, %d triangles, %d points (%d sampled), %d kept, margins floor %.2e sum %.2e pair %.2e"
          % (path, os.path.getsize(path), seed, len(f), len(cloud), int(counts.sum()), int(mask.sum()), margins["floor_margin"], margins["sum_margin"], pair))


if __name__ == "__main__":
    main()
