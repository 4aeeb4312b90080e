"""Host restatement of the DTU-evaluation contract ("DTU evaluation"; header of ibgs_amd/csrc/dtu.hip) in numpy.  It shares no code
with the kernels or with ibgs_amd/dtu.py; sampling, thinning and the distances come from tests/mesh_eval_ref.py.  The dilation is the 2-D definition read
literally, the vertex rule is written with numpy f32 arrays, one rounded operation per line, the filters are f64."""
import numpy as np

from tests import mesh_eval_ref

F32 = np.float32


# ---- dilation --------------------------------------------------------------------------------------------------------------------------------------
def disc_offsets(r):
    """Every integer (dy, dx) with dx dx + dy dy <= r r."""
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def dilate(mask, r):
    """out[y, x] = OR of mask[y + dy, x + dx] over the disc, zero outside the image.  mask: (H, W), non-zero = set.  -> (H, W) bool."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    out = np.zeros((H, W), bool)
    for dy, dx in disc_offsets(int(r)):
        # out[y, x] |= m[y + dy, x + dx] for the (y, x) whose source lies inside the image
        y0, y1 = max(0, -dy), min(H, H - dy)
        x0, x1 = max(0, -dx), min(W, W - dx)
        if y0 < y1 and x0 < x1:
            out[y0:y1, x0:x1] |= m[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def dilate_all(masks, r):
    masks = np.asarray(masks)
    return np.stack([dilate(m, r) for m in masks]) if len(masks) else np.zeros(masks.shape, bool)


def pack_bits(masks):
    """(n, H, W) bool -> (n, H, ceil(W / 64)) int64: bit (x & 63) of word (x >> 6) is pixel x; bits at x >= W are zero."""
    m = np.asarray(masks) != 0
    n, H, W = m.shape
    WW = (W + 63) // 64
    words = np.zeros((n, H, WW), np.uint64)
    for x in range(W):
        words[:, :, x >> 6] |= m[:, :, x].astype(np.uint64) << np.uint64(x & 63)
    return words.view(np.int64)


def unpack_bits(words, W):
    w = np.asarray(words).view(np.uint64)
    x = np.arange(w.shape[-1] * 64)
    bits = (w[..., x >> 6] >> (x & 63).astype(np.uint64)) & np.uint64(1)
    return bits[..., :W] != 0, bits[..., W:] != 0          # (the image, the pad bits)


# ---- the vertex rule -------------------------------------------------------------------------------------------------------------------------------
def pixel_of(u, v, W, H):
    """The grid_sample(mode="nearest", align_corners=True) round trip of pixel coordinates (u, v), f32 arrays.  -> (valid, ix, iy)."""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    wm1, hm1 = F32(W - 1), F32(H - 1)
    with np.errstate(all="ignore"):
        gx = u / wm1
        gx = gx - F32(0.5)
        gx = gx * F32(2)
        gy = v / hm1
        gy = gy - F32(0.5)
        gy = gy * F32(2)
        valid = (gx > F32(-1)) & (gx < F32(1)) & (gy > F32(-1)) & (gy < F32(1))          # (false when either is NaN)
        fx = gx + F32(1)
        fx = fx / F32(2)
        fx = fx * wm1
        fx = np.rint(fx)          # ties to even
        fy = gy + F32(1)
        fy = fy / F32(2)
        fy = fy * hm1
        fy = np.rint(fy)
    assert gx.dtype == F32 and fx.dtype == F32
    ix = np.where(valid, fx, 0).astype(np.int64)
    iy = np.where(valid, fy, 0).astype(np.int64)
    return valid, ix, iy


def project(vertices, P):
    """(u, v) of every vertex under one 3 x 4 f32 matrix: c_r = ((P_r0 x + P_r1 y) + P_r2 z) + P_r3, u = c_0 / (c_2 + 1e-6f), v = c_1 / (c_2 + 1e-6f)."""
    p = np.asarray(vertices, F32)
    P = np.asarray(P, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = []
    with np.errstate(all="ignore"):
        for r in range(3):
            a = P[r, 0] * x
            b = P[r, 1] * y
            s = a + b
            b = P[r, 2] * z
            s = s + b
            s = s + P[r, 3]
            c.append(s)
        den = c[2] + F32(1e-6)
        u = c[0] / den
        v = c[1] / den
    assert u.dtype == F32 and den.dtype == F32
    return u, v, den


def view_passes(vertices, P, dilated):
    """(pass, valid) of every vertex for one view; dilated: (H, W) bool."""
    H, W = dilated.shape
    u, v, _ = project(vertices, P)
    valid, ix, iy = pixel_of(u, v, W, H)
    assert np.all(ix[valid] >= 0) and np.all(ix[valid] < W) and np.all(iy[valid] >= 0) and np.all(iy[valid] < H)
    return ~valid | dilated[iy, ix], valid


def cull_vertices(vertices, projections, dilated):
    """keep = AND over the views of (not valid or the dilated mask at the pixel); no view keeps everything.  dilated: (n, H, W) bool."""
    keep = np.ones(len(vertices), bool)
    for P, d in zip(np.asarray(projections, F32), dilated):
        keep &= view_passes(vertices, P, d)[0]
    return keep


# ---- compaction ------------------------------------------------------------------------------------------------------------------------------------
def cull_mesh(vertices, faces, keep, scale=1.0, offset=(0.0, 0.0, 0.0), attrs=()):
    """-> (vertices', faces', [attrs']): the kept vertices in index order at v * scale + offset in f32; faces whose three vertices are kept, re-indexed."""
    v, f, keep = np.asarray(vertices, F32), np.asarray(faces, np.int64), np.asarray(keep, bool)
    new = np.cumsum(keep) - 1
    fk = keep[f].all(axis=1) if len(f) else np.zeros(0, bool)
    out_v = v[keep] * F32(scale)
    out_v = out_v + np.asarray(offset, np.float64).astype(F32)[None, :]
    assert out_v.dtype == F32
    return out_v, new[f[fk]].astype(np.int32).reshape(-1, 3), [np.asarray(a)[keep] for a in attrs]


# ---- the point filters -----------------------------------------------------------------------------------------------------------------------------
def box_bounds(bb, patch):
    bb = np.asarray(bb, np.float64).astype(F32)
    lo = bb[0] - F32(patch)
    hi = bb[1] + F32(patch * 2)
    assert lo.dtype == F32 and hi.dtype == F32
    return lo, hi


def obs_mask_filter(points, obs_mask, bb, res, patch=60.0):
    """-> (inbound, in_obs), f64 on the f32 points (eval.py:98-110)."""
    p = np.asarray(points, F32).astype(np.float64)
    obs = np.asarray(obs_mask) != 0
    lo, hi = box_bounds(bb, patch)
    inbound = np.all((p >= lo.astype(np.float64)) & (p < hi.astype(np.float64)), axis=1)
    bb0 = np.asarray(bb, np.float64).astype(F32)[0].astype(np.float64)
    g = np.around((p - bb0) / float(res))          # ties to even
    on = np.all((g >= 0) & (g < np.array(obs.shape, np.float64)), axis=1)
    gi = np.where(on[:, None], g, 0).astype(np.int64)
    in_obs = inbound & on & obs[gi[:, 0], gi[:, 1], gi[:, 2]]
    return inbound, in_obs


def above_plane(points, plane):
    p = np.asarray(points, F32).astype(np.float64)
    P = np.asarray(plane, np.float64).reshape(4)
    return ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] > 0


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------------
def sampled_cloud(vertices, faces, density):
    return mesh_eval_ref.sample_surface(vertices, faces, density)[0].astype(F32)


def evaluate_dtu(vertices, faces, gt, obs_mask, bb, res, plane, density, max_dist, patch, order):
    """eval.py:43-157 from a mesh; order: the visiting order of the thinning (a permutation of the sampled cloud's indices)."""
    cloud = sampled_cloud(vertices, faces, density)
    thinned = cloud[mesh_eval_ref.downsample(cloud, density, order=order)]
    inbound, in_obs = obs_mask_filter(thinned, obs_mask, bb, res, patch)
    data_in = thinned[inbound]
    above = above_plane(gt, plane)
    out = mesh_eval_ref.chamfer(data_in, gt, max_dist, pred_query_mask=in_obs[inbound], gt_query_mask=above)
    out.update(n_sampled=len(cloud), n_thinned=len(thinned), n_inbound=int(inbound.sum()), n_in_obs=int(in_obs.sum()), n_above=int(above.sum()))
    # the same with the gt -> pred search among ALL thinned points: what the call must NOT compute
    out["all_thinned"] = mesh_eval_ref.chamfer(thinned, gt, max_dist, pred_query_mask=in_obs, gt_query_mask=above)
    return out


# ---- test inputs -----------------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up, f, W, H):
    """3 x 4 f32 K @ world_to_camera of a pinhole camera at `eye` looking at `target` (camera z forward, x right, y down), principal point at the centre."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    w2c = np.concatenate([R, (-R @ eye)[:, None]], 1)
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    return (K @ w2c).astype(F32)


VIEW_W, VIEW_H = 130, 67
VIEW2_SCALE = 2.0 ** -21          # view 2's matrix is scaled as a whole (the same pinhole image up to the 1e-6 of the divisor): its c_2 can then be -1e-6f exactly


def three_views():
    """(3, 3, 4) f32: cameras looking at the origin from -z, +x and -y.  View 0 has f = 64 at distance 4: a point at camera depth 32 lands on u = 2 x + 64.5,
    v = 2 y + 33 exactly (and 32 + 1e-6f rounds to 32)."""
    W, H = VIEW_W, VIEW_H
    P0 = look_at((0, 0, -4), (0, 0, 0), (0, -1, 0), 64.0, W, H)
    P1 = look_at((5, 0, 0), (0, 0, 0), (0, 0, 1), 70.0, W, H)
    P2 = look_at((0, -1.5, 0), (0, 0, 0), (0, 0, 1), 50.0, W, H) * F32(VIEW2_SCALE)          # (1e-6 / 2^-21 = 2.1: the image of a camera 3.6 away)
    return np.stack([P0, P1, P2]).astype(F32)


def blob_masks(seed=5):
    """(3, H, W) uint8 raw object masks: an off-centre ellipse and a few specks per view."""
    W, H = VIEW_W, VIEW_H
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = []
    for cx, cy, a, b in ((60.0, 30.0, 30.0, 16.0), (70.0, 36.0, 34.0, 18.0), (64.0, 33.0, 36.0, 20.0)):
        m = ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0
        m |= rng.uniform(size=(H, W)) < 0.002
        out.append(m)
    return np.stack(out).astype(np.uint8)


def zero_divisor_vertex(P):
    """A vertex (0, y, 0) whose c_2 under P (view 2: c_2 = P[2,1] y + P[2,3]) is -1e-6f exactly, so that the divisor c_2 + 1e-6f is zero."""
    e = F32(1e-6)
    y = F32(-(np.float64(e) + np.float64(P[2, 3])) / np.float64(P[2, 1]))
    assert F32(F32(P[2, 1] * y) + P[2, 3]) == -e and F32(F32(F32(P[2, 1] * y) + P[2, 3]) + e) == 0
    return np.array([0.0, y, 0.0], F32)


def cull_vertices_case(n_random=50_000, seed=6):
    """Vertices for three_views(): a box larger than every frustum, the half-pixel lattice of view 0, points behind the cameras, the zero-divisor vertex."""
    rng = np.random.default_rng(seed)
    P = three_views()
    box = rng.uniform(-4.0, 4.0, (n_random, 3)).astype(F32)
    k, j = np.meshgrid(np.arange(-2, VIEW_W + 2), np.arange(-2, VIEW_H + 2), indexing="ij")
    lattice = np.stack([(k.ravel() - 64) / 2.0, (j.ravel() + 0.5 - 33) / 2.0, np.full(k.size, 28.0)], 1).astype(F32)          # u = k + 0.5, v = j + 0.5 in view 0
    behind = np.concatenate([rng.uniform(-1, 1, (300, 3)) + [0, 0, -6], rng.uniform(-1, 1, (300, 3)) + [7, 0, 0], rng.uniform(-1, 1, (300, 3)) + [0, -6, 0]]).astype(F32)
    return np.concatenate([box, lattice, behind, zero_divisor_vertex(P[2])[None]]), P, len(box), len(lattice)


def grid_mesh_case():
    """A 33 x 32 grid in the plane z = 0 (1984 faces) that spans the border of the dilated masks, plus: vertex V-3, which is kept but whose only face has a
    culled corner; a face that repeats an index.  -> (vertices, faces, colors, normals)."""
    from tests import mesh_ref
    v, f = mesh_ref.grid(33, 32, 0.125, origin=(-2.0, -2.0, 0.0))
    n = len(v)
    extra = np.array([[0.0, 0.0, 0.5], [-2.9, 0.0, 0.0], [-2.9, 0.1, 0.0]], F32)          # kept; culled; culled
    v = np.concatenate([v, extra])
    centre = 16 * 32 + 16
    f = np.concatenate([f[:1000], np.array([[n, n + 1, n + 2], [centre, centre, centre + 1]], np.int32), f[1000:]])
    rng = np.random.default_rng(8)
    return v, f.astype(np.int32), rng.uniform(0, 1, v.shape).astype(F32), rng.normal(size=v.shape).astype(F32)


OBS_SHAPE = (12, 9, 7)


def filter_case(n_random=20_000, seed=9):
    """-> (points, obs_mask, bb, res, patch): random points around a 12 x 9 x 7 grid, points exactly on lo and on hi, and points on half-voxel ties."""
    rng = np.random.default_rng(seed)
    obs = (rng.uniform(size=OBS_SHAPE) < 0.6).astype(np.uint8)
    res, patch = 0.5, 0.75
    bb = np.array([[-3.0, 2.0, 1.0], [-3.0 + 11 * res, 2.0 + 8 * res, 1.0 + 6 * res]], F32)
    lo, hi = box_bounds(bb, patch)
    p = rng.uniform(lo - 1, hi + 1, (n_random, 3)).astype(F32)
    inside = rng.uniform(bb[0], bb[1], (600, 3)).astype(F32)
    on_lo, on_hi, tie = inside[:200].copy(), inside[200:400].copy(), inside[400:].copy()
    for k in range(3):
        on_lo[k::3, k] = lo[k]
        on_hi[k::3, k] = hi[k]
        tie[k::3, k] = bb[0, k] + F32(res) * (rng.integers(-1, OBS_SHAPE[k], len(tie[k::3])) + F32(0.5))          # (p - bb0) / res = k + 1/2 exactly
    just = np.concatenate([np.nextafter(on_lo, F32(-np.inf)), np.nextafter(on_hi, F32(-np.inf))])
    return np.concatenate([p, on_lo, on_hi, tie, just]), obs, bb, res, patch


def eval_case(seed=10):
    """-> (gt, obs_mask, bb, res, plane, density, max_dist, patch) for grid_mesh_case(): the box with its patch margin cuts the mesh, so some thinned points are
    out of bounds, and gt points beyond it find a nearer neighbour among all thinned points than among the in-bound ones."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-2.3, 2.3, (30_000, 2))
    z = 0.05 * np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1]) + 0.01 * rng.normal(size=len(xy))
    gt = np.concatenate([xy, z[:, None]], 1).astype(F32)
    obs = (rng.uniform(size=OBS_SHAPE) < 0.6).astype(np.uint8)
    res, patch = 0.25, 0.25
    bb = np.array([[-1.5, -1.75, -0.5], [-1.5 + 11 * res, -1.75 + 8 * res, -0.5 + 6 * res]], F32)
    plane = np.array([0.3, 1.0, 0.2, 0.4])
    return gt, obs, bb, res, plane, 0.05, 0.3, patch
