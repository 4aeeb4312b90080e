"""numpy restatement of the TSDF contract (header of ibgs_amd/csrc/tsdf.hip): integration in f32 in the stated operation order,
marching cubes from the library's exported table with the stated vertex normals and output order.  Every f32 operation below is one IEEE operation
on np.float32 operands (no python floats reach an f32 expression), so the results are those of the kernels (compiled without contraction)."""
import numpy as np

from ibgs_amd.tsdf import BLOCK, KEY_BIAS, VOXELS, pack_keys, pose_inverse

f32 = np.float32
# voxel l = i + 8 j + 64 k: LOCAL[l] = (i, j, k)
_l = np.arange(VOXELS)
LOCAL = np.stack([_l & 7, (_l >> 3) & 7, _l >> 6], axis=1)


def _other(a):
    return [x for x in range(3) if x != a]


class RefVolume:
    def __init__(self, voxel_length, sdf_trunc):
        self.v, self.tau = f32(voxel_length), f32(sdf_trunc)
        self.index = {}          # packed key -> row
        self.coords = np.zeros((0, 3), np.int64)
        self.tsdf = np.zeros((0, VOXELS), f32)
        self.weight = np.zeros((0, VOXELS), f32)
        self.color = np.zeros((0, VOXELS, 3), f32)
        self.ignored = 0
        self.last_active = None          # packed keys of the last view's active blocks

    def _rows(self, coords):
        keys = pack_keys(coords)
        new = [i for i, k in enumerate(keys) if int(k) not in self.index]
        if new:
            n0 = len(self.index)
            for j, i in enumerate(new):
                self.index[int(keys[i])] = n0 + j
            self.coords = np.concatenate([self.coords, coords[new]])
            z = np.zeros((len(new), VOXELS), f32)
            self.tsdf = np.concatenate([self.tsdf, z]); self.weight = np.concatenate([self.weight, z])
            self.color = np.concatenate([self.color, np.zeros((len(new), VOXELS, 3), f32)])
        return np.array([self.index[int(k)] for k in keys], np.int64)

    def allocation(self, depth, fx, fy, cx, cy, world_to_camera, depth_trunc=np.inf):
        """The view's active block coordinates (unique, (n, 3)) and the per-point block ranges' float bounds (for tie diagnostics)."""
        fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
        M = pose_inverse(world_to_camera)
        depth = np.asarray(depth, f32)
        valid = (depth > 0) & (depth <= f32(depth_trunc))
        vv, uu = np.nonzero(valid)
        d = depth[vv, uu]
        xc = ((uu.astype(f32) - cx) / fx) * d
        yc = ((vv.astype(f32) - cy) / fy) * d
        p = np.stack([((M[r, 0] * xc + M[r, 1] * yc) + M[r, 2] * d) + M[r, 3] for r in range(3)], axis=1)
        B = self.v * f32(BLOCK)
        lo = np.floor((p - self.tau) / B)
        hi = np.floor((p + self.tau) / B)
        ok = np.all(lo >= f32(-KEY_BIAS), axis=1) & np.all(hi <= f32(KEY_BIAS - 1), axis=1)
        ignored = int((~ok).sum())
        lo, hi = lo[ok].astype(np.int64), hi[ok].astype(np.int64)
        span = (hi - lo).max(axis=0) + 1 if len(lo) else np.zeros(3, np.int64)
        out = []
        for dz in range(int(span[2])):
            for dy in range(int(span[1])):
                for dx in range(int(span[0])):
                    c = lo + np.array([dx, dy, dz])
                    m = np.all(c <= hi, axis=1)
                    out.append(c[m])
        coords = np.unique(np.concatenate(out), axis=0) if out else np.zeros((0, 3), np.int64)
        return coords, ignored, (p, lo, hi)

    def integrate(self, depth, fx, fy, cx, cy, world_to_camera, color=None, depth_trunc=np.inf):
        coords, ignored, _ = self.allocation(depth, fx, fy, cx, cy, world_to_camera, depth_trunc)
        self.ignored += ignored
        rows = self._rows(coords)
        self.last_active = pack_keys(coords)
        if len(rows) == 0:
            return
        fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
        Wm = np.asarray(world_to_camera, f32)
        depth = np.asarray(depth, f32)
        H, W = depth.shape
        I = coords[:, None, :] * BLOCK + LOCAL[None]                     # (n, 512, 3) voxel coordinates
        X = (I.astype(f32) + f32(0.5)) * self.v
        x = ((Wm[0, 0] * X[..., 0] + Wm[0, 1] * X[..., 1]) + Wm[0, 2] * X[..., 2]) + Wm[0, 3]
        y = ((Wm[1, 0] * X[..., 0] + Wm[1, 1] * X[..., 1]) + Wm[1, 2] * X[..., 2]) + Wm[1, 3]
        z = ((Wm[2, 0] * X[..., 0] + Wm[2, 1] * X[..., 1]) + Wm[2, 2] * X[..., 2]) + Wm[2, 3]
        front = z > 0
        zs = np.where(front, z, f32(1))
        with np.errstate(invalid="ignore", over="ignore"):
            fu = np.floor(((fx * x) / zs + cx) + f32(0.5))
            fv = np.floor(((fy * y) / zs + cy) + f32(0.5))
        inside = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        pu = np.where(inside, fu, 0).astype(np.int64); pv = np.where(inside, fv, 0).astype(np.int64)
        d = depth[pv, pu]
        ok = inside & (d > 0) & (d <= f32(depth_trunc))
        ra = (pu.astype(f32) - cx) / fx
        rb = (pv.astype(f32) - cy) / fy
        sdf = (d - z) * np.sqrt((f32(1) + ra * ra) + rb * rb)
        ok &= sdf > -self.tau
        t = np.minimum(f32(1), sdf / self.tau)
        w = self.weight[rows]
        w1 = w + f32(1)
        self.tsdf[rows] = np.where(ok, (self.tsdf[rows] * w + t) / w1, self.tsdf[rows])
        if color is not None:
            C = np.asarray(color, f32)[:, pv, pu]                        # (3, n, 512)
            for ch in range(3):
                old = self.color[rows, :, ch]
                self.color[rows, :, ch] = np.where(ok, (old * w + C[ch]) / w1, old)
        self.weight[rows] = np.where(ok, w1, w)

    def blocks(self):
        keys = pack_keys(self.coords)
        o = np.argsort(keys, kind="stable")
        return {"keys": keys[o], "coords": self.coords[o], "tsdf": self.tsdf[o], "weight": self.weight[o], "color": self.color[o]}


# ---- marching cubes -------------------------------------------------------------------------------------------------------------------------

def tri_counts(table):
    t = np.asarray(table).reshape(256, 16)
    return np.array([int(np.sum(t[c, 0:15:3] >= 0)) for c in range(256)])


def marching_cubes(blocks, voxel_length, table):
    """blocks: RefVolume.blocks() / TSDFVolume.blocks().  Returns (vertices (V,3), faces (F,3) int32, colors (V,3), normals (V,3)) in the contract's
    order: blocks by key, voxel l, edge axis (vertices) / triangle (faces)."""
    v = f32(voxel_length)
    tab = np.asarray(table, np.int64).reshape(256, 16)
    ntri = tri_counts(tab)
    coords = np.asarray(blocks["coords"], np.int64)
    if len(coords) == 0:
        z = np.zeros((0, 3), f32)
        return z, np.zeros((0, 3), np.int32), z, z
    g0 = coords.min(0) * BLOCK - 1
    dims = (coords.max(0) - coords.min(0) + 1) * BLOCK + 2
    T = np.zeros(dims, f32); OK = np.zeros(dims, bool); C = np.zeros(tuple(dims) + (3,), f32)
    alloc = np.zeros(dims, bool)
    for n, bc in enumerate(coords):
        o = bc * BLOCK - g0
        sl = (slice(o[0], o[0] + 8), slice(o[1], o[1] + 8), slice(o[2], o[2] + 8))
        T[sl] = blocks["tsdf"][n].reshape(8, 8, 8).transpose(2, 1, 0)
        OK[sl] = blocks["weight"][n].reshape(8, 8, 8).transpose(2, 1, 0) > 0
        C[sl] = blocks["color"][n].reshape(8, 8, 8, 3).transpose(2, 1, 0, 3)
        alloc[sl] = True
    neg = T < 0
    X, Y, Z = dims

    def shifted(arr, off, fill):
        """arr[p + off] for every p of the grid (fill outside)."""
        out = np.full(arr.shape, fill, arr.dtype)
        src = tuple(slice(max(0, o), dims[r] + min(0, o)) for r, o in enumerate(off))
        dst = tuple(slice(max(0, -o), dims[r] - max(0, o)) for r, o in enumerate(off))
        out[dst] = arr[src]
        return out

    corner = [np.array([n & 1, (n >> 1) & 1, n >> 2]) for n in range(8)]
    cell_ok = np.ones(dims, bool)
    case = np.zeros(dims, np.int64)
    for n in range(8):
        cell_ok &= shifted(OK, corner[n], False)
        case |= shifted(neg, corner[n], False).astype(np.int64) << n
    case = np.where(cell_ok, case, 0)

    # vertices: owner p, axis a
    exists = []
    for a in range(3):
        ea = np.zeros(3, np.int64); ea[a] = 1
        cross = OK & shifted(OK, ea, False) & (neg != shifted(neg, ea, False))
        b, c = _other(a)
        around = np.zeros(dims, bool)
        for k in range(4):
            off = np.zeros(3, np.int64); off[b] = -(k & 1); off[c] = -(k >> 1)
            around |= shifted(cell_ok, off, False)
        exists.append(cross & around & alloc)
    gidx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1) + g0      # global voxel coordinates
    keyg = pack_keys((gidx.reshape(-1, 3) // BLOCK)).reshape(dims)
    lg = ((gidx[..., 0] % 8) + 8 * (gidx[..., 1] % 8) + 64 * (gidx[..., 2] % 8))
    own = [np.argwhere(exists[a]) for a in range(3)]
    allp = np.concatenate([own[a] for a in range(3)])
    alla = np.concatenate([np.full(len(own[a]), a) for a in range(3)])
    order = np.lexsort((alla, lg[tuple(allp.T)], keyg[tuple(allp.T)]))
    allp, alla = allp[order], alla[order]
    V = len(allp)
    vid = np.full((3,) + tuple(dims), -1, np.int64)
    vid[alla, allp[:, 0], allp[:, 1], allp[:, 2]] = np.arange(V)

    def edge_point(m, e):
        """position (n,3) and t (n,) and corner grid indices of cell-edge e (array (n,)) of cells with min corner m (n,3 grid indices)."""
        a = e // 4; k = e % 4
        off = np.zeros((len(e), 3), np.int64)
        for aa in range(3):
            b, c = _other(aa)
            sel = a == aa
            off[sel, b] = k[sel] & 1
            off[sel, c] = k[sel] >> 1
        o0 = m + off
        o1 = o0.copy(); o1[np.arange(len(e)), a] += 1
        f0 = T[tuple(o0.T)]; f1 = T[tuple(o1.T)]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = f0 / (f0 - f1)
        x0 = ((o0 + g0).astype(f32) + f32(0.5)) * v
        x1 = ((o1 + g0).astype(f32) + f32(0.5)) * v
        return x0 + t[:, None] * (x1 - x0), t, o0, o1

    pos, t, o0, o1 = edge_point(allp, 4 * alla)
    col = C[tuple(o0.T)] + t[:, None] * (C[tuple(o1.T)] - C[tuple(o0.T)])
    nrm = np.zeros((V, 3), f32)
    for k in range(4):
        m = allp.copy()
        for aa in range(3):
            b, c = _other(aa)
            sel = alla == aa
            m[sel, b] -= k & 1
            m[sel, c] -= k >> 1
        mok = cell_ok[tuple(m.T)]
        mcs = case[tuple(m.T)]
        me = 4 * alla + k
        for tr in range(5):
            es = [tab[mcs, 3 * tr + j] for j in range(3)]
            use = mok & (tr < ntri[mcs]) & ((es[0] == me) | (es[1] == me) | (es[2] == me))
            if not use.any():
                continue
            P = [edge_point(m[use], es[j][use])[0] for j in range(3)]
            u = P[1] - P[0]; w = P[2] - P[0]
            cr = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
            nrm[use] = nrm[use] + cr
    ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    nz = ln > 0
    nrm[nz] = nrm[nz] / ln[nz, None]

    # faces: cell p (valid, in an allocated block), triangle tr
    cells = np.argwhere(cell_ok & alloc)
    cells = cells[np.lexsort((lg[tuple(cells.T)], keyg[tuple(cells.T)]))]
    cs = case[tuple(cells.T)]
    faces = []
    fkey = []
    for tr in range(5):
        has = tr < ntri[cs]
        if not has.any():
            continue
        idx = []
        for j in range(3):
            e = tab[cs[has], 3 * tr + j]
            a = e // 4; k = e % 4
            q = cells[has].copy()
            for aa in range(3):
                b, c = _other(aa)
                sel = a == aa
                q[sel, b] += k[sel] & 1
                q[sel, c] += k[sel] >> 1
            idx.append(vid[a, q[:, 0], q[:, 1], q[:, 2]])
        faces.append(np.stack(idx, 1))
        fkey.append(np.stack([np.nonzero(has)[0], np.full(int(has.sum()), tr)], 1))
    if faces:
        faces = np.concatenate(faces); fkey = np.concatenate(fkey)
        faces = faces[np.lexsort((fkey[:, 1], fkey[:, 0]))]
    else:
        faces = np.zeros((0, 3), np.int64)
    assert (faces >= 0).all(), "a face uses an edge without a vertex"
    return pos.astype(f32), faces.astype(np.int32), col.astype(f32), nrm


# ---- analytic scenes shared by the host and GPU tests ------------------------------------------------------------------------------------------

def look_at(eye, target=(0.0, 0.0, 0.0)):
    """4 x 4 world_to_camera (x right, y down, z forward) of a camera at `eye` looking at `target` (float64)."""
    eye = np.asarray(eye, np.float64); z = np.asarray(target, np.float64) - eye; z /= np.linalg.norm(z)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])          # rows: world -> camera
    M = np.identity(4); M[:3, :3] = R; M[:3, 3] = -R @ eye
    return M


def fibonacci_directions(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n); theta = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1)


def sphere_view(world_to_camera, W, H, fx, fy, cx, cy, radius, center=(0.0, 0.0, 0.0)):
    """Depth (H, W) f32 (0 off the sphere) and colour (3, H, W) f32 (0.5 + 0.5 * outward normal) of a sphere, in float64 then rounded."""
    M = np.asarray(world_to_camera, np.float64)
    R, t = M[:3, :3], M[:3, 3]
    o = -R.T @ t - np.asarray(center, np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)          # camera rays with z = 1: the ray parameter is the depth
    dw = rc @ R          # (R^T rc) per pixel
    a = (dw * dw).sum(-1); b = 2 * (dw @ o); c = o @ o - radius ** 2
    disc = b * b - 4 * a * c
    hit = disc > 0
    s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), 0)
    hit &= s > 0
    depth = np.where(hit, s, 0).astype(np.float32)
    p = o + s[..., None] * dw
    col = np.where(hit[..., None], 0.5 + 0.5 * p / radius, 0).transpose(2, 0, 1).astype(np.float32)
    return depth, col


PLANE = dict(W=160, H=120, fx=100.0, fy=100.0, cx=80.0, cy=60.0, z0=1.0, voxel=0.02, offsets=((0, 0), (0.1, 0), (-0.1, 0), (0, 0.1), (0, -0.1)))


def plane_views(p=PLANE):
    """A fronto-parallel plane z = z0 seen by cameras that look along +z from (ox, oy, 0): [(depth, world_to_camera)]."""
    out = []
    for ox, oy in p["offsets"]:
        M = np.identity(4); M[0, 3] = -ox; M[1, 3] = -oy
        out.append((np.full((p["H"], p["W"]), p["z0"], np.float32), M))
    return out


def plane_closed_form(X, p=PLANE):
    """float64 closed form of tsdf and weight at voxel centres X (n, 3) after integrating plane_views(): the mean over the views that update
    the voxel of min(1, (d - z) m / tau), m = sqrt(1 + ((pu - cx) / fx)^2 + ((pv - cy) / fy)^2), and their number."""
    tau = 4 * p["voxel"]
    acc = np.zeros(len(X)); cnt = np.zeros(len(X))
    for ox, oy in p["offsets"]:
        x, y, z = X[:, 0] - ox, X[:, 1] - oy, X[:, 2]
        pu = np.floor(p["fx"] * x / z + p["cx"] + 0.5); pv = np.floor(p["fy"] * y / z + p["cy"] + 0.5)
        m = np.sqrt(1 + ((pu - p["cx"]) / p["fx"]) ** 2 + ((pv - p["cy"]) / p["fy"]) ** 2)
        sdf = (p["z0"] - z) * m
        use = (z > 0) & (pu >= 0) & (pu < p["W"]) & (pv >= 0) & (pv < p["H"]) & (sdf > -tau)
        acc += np.where(use, np.minimum(1, sdf / tau), 0); cnt += use
    return np.where(cnt > 0, acc / np.maximum(cnt, 1), 0), cnt


def axis_voxels(blocks, voxel, ox=0.0, oy=0.0):
    """(tsdf, weight, centres) of the allocated voxels in the column nearest the optical axis through (ox, oy)."""
    I = blocks["coords"][:, None, :] * BLOCK + LOCAL[None]
    i0 = int(np.floor(ox / voxel)); j0 = int(np.floor(oy / voxel))
    sel = (I[..., 0] == i0) & (I[..., 1] == j0)
    X = (I[sel].astype(np.float64) + 0.5) * voxel
    return blocks["tsdf"][sel], blocks["weight"][sel], X
