"""DTU evaluation on the MI355X: what the reference's DTU scripts do between a mesh and its Chamfer distance, which runs on the host through cv2, skimage,
torch's CPU grid_sample, trimesh and numpy (scripts/eval_dtu/evaluate_single_scene.py:53-95, eval.py:43-157): dilate the object masks, cull the mesh against
them, sample and thin its surface, keep the points inside the bounding box and the observation mask, drop the ground truth below the ground plane, and take
the Chamfer distance with the gt -> pred search among the in-bound points.  The sibling of registration.evaluate_tnt:

    obs_mask, bb, res, plane = dtu.read_obs_mask("ObsMask24_10.mat", "Plane24.mat")
    cull = dtu.Cull(projections, masks, radius=24, scale=scale_mat[0, 0], offset=scale_mat[:3, 3])
    scores = dtu.evaluate_dtu(mesh, gt_points, obs_mask, bb, res, plane, cull=cull)          # {"mean_d2s", "mean_s2d", "overall", ...}

The contract is this project's own statement of those stages ("DTU evaluation"; header of ibgs_amd/csrc/dtu.hip); tests/dtu_ref.py
restates it.  Dilated masks, keep masks, culled meshes and filter masks are a pure function of the inputs (bit-identical from run to run).

HIP only (C ABI include/ibgs_dtu.h): CPU tensors are refused, every argument is checked before any GPU work, every kernel runs on torch's current stream,
inputs are never written.  Each call that sizes an output or can fail on its data reads a few words back (it waits for the stream): the docstrings say
which."""
import ctypes
from typing import NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _device, _lib, mesh_eval
from .tsdf import TriangleMesh


class MaskBits(NamedTuple):
    """Dilated masks as bits: bit (x & 63) of words[i, y, x >> 6] is pixel (y, x) of view i; bits at x >= W are zero."""
    words: torch.Tensor          # (n, H, ceil(W / 64)) int64
    H: int
    W: int


class ObsFilter(NamedTuple):
    inbound: torch.Tensor        # (N,) bool: inside the bounding box with its patch margin
    in_obs: torch.Tensor         # (N,) bool: inbound, and on a set voxel of the observation mask


class Cull(NamedTuple):
    """The mask culling evaluate_dtu applies first (the arguments of cull_mesh)."""
    projections: torch.Tensor
    masks: Union[torch.Tensor, MaskBits]
    radius: int = 24
    scale: float = 1.0
    offset: Sequence[float] = (0.0, 0.0, 0.0)


class DTUError(RuntimeError):
    pass


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------------
def _new_state(dev):
    return _device.zeros_state(dev, _lib.DTU_STATE_WORDS)


def _raise_on(s, what, V=None):
    """s: the state words on the host."""
    if s[_lib.DTU_BAD_FACES]:
        raise DTUError("%s: mesh.faces holds %d triangle(s) with a vertex index outside [0, %s)" % (what, s[_lib.DTU_BAD_FACES], V))
    if s[_lib.DTU_BAD_POINTS]:
        raise ValueError("%s: %d point(s) with a non-finite coordinate" % (what, s[_lib.DTU_BAD_POINTS]))
    if s[_lib.DTU_OVERRUN]:
        raise DTUError("%s: library fault: %d access(es) out of range" % (what, s[_lib.DTU_OVERRUN]))


def _check_mesh(mesh):
    """(V, F) of a mesh with all four arrays; shapes and dtypes only (where the tensors live is settled last, with the other arguments')."""
    v, f = mesh_eval._check_mesh(mesh)
    try:
        c, n = mesh.colors, mesh.normals
    except AttributeError:
        raise TypeError("mesh must be a tsdf.TriangleMesh (vertices, faces, colors, normals), got %s" % type(mesh).__name__) from None
    V = int(v.shape[0])
    for name, t in (("colors", c), ("normals", n)):
        if not torch.is_tensor(t):
            raise TypeError("mesh.%s must be a tensor, got %s" % (name, type(t).__name__))
        if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (V, 3):
            raise ValueError("mesh.%s must be (%d, 3) float32, one row per vertex, got %s %s" % (name, V, tuple(t.shape), t.dtype))
    return V, int(f.shape[0])


def _check_radius(radius):
    try:
        r = int(radius)
    except (TypeError, ValueError):
        raise TypeError("radius must be an integer, got %s" % type(radius).__name__) from None
    if r != radius or not 0 <= r <= _lib.DTU_MAX_RADIUS:
        raise ValueError("radius must be an integer in 0 .. %d, got %r" % (_lib.DTU_MAX_RADIUS, radius))
    return r


def _check_masks(masks):
    if not torch.is_tensor(masks):
        raise TypeError("masks must be a tensor or a MaskBits, got %s" % type(masks).__name__)
    if masks.dtype not in (torch.uint8, torch.bool) or masks.dim() != 3:
        raise ValueError("masks must be (n, H, W) uint8 or bool, got %s %s" % (tuple(masks.shape), masks.dtype))
    n, H, W = (int(x) for x in masks.shape)
    if H < 2 or W < 2 or H > _lib.DTU_MAX_SIDE or W > _lib.DTU_MAX_SIDE:
        raise ValueError("masks must have 2 <= H, W <= %d, got H %d, W %d" % (_lib.DTU_MAX_SIDE, H, W))
    if n * H * ((W + 63) // 64) >= 1 << 32:
        raise ValueError("masks too large: n %d, H %d, W %d (limit: n H ceil(W / 64) < 2^32)" % (n, H, W))
    return masks


def _check_bits(mb):
    try:
        words, H, W = mb.words, int(mb.H), int(mb.W)
    except (AttributeError, TypeError, ValueError):
        raise TypeError("mask_bits must be a MaskBits, got %s" % type(mb).__name__) from None
    if not torch.is_tensor(words):
        raise TypeError("mask_bits.words must be a tensor, got %s" % type(words).__name__)
    if H < 2 or W < 2 or H > _lib.DTU_MAX_SIDE or W > _lib.DTU_MAX_SIDE:
        raise ValueError("mask_bits must have 2 <= H, W <= %d, got H %d, W %d" % (_lib.DTU_MAX_SIDE, H, W))
    if words.dtype != torch.int64 or words.dim() != 3 or tuple(words.shape[1:]) != (H, (W + 63) // 64):
        raise ValueError("mask_bits.words must be (n, %d, %d) int64, got %s %s" % (H, (W + 63) // 64, tuple(words.shape), words.dtype))
    return MaskBits(words, H, W)


def _check_projections(p, n=None):
    if not torch.is_tensor(p):
        raise TypeError("projections must be a tensor, got %s" % type(p).__name__)
    if p.dtype != torch.float32 or p.dim() != 3 or tuple(p.shape[1:]) != (3, 4):
        raise ValueError("projections must be (n, 3, 4) float32, got %s %s" % (tuple(p.shape), p.dtype))
    if n is not None and p.shape[0] != n:
        raise ValueError("projections holds %d view(s), the masks %d" % (p.shape[0], n))
    return p


def _check_move(scale, offset):
    try:
        scale = float(scale)
        off = np.asarray(offset, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError("scale must be a number and offset three numbers") from None
    if off.shape[0] != 3 or not (np.isfinite(scale) and np.all(np.isfinite(off))):
        raise ValueError("scale must be finite and offset three finite numbers, got %r, %r" % (scale, offset))
    return scale, (ctypes.c_float * 3)(*off.tolist())


def _check_masks_or_bits(masks, radius):
    """-> (radius, MaskBits or None, raw masks or None), checked."""
    radius = _check_radius(radius)
    if isinstance(masks, MaskBits):
        return radius, _check_bits(masks), None
    return radius, None, _check_masks(masks)


# ---- dilation ------------------------------------------------------------------------------------------------------------------------------------------
def _dilate_async(masks, radius):
    n, H, W = (int(x) for x in masks.shape)
    dev, WW = masks.device, (W + 63) // 64
    nbytes = _lib.load().ibgs_dtu_required_dilate_scratch(n, H, W)
    if nbytes == 0:
        raise ValueError("masks too large: n %d, H %d, W %d" % (n, H, W))
    with torch.cuda.device(dev):
        words = torch.empty(n, H, WW, dtype=torch.int64, device=dev)
    if n:
        scratch = _device.scratch(dev, nbytes)
        _device.call(dev, "ibgs_dtu_dilate", n, H, W, radius, masks.view(torch.uint8).data_ptr(), scratch.data_ptr(), nbytes, words.data_ptr())
    return MaskBits(words, H, W)


def dilate_masks(masks, radius=24):
    """The binary dilation evaluate_single_scene.py:60-66 applies to every object mask (skimage's disc footprint, zero outside the image):
    out[y, x] = OR of masks[y + dy, x + dx] over the integer (dx, dy) with dx^2 + dy^2 <= radius^2 inside the image.  masks: (n, H, W) uint8 or bool on the
    device, non-zero = set; H, W >= 2, 0 <= radius <= 255, n >= 0.  -> MaskBits(words (n, H, ceil(W / 64)) int64, H, W).  Nothing is read back."""
    radius = _check_radius(radius)
    masks = _check_masks(masks)
    masks, = _device.check_cuda("dtu", ("masks", masks))
    return _dilate_async(masks, radius)


# ---- culling -------------------------------------------------------------------------------------------------------------------------------------------
def _cull_vertices_async(vertices, projections, bits, state):
    V, n, dev = int(vertices.shape[0]), int(projections.shape[0]), vertices.device
    with torch.cuda.device(dev):
        keep = torch.empty(V, dtype=torch.uint8, device=dev)
    _device.call(dev, "ibgs_dtu_cull_vertices", V, vertices.data_ptr(), n, projections.data_ptr(), bits.H, bits.W, bits.words.data_ptr(), keep.data_ptr(),
                 state.data_ptr())
    return keep


def cull_vertices(vertices, projections, mask_bits):
    """evaluate_single_scene.py:68-88: keep[v] iff every view either does not see vertex v or sees it on a set bit of its dilated mask.  vertices (V, 3) f32;
    projections (n, 3, 4) f32, rows 0..2 of K @ world_to_camera; mask_bits from dilate_masks with the same n.  Everything in f32, one rounding per operation,
    torch's CPU grid_sample(mode="nearest", align_corners=True) chain reproduced (header of csrc/dtu.hip).  n = 0 keeps every vertex; points behind a camera
    get no special treatment.  -> (V,) bool on the device.  One host read-back, at the end: the state words."""
    vertices = _device.check_points("vertices", vertices)
    bits = _check_bits(mask_bits)
    projections = _check_projections(projections, int(bits.words.shape[0]))
    vertices, projections, words = _device.check_cuda("dtu", ("vertices", vertices), ("projections", projections), ("mask_bits.words", bits.words))
    state = _new_state(vertices.device)
    keep = _cull_vertices_async(vertices, projections, MaskBits(words, bits.H, bits.W), state)
    _raise_on(state.cpu().tolist(), "cull_vertices")          # (waits for the stream)
    return keep.view(torch.bool)


def _check_cull(mesh, projections, masks, radius, scale, offset):
    """Every shape and value check of a cull.  -> (the (name, tensor) pairs that must live on one device, the rest)."""
    V, F = _check_mesh(mesh)
    radius, bits, raw = _check_masks_or_bits(masks, radius)
    n = int(bits.words.shape[0]) if bits is not None else int(raw.shape[0])
    projections = _check_projections(projections, n)
    scale, off = _check_move(scale, offset)
    m_t = ("masks", raw) if raw is not None else ("masks.words", bits.words)
    named = (("mesh.vertices", mesh.vertices), ("mesh.faces", mesh.faces), ("mesh.colors", mesh.colors), ("mesh.normals", mesh.normals),
             ("projections", projections), m_t)
    return named, (V, F, radius, bits, raw, scale, off)


def _cull_mesh(tensors, rest):
    """-> (TriangleMesh, V, F).  tensors: _check_cull's six, through _device.check_cuda (on one device, contiguous); rest: its second result."""
    V, F, radius, bits, raw, scale, off = rest
    vertices, faces, colors, normals, projections, m = tensors
    dev = vertices.device
    bits = _dilate_async(m, radius) if raw is not None else MaskBits(m, bits.H, bits.W)
    lib = _lib.load()
    nbytes = lib.ibgs_dtu_required_cull_scratch(V, F)
    if nbytes == 0:
        raise ValueError("mesh too large: V %d, F %d" % (V, F))
    scratch, state = _device.scratch(dev, nbytes), _new_state(dev)
    keep = _cull_vertices_async(vertices, projections, bits, state)
    _device.call(dev, "ibgs_dtu_cull_count", V, F, faces.data_ptr(), keep.data_ptr(), scratch.data_ptr(), nbytes, state.data_ptr())
    s = state.cpu().tolist()          # (waits for the stream)
    _raise_on(s, "cull_mesh", V)
    V2, F2 = s[_lib.DTU_VERTICES_OUT], s[_lib.DTU_FACES_OUT]
    with torch.cuda.device(dev):
        out_v, out_c, out_n = (torch.empty(V2, 3, dtype=torch.float32, device=dev) for _ in range(3))
        out_f = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    _device.call(dev, "ibgs_dtu_cull_emit", V, F, vertices.data_ptr(), faces.data_ptr(), colors.data_ptr(), normals.data_ptr(), scratch.data_ptr(), nbytes, scale, off,
                 V2, F2, out_v.data_ptr(), out_f.data_ptr(), out_c.data_ptr(), out_n.data_ptr(), state.data_ptr())
    _raise_on(state.cpu().tolist(), "cull_mesh", V)          # (an emit outside the outputs would be a library fault: raise rather than hand out a partial mesh)
    return TriangleMesh(out_v, out_f, out_c, out_n), V, F


def cull_mesh(mesh, projections, masks, radius=24, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """evaluate_single_scene.py:53-95 on a device mesh: dilate the masks by `radius` (or take an already dilated MaskBits), keep the vertices cull_vertices
    keeps, keep the faces whose three vertices are kept, and move the result by the scene's scale_mat.

    The output holds exactly the kept vertices in index order -- a kept vertex that no surviving face refers to stays, as with trimesh's update_vertices --
    at v * scale + offset in f32 (a multiply, then an add; `scale` = scale_mat[0, 0], `offset` = scale_mat[:3, 3]), colours and normals copied bit for bit;
    face order is kept and the indices are re-mapped.  -> a new tsdf.TriangleMesh on the device; the input is left untouched.

    A face with an index outside [0, V) is never dereferenced and raises DTUError before any output is allocated.
    Host read-backs: the state words after the count pass (V', F': they size the outputs) and once more after the emit."""
    named, rest = _check_cull(mesh, projections, masks, radius, scale, offset)
    return _cull_mesh(_device.check_cuda("dtu", *named), rest)[0]


# ---- the point filters ---------------------------------------------------------------------------------------------------------------------------------
def _check_box(obs_mask, bb, res, patch):
    """-> (lo, hi: f32 (3,); bb0: f64 (3,); res, patch)."""
    if not torch.is_tensor(obs_mask):
        raise TypeError("obs_mask must be a tensor, got %s" % type(obs_mask).__name__)
    if obs_mask.dtype not in (torch.uint8, torch.bool) or obs_mask.dim() != 3 or min(obs_mask.shape) < 1:
        raise ValueError("obs_mask must be (X, Y, Z) uint8 or bool with no empty axis, got %s %s" % (tuple(obs_mask.shape), obs_mask.dtype))
    if max(obs_mask.shape) >= 1 << 31 or obs_mask.numel() >= 1 << 40:
        raise ValueError("obs_mask too large: %s" % (tuple(obs_mask.shape),))
    if torch.is_tensor(bb):
        bb = bb.detach().cpu().numpy()
    try:
        bb = np.asarray(bb, np.float64)
    except (TypeError, ValueError):
        raise TypeError("bb must be a (2, 3) array, got %s" % type(bb).__name__) from None
    if bb.shape != (2, 3) or not np.all(np.isfinite(bb)):
        raise ValueError("bb must be (2, 3) and finite, got %s" % (bb.shape,))
    res = _device.check_positive("res", res)
    patch = _device.check_positive("patch", patch, allow_zero=True)
    bb32 = bb.astype(np.float32)
    lo = bb32[0] - np.float32(patch)
    hi = bb32[1] + np.float32(patch * 2)
    return lo, hi, bb32[0].astype(np.float64), res, patch


def _obs_filter_async(points, obs_mask, box, state):
    lo, hi, bb0, res, _ = box
    N, dev = int(points.shape[0]), points.device
    X, Y, Z = (int(x) for x in obs_mask.shape)
    with torch.cuda.device(dev):
        inbound = torch.zeros(N, dtype=torch.uint8, device=dev)
        in_obs = torch.zeros(N, dtype=torch.uint8, device=dev)
    _device.call(dev, "ibgs_dtu_obs_filter", N, points.data_ptr(), obs_mask.view(torch.uint8).data_ptr(), X, Y, Z, (ctypes.c_float * 3)(*lo.tolist()),
                 (ctypes.c_float * 3)(*hi.tolist()), (ctypes.c_double * 3)(*bb0.tolist()), res, inbound.data_ptr(), in_obs.data_ptr(), state.data_ptr())
    return ObsFilter(inbound.view(torch.bool), in_obs.view(torch.bool))


def obs_mask_filter(points, obs_mask, bb, res, patch=60.0):
    """eval.py:98-110: the bounding box with its patch margin, then the look-up in the ObsMask voxel grid.  points (N, 3) f32; obs_mask (X, Y, Z) uint8 (or
    bool) on the device; bb (2, 3); res, patch floats.  The bounds are formed on the host in f32, lo = f32(bb[0]) - f32(patch), hi = f32(bb[1]) + f32(2 patch);
    the kernel works in f64 on the f32 points: inbound = all_k (lo_k <= p_k < hi_k); g_k = rint((p_k - f32(bb[0][k])) / res), ties to even;
    in_obs = inbound and all_k (0 <= g_k < shape_k) and obs_mask[g_0, g_1, g_2] != 0.  -> ObsFilter(inbound, in_obs), (N,) bool each, on the device.
    One host read-back, at the end: the state words (a non-finite coordinate raises ValueError)."""
    points = _device.check_points("points", points)
    box = _check_box(obs_mask, bb, res, patch)
    points, obs_mask = _device.check_cuda("dtu", ("points", points), ("obs_mask", obs_mask))
    state = _new_state(points.device)
    out = _obs_filter_async(points, obs_mask, box, state)
    _raise_on(state.cpu().tolist(), "obs_mask_filter")          # (waits for the stream)
    return out


def _check_plane(plane):
    if torch.is_tensor(plane):
        plane = plane.detach().cpu().numpy()
    try:
        p = np.asarray(plane, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError("plane must hold 4 numbers, got %s" % type(plane).__name__) from None
    if p.shape[0] != 4 or not np.all(np.isfinite(p)):
        raise ValueError("plane must hold 4 finite numbers, got %r" % (plane,))
    return p


def _above_plane_async(points, plane, state):
    N, dev = int(points.shape[0]), points.device
    with torch.cuda.device(dev):
        out = torch.zeros(N, dtype=torch.uint8, device=dev)
    _device.call(dev, "ibgs_dtu_above_plane", N, points.data_ptr(), (ctypes.c_double * 4)(*plane.tolist()), out.data_ptr(), state.data_ptr())
    return out.view(torch.bool)


def above_plane(points, plane):
    """eval.py:126-129: ((P_0 x + P_1 y) + P_2 z) + P_3 > 0 in f64 from the f32 points and the 4 numbers of `plane` (a point on the plane is not above it).
    -> (N,) bool on the device.  One host read-back, at the end: the state words (a non-finite coordinate raises ValueError)."""
    points = _device.check_points("points", points)
    plane = _check_plane(plane)
    points, = _device.check_cuda("dtu", ("points", points))
    state = _new_state(points.device)
    out = _above_plane_async(points, plane, state)
    _raise_on(state.cpu().tolist(), "above_plane")          # (waits for the stream)
    return out


# ---- the DTU chain -------------------------------------------------------------------------------------------------------------------------------------
def evaluate_dtu(mesh, gt_points, obs_mask, bb, res, plane, density=0.2, max_dist=20.0, patch=60.0, seed=0, cull: Optional[Cull] = None):
    """eval.py:43-157 on a device mesh.  With `cull` (a Cull, or a (projections, masks, radius, scale, offset) tuple) the mesh first goes through cull_mesh.
    Then: sample the surface at `density`; visit the points in the order of a torch.randperm seeded with `seed` and thin them to a spacing of `density`;
    obs_mask_filter on the thinned cloud; data_in = the in-bound points; Chamfer distance with the cut-off max_dist between data_in and gt_points, the
    pred -> gt queries being the points inside the observation mask, the gt -> pred queries the gt points above_plane, searched among data_in (eval.py:132),
    not among the whole thinned cloud.

    -> dict: mean_d2s, mean_s2d, overall, n_d2s, n_s2d, n_sampled, n_thinned, n_inbound, n_in_obs, n_above, and after a cull n_vertices_culled, n_faces_culled
    (how many the cull removed).  Host read-backs: those of cull_mesh, sample_surface, downsample and chamfer, one for the filters' state words and one per
    boolean selection (torch sizes it)."""
    gt_points = _device.check_points("gt_points", gt_points)
    box = _check_box(obs_mask, bb, res, patch)
    plane = _check_plane(plane)
    density = _device.check_positive("density", density)
    max_dist = _device.check_positive("max_dist", max_dist, allow_zero=True)
    v, f = mesh_eval._check_mesh(mesh)
    named = (("mesh.vertices", v), ("mesh.faces", f))
    if cull is not None:
        try:
            cull = Cull(*cull)
        except TypeError:
            raise TypeError("cull must be a Cull or a (projections, masks, radius, scale, offset) tuple, got %s" % type(cull).__name__) from None
        named, rest = _check_cull(mesh, cull.projections, cull.masks, cull.radius, cull.scale, cull.offset)
    checked = _device.check_cuda("dtu", ("gt_points", gt_points), ("obs_mask", obs_mask), *named)
    out = {}
    if cull is not None:
        mesh, V, F = _cull_mesh(checked[2:], rest)
        out.update(n_vertices_culled=V - int(mesh.vertices.shape[0]), n_faces_culled=F - int(mesh.faces.shape[0]))
    gt_points, obs_mask = checked[:2]
    cloud = mesh_eval.sample_surface(mesh, density)
    dev = cloud.device
    with torch.cuda.device(dev):
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed))
        order = torch.randperm(cloud.shape[0], generator=g, device=dev)
        thinned = cloud[mesh_eval.downsample(cloud, density, order=order)]
    state = _new_state(dev)
    filt = _obs_filter_async(thinned, obs_mask, box, state)
    above = _above_plane_async(gt_points, plane, state)
    with torch.cuda.device(dev):
        counts = torch.stack([filt.inbound.sum(), filt.in_obs.sum(), above.sum()]).to(torch.int32)
        back = torch.cat([state, counts]).cpu().tolist()          # (waits for the stream)
    _raise_on(back[:_lib.DTU_STATE_WORDS], "evaluate_dtu")
    with torch.cuda.device(dev):
        data_in = thinned[filt.inbound]
        query = filt.in_obs[filt.inbound]
    c = mesh_eval.chamfer(data_in, gt_points, max_dist, pred_query_mask=query, gt_query_mask=above)
    out.update({"mean_d2s": c.mean_d2s, "mean_s2d": c.mean_s2d, "overall": c.overall, "n_d2s": c.n_d2s, "n_s2d": c.n_s2d, "n_sampled": int(cloud.shape[0]),
                "n_thinned": int(thinned.shape[0]), "n_inbound": back[-3], "n_in_obs": back[-2], "n_above": back[-1]})
    return out


def read_obs_mask(obs_mat_path, plane_mat_path):
    """The two MATLAB files of a DTU scan (eval.py:96-97, 125): ObsMask{scan}_10.mat holds ObsMask, BB and Res, Plane{scan}.mat holds P.
    -> (obs_mask (X, Y, Z) uint8 numpy, bb (2, 3) f32 numpy, res float, plane (4,) f64 numpy), on the host: move obs_mask to the device for the calls above.
    Needs scipy (imported here, not with the module)."""
    try:
        from scipy.io import loadmat
    except ImportError:
        raise ImportError("read_obs_mask needs scipy (scipy.io.loadmat) to read .mat files; the device code does not") from None
    m = loadmat(obs_mat_path)
    for key in ("ObsMask", "BB", "Res"):
        if key not in m:
            raise ValueError("%s holds no %s" % (obs_mat_path, key))
    p = loadmat(plane_mat_path)
    if "P" not in p:
        raise ValueError("%s holds no P" % plane_mat_path)
    obs = np.ascontiguousarray(np.asarray(m["ObsMask"]) != 0).astype(np.uint8)
    bb = np.asarray(m["BB"], np.float32).reshape(2, 3)
    res = float(np.asarray(m["Res"]).reshape(-1)[0])
    plane = np.asarray(p["P"], np.float64).reshape(-1)
    if obs.ndim != 3 or plane.shape[0] != 4:
        raise ValueError("ObsMask must be 3-D and P hold 4 numbers, got %s and %s" % (obs.shape, plane.shape))
    return obs, bb, res, plane
