"""Point-cloud registration on the MI355X: what the reference's Tanks-and-Temples script does between a reconstruction and its F-score
(scripts/tnt_eval/run.py:94-128, registration.py:106-195, evaluation.py:74-91), which runs on the host through Open3D: transform, crop to the scene's
selection volume, voxel_down_sample, three rounds of ICP with scale, and the two distance sweeps.  With mesh_eval:

    vol = registration.read_crop_volume("Barn.json")
    scores = registration.evaluate_tnt(mesh.vertices, gt_points, init_trans, vol, tau=0.01)          # {"precision", "recall", "fscore", "transformation", ...}

The contract is this project's own statement of those stages ("Registration"; header of ibgs_amd/csrc/registration.hip);
tests/registration_ref.py restates it.  Every result is a pure function of the inputs: the sums are made in a fixed order without float atomics, so a
transformation is bit-identical from run to run.

HIP only (C ABI include/ibgs_registration.h): CPU tensors are refused, every argument is checked before any GPU work, every kernel runs on torch's current
stream, inputs are never written.  The orderings (voxel keys; Morton keys for ICP's search hierarchy, ibgs_amd/mesh_eval.py) are torch.sort calls; everything
else is the library's kernels.  The similarity fit itself (a 3 x 3 SVD) is numpy on the host.  Each call reads a few words back (it waits for the stream):
the docstrings say which."""
import ctypes
import json
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _device, _lib, mesh_eval

_AXES = {"X": 0, "Y": 1, "Z": 2}


class CropVolume(NamedTuple):
    """Open3D's SelectionPolygonVolume, the content of a TnT crop file."""
    axis: str                    # orthogonal_axis: "X", "Y" or "Z"
    axis_min: float
    axis_max: float
    polygon: np.ndarray          # bounding_polygon: (n, 3) f64, 3 <= n <= 1024; the coordinate along `axis` is not used


class ICPResult(NamedTuple):
    transformation: np.ndarray   # 4 x 4 f64: source -> target
    fitness: float               # correspondences / source points, at `transformation`
    inlier_rmse: float           # sqrt(sum d^2 / correspondences), at `transformation`
    iterations: int              # updates of the transformation
    n_correspondences: int


class RegistrationError(RuntimeError):
    pass


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------------
def _check_T(name, T):
    try:
        T = np.array(T, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("%s must be a 4 x 4 matrix, got %s" % (name, type(T).__name__)) from None
    if T.shape != (4, 4):
        raise ValueError("%s must be 4 x 4, got %s" % (name, T.shape))
    if not np.all(np.isfinite(T)):
        raise ValueError("%s holds a non-finite entry" % name)
    if T[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise ValueError("the last row of %s must be 0 0 0 1, got %s" % (name, T[3].tolist()))
    return np.ascontiguousarray(T)


def _check_volume(vol):
    """-> (w, axis_min, axis_max, (n, 2) f64 {u, v})."""
    try:
        axis, lo, hi, poly = vol.axis, vol.axis_min, vol.axis_max, vol.polygon
    except AttributeError:
        raise TypeError("volume must be a CropVolume, got %s" % type(vol).__name__) from None
    if axis not in _AXES:
        raise ValueError("volume.axis must be 'X', 'Y' or 'Z', got %r" % (axis,))
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("volume.axis_min / axis_max must be finite with axis_min <= axis_max, got %r, %r" % (lo, hi))
    poly = np.asarray(poly, np.float64)
    if poly.ndim != 2 or poly.shape[1] != 3:
        raise ValueError("volume.polygon must be (n, 3), got %s" % (poly.shape,))
    if not 3 <= poly.shape[0] <= _lib.PCREG_MAX_POLYGON:
        raise ValueError("volume.polygon has %d vertices (3 .. %d)" % (poly.shape[0], _lib.PCREG_MAX_POLYGON))
    w = _AXES[axis]
    uv = np.ascontiguousarray(poly[:, [k for k in range(3) if k != w]])
    if not np.all(np.isfinite(uv)):
        raise ValueError("volume.polygon holds a non-finite coordinate")
    return w, lo, hi, uv


def read_crop_volume(path):
    """A TnT crop file (Open3D's read_selection_polygon_volume): JSON with orthogonal_axis, axis_min, axis_max, bounding_polygon.  -> CropVolume."""
    with open(path) as f:
        d = json.load(f)
    vol = CropVolume(str(d["orthogonal_axis"]).upper(), float(d["axis_min"]), float(d["axis_max"]), np.asarray(d["bounding_polygon"], np.float64).reshape(-1, 3))
    _check_volume(vol)
    return vol


def _c16(T):
    return (ctypes.c_double * 16)(*T.reshape(-1).tolist())


def _new_state(dev):
    return _device.zeros_state(dev, _lib.PCREG_STATE_WORDS)


def _scratch(dev, n):
    nbytes = _lib.load().ibgs_pcreg_required_scratch(n)
    if nbytes == 0:
        raise ValueError("cloud too large: N %d" % n)
    return _device.scratch(dev, nbytes), nbytes


def _raise_on(s, what, voxel=None):
    """s: the state words on the host."""
    if s[_lib.PCREG_BAD_POINTS]:
        raise ValueError("%s: %d point(s) with a non-finite coordinate" % (what, s[_lib.PCREG_BAD_POINTS]))
    if s[_lib.PCREG_KEY_OVERFLOW]:
        raise ValueError("%s: the voxel size %g is too small for the cloud's extent: %d point(s) lie beyond voxel %d along an axis"
                         % (what, voxel, s[_lib.PCREG_KEY_OVERFLOW], _lib.PCREG_MAX_INDEX))
    if s[_lib.PCREG_BAD_INDEX] or s[_lib.PCREG_OVERRUN]:
        raise RegistrationError("%s: library fault: %d index(es) / %d write(s) out of range" % (what, s[_lib.PCREG_BAD_INDEX], s[_lib.PCREG_OVERRUN]))


# ---- transform and crop --------------------------------------------------------------------------------------------------------------------------------
def _transform_into(points, T, out, state):
    _device.call(points.device, "ibgs_pcreg_transform", int(points.shape[0]), points.data_ptr(), _c16(T), out.data_ptr(), state.data_ptr())


def transform(points, T):
    """T (4 x 4 f64 on the host, last row 0 0 0 1) applied to every point: x' = ((T00 x + T01 y) + T02 z) + T03 in f64 from the f32 coordinates, rounded once to
    f32.  -> (N, 3) f32 on the device.  One host read-back, at the end: the state words (a non-finite coordinate raises ValueError)."""
    points = _device.check_points("points", points)
    T = _check_T("T", T)
    points, = _device.check_cuda("registration", ("points", points))
    dev = points.device
    with torch.cuda.device(dev):
        out = torch.empty_like(points)
        state = _new_state(dev)
    _transform_into(points, T, out, state)
    _raise_on(state.cpu().tolist(), "transform")          # (waits for the stream)
    return out


def _crop_async(points, vol, T, state):
    w, lo, hi, uv = vol
    dev = points.device
    with torch.cuda.device(dev):
        mask = torch.zeros(int(points.shape[0]), dtype=torch.uint8, device=dev)
        poly = torch.from_numpy(uv).to(dev)
    _device.call(dev, "ibgs_pcreg_crop", int(points.shape[0]), points.data_ptr(), _c16(T) if T is not None else None, w, lo, hi, int(uv.shape[0]), poly.data_ptr(),
                 mask.data_ptr(), state.data_ptr())
    return mask.view(torch.bool)


def crop(points, volume, T=None):
    """SelectionPolygonVolume.crop_point_cloud as a mask: a point is kept iff axis_min <= p[w] <= axis_max and an odd number of polygon edges cross its
    v-coordinate to the left of it (the half-open rule of the header of registration.hip), all in f64.  With T the point is transformed first exactly as
    transform() does: crop(points, vol, T) equals crop(transform(points, T), vol) bit for bit.  -> (N,) bool on the device.
    One host read-back, at the end: the state words."""
    points = _device.check_points("points", points)
    vol = _check_volume(volume)
    if T is not None:
        T = _check_T("T", T)
    points, = _device.check_cuda("registration", ("points", points))
    state = _new_state(points.device)
    mask = _crop_async(points, vol, T, state)
    _raise_on(state.cpu().tolist(), "crop")          # (waits for the stream)
    return mask


# ---- voxel thinning ------------------------------------------------------------------------------------------------------------------------------------
def voxel_down_sample(points, voxel_size, return_keys=False):
    """Open3D's voxel_down_sample: one point per occupied voxel of the grid whose origin is the cloud's per-axis minimum minus half a voxel, the mean of the
    voxel's points (f64 sum, one division, one rounding to f32).  The rows come IN ASCENDING KEY ORDER, key = ix << 42 | iy << 21 | iz (Open3D's order is
    that of a hash map).  -> (M, 3) f32 on the device; with return_keys also the (M,) int64 keys.

    A voxel index above 2^21 - 1 raises ValueError (the voxel size is too small for the cloud's extent).  One host read-back sizes the output: M and the
    state words."""
    points = _device.check_points("points", points)
    voxel_size = _device.check_positive("voxel_size", voxel_size)
    points, = _device.check_cuda("registration", ("points", points))
    N, dev = int(points.shape[0]), points.device
    if N == 0:
        with torch.cuda.device(dev):
            out = torch.empty(0, 3, dtype=torch.float32, device=dev)
            return (out, torch.empty(0, dtype=torch.int64, device=dev)) if return_keys else out
    scratch, nbytes = _scratch(dev, N)
    with torch.cuda.device(dev):
        state = _new_state(dev)
        bounds = torch.empty(6, dtype=torch.float32, device=dev)
        keys = torch.empty(N, dtype=torch.int64, device=dev)
        total = torch.zeros(1, dtype=torch.int32, device=dev)
    _device.call(dev, "ibgs_pcreg_bounds", N, points.data_ptr(), scratch.data_ptr(), nbytes, bounds.data_ptr(), state.data_ptr())
    _device.call(dev, "ibgs_pcreg_voxel_keys", N, points.data_ptr(), bounds.data_ptr(), voxel_size, keys.data_ptr(), state.data_ptr())
    with torch.cuda.device(dev):
        skeys, order = torch.sort(keys, stable=True)          # equal keys stay in index order: a voxel's sum is made in that order
    _device.call(dev, "ibgs_pcreg_voxel_count", N, skeys.data_ptr(), scratch.data_ptr(), nbytes, total.data_ptr(), state.data_ptr())
    back = torch.cat([total, state]).cpu().tolist()          # (waits for the stream)
    _raise_on(back[1:], "voxel_down_sample", voxel_size)
    M = back[0]
    with torch.cuda.device(dev):
        out = torch.empty(M, 3, dtype=torch.float32, device=dev)
        okeys = torch.empty(M, dtype=torch.int64, device=dev) if return_keys else None
    _device.call(dev, "ibgs_pcreg_voxel_emit", N, points.data_ptr(), order.data_ptr(), skeys.data_ptr(), scratch.data_ptr(), nbytes, M, out.data_ptr(),
                 okeys.data_ptr() if return_keys else None, state.data_ptr())
    return (out, okeys) if return_keys else out


# ---- the similarity fit --------------------------------------------------------------------------------------------------------------------------------
def umeyama(moments, pivot=(0.0, 0.0, 0.0), what="umeyama"):
    """Eigen's umeyama(src, dst, with_scaling = true) from the 18 moments of ibgs_pcreg_moments about `pivot`: n, sum(s - c), sum(t - c),
    sum (s - c)(t - c)^T, sum |s - c|^2, sum d^2.  Sigma = (1 / n) sum (t - m_t)(s - m_s)^T = U D V^T, S = diag(1, 1, det U det V < 0 ? -1 : 1), R = U S V^T,
    scale = tr(D S) / var_s, translation = m_t - scale R m_s.  numpy f64 on the host.  -> 4 x 4 f64."""
    m = np.asarray(moments, np.float64).reshape(-1)
    if m.shape[0] != _lib.PCREG_MOMENTS:
        raise ValueError("moments must hold %d numbers, got %d" % (_lib.PCREG_MOMENTS, m.shape[0]))
    c = np.asarray(pivot, np.float64).reshape(3)
    n = m[0]
    if not n >= 3:
        raise RegistrationError("%s: %g correspondence(s), at least 3 are needed" % (what, n))
    ms, mt = m[1:4] / n, m[4:7] / n          # (about the pivot)
    sigma = m[7:16].reshape(3, 3).T / n - np.outer(mt, ms)
    var_s = m[16] / n - float(ms @ ms)
    if not var_s > 0:
        raise RegistrationError("%s: the source correspondences have no extent (variance %g)" % (what, var_s))
    U, D, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = (U * S) @ Vt
    scale = float((D * S).sum()) / var_s
    T = np.identity(4)
    T[:3, :3] = scale * R
    T[:3, 3] = (c + mt) - scale * (R @ (c + ms))
    return T


def umeyama_points(src, dst):
    """The closed form for matched points (camera centres, say): the similarity that maps src (n, 3) onto dst (n, 3) in the least-squares sense.  Host, numpy."""
    s, t = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if s.ndim != 2 or s.shape[1] != 3 or s.shape != t.shape:
        raise ValueError("src and dst must both be (n, 3), got %s and %s" % (s.shape, t.shape))
    if not (np.all(np.isfinite(s)) and np.all(np.isfinite(t))):
        raise ValueError("src / dst hold a non-finite coordinate")
    c = (t.min(0) + t.max(0)) / 2 if len(t) else np.zeros(3)
    sc, tc = s - c, t - c
    m = np.concatenate([[float(len(s))], sc.sum(0), tc.sum(0), (sc[:, :, None] * tc[:, None, :]).sum(0).reshape(-1), [(sc * sc).sum()], [((s - t) ** 2).sum()]])
    return umeyama(m, c, "umeyama_points")


# ---- ICP -----------------------------------------------------------------------------------------------------------------------------------------------
def _icp_step(source, index, T, max_dist, qorder, q, out, pivot, scratch, mstate, pstate):
    """One evaluation at T, nothing read back: q = T source, its nearest targets within max_dist, the 18 moments into `out`."""
    dev, Q = source.device, int(source.shape[0])
    _transform_into(source, T, q, pstate)
    with torch.cuda.device(dev):
        dist = torch.empty(Q, dtype=torch.float32, device=dev)
        idx = torch.empty(Q, dtype=torch.int32, device=dev)
    _device.call(dev, "ibgs_meval_nearest", Q, q.data_ptr(), qorder.data_ptr() if qorder is not None else None, index.N, index.tree.data_ptr(), index.nbytes,
                 max_dist, dist.data_ptr(), idx.data_ptr(), mstate.data_ptr())
    _device.call(dev, "ibgs_pcreg_moments", Q, q.data_ptr(), idx.data_ptr(), index.N, index.points.data_ptr(), (ctypes.c_double * 3)(*pivot.tolist()), scratch[0].data_ptr(),
                 scratch[1], out.data_ptr(), pstate.data_ptr())
    return idx


def _read_step(out, mstate, pstate, what):
    """The one read-back of an ICP iteration: the 18 doubles and both units' state words.  -> the moments (numpy f64)."""
    with torch.cuda.device(out.device):
        back = torch.cat([out.view(torch.int64), mstate.to(torch.int64), pstate.to(torch.int64)]).cpu()          # (waits for the stream)
    mesh_eval.raise_on(back[_lib.PCREG_MOMENTS:_lib.PCREG_MOMENTS + _lib.MEVAL_STATE_WORDS].tolist(), what)
    _raise_on(back[_lib.PCREG_MOMENTS + _lib.MEVAL_STATE_WORDS:].tolist(), what)
    return back[:_lib.PCREG_MOMENTS].view(torch.float64).numpy().copy()


def _target_index(target, mstate, what):
    """The hierarchy over the target and the pivot of the moments, the centre of its bounding box (one read-back: the bounds)."""
    index = mesh_eval.Index(target, mstate)
    b = index.bounds.cpu().numpy().astype(np.float64)          # (waits for the stream)
    if not np.all(np.isfinite(b)):
        raise ValueError("%s: target holds a non-finite coordinate" % what)
    return index, (b[:3] + b[3:]) / 2


def moments(source, target, max_dist, T=None):
    """One ICP evaluation: the 18 moments of the pairs (T source[i], its nearest target within max_dist) about the centre of the target's bounding box.
    -> (moments (18,) f64 numpy: n, sum(s - c), sum(t - c), sum (s - c)(t - c)^T row-major, sum |s - c|^2, sum d^2; pivot (3,) f64; index (Q,) int32 on the
    device, -1 where there is no pair).  Two host read-backs: the target's bounds, then the moments with the state words."""
    source, target = _device.check_points("source", source), _device.check_points("target", target)
    max_dist = _device.check_positive("max_dist", max_dist)
    T = _check_T("T", np.identity(4) if T is None else T)
    source, target = _device.check_cuda("registration", ("source", source), ("target", target))
    dev = source.device
    if source.shape[0] == 0 or target.shape[0] == 0:
        raise RegistrationError("moments: source %d, target %d points: both must hold points" % (source.shape[0], target.shape[0]))
    mstate, pstate = mesh_eval.new_state(dev), _new_state(dev)
    index, pivot = _target_index(target, mstate, "moments")
    with torch.cuda.device(dev):
        q = torch.empty_like(source)
        out = torch.zeros(_lib.PCREG_MOMENTS, dtype=torch.float64, device=dev)
    idx = _icp_step(source, index, T, max_dist, None, q, out, pivot, _scratch(dev, 0), mstate, pstate)
    return _read_step(out, mstate, pstate, "moments"), pivot, idx


def icp(source, target, max_dist, init=None, max_iter=20, rel_fitness=1e-6, rel_rmse=1e-6):
    """Point-to-point ICP with scale (Open3D's registration_icp with TransformationEstimationPointToPoint(True) and ICPConvergenceCriteria(rel_fitness,
    rel_rmse, max_iter)): iteration k transforms the ORIGINAL source by the accumulated f64 T_k (Open3D re-transforms the moved cloud), finds every point's
    nearest target within max_dist, sums the 18 moments of the pairs about the centre of the target's bounding box, and reads them back; fitness = n / N,
    rmse = sqrt(sum d^2 / n); it stops when both change by less than the tolerances or after max_iter updates, else T_{k+1} = umeyama(moments) T_k.
    -> ICPResult; fitness and inlier_rmse are those measured at the returned transformation.

    The hierarchy over `target` and the queries' walk order are built once.  Host read-backs: the target's bounds once, then the 18 doubles and the state
    words once per iteration.  Fewer than 3 correspondences raise RegistrationError with the iteration."""
    source, target = _device.check_points("source", source), _device.check_points("target", target)
    max_dist = _device.check_positive("max_dist", max_dist)
    T = _check_T("init", np.identity(4) if init is None else init)
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError("max_iter must be >= 0, got %d" % max_iter)
    rel_fitness, rel_rmse = _device.check_positive("rel_fitness", rel_fitness, allow_zero=True), _device.check_positive("rel_rmse", rel_rmse, allow_zero=True)
    source, target = _device.check_cuda("registration", ("source", source), ("target", target))
    dev, Q = source.device, int(source.shape[0])
    if Q == 0 or target.shape[0] == 0:
        raise RegistrationError("icp: iteration 0: 0 correspondence(s) (source %d, target %d points), at least 3 are needed" % (Q, target.shape[0]))
    mstate, pstate = mesh_eval.new_state(dev), _new_state(dev)
    index, pivot = _target_index(target, mstate, "icp")
    scratch = _scratch(dev, 0)
    with torch.cuda.device(dev):
        q = torch.empty_like(source)
        out = torch.zeros(_lib.PCREG_MOMENTS, dtype=torch.float64, device=dev)
    _transform_into(source, T, q, pstate)
    with torch.cuda.device(dev):
        qorder = torch.sort(index.keys(q)).indices          # neighbouring lanes walk neighbouring boxes; only a locality hint, so it is kept for every iteration
    prev = None
    k = 0
    while True:
        _icp_step(source, index, T, max_dist, qorder, q, out, pivot, scratch, mstate, pstate)
        m = _read_step(out, mstate, pstate, "icp")
        n = int(m[0])
        if n < 3:
            raise RegistrationError("icp: iteration %d: %d correspondence(s) within max_dist %g, at least 3 are needed" % (k, n, max_dist))
        fitness, rmse = n / Q, math.sqrt(m[17] / n)
        if (prev is not None and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse) or k == max_iter:
            return ICPResult(T, fitness, rmse, k, n)
        prev = (fitness, rmse)
        T = umeyama(m, pivot, "icp: iteration %d" % k) @ T
        k += 1


# ---- the TnT chain -------------------------------------------------------------------------------------------------------------------------------------
def _uniform(cloud, max_points):
    """registration.py:119-124: every round(n / max_points)-th point, only when the cloud holds more than max_points."""
    n = int(cloud.shape[0])
    if n > max_points:
        return cloud[::int(round(n / float(max_points)))].contiguous()
    return cloud


def evaluate_tnt(pred_points, gt_points, init_trans, volume, tau, voxel_rounds=((1, 80), (0.5, 20)), uniform_round=2, max_iter=20, max_points=4_000_000):
    """run.py:103-128 without the plots.  For each (a, b) of voxel_rounds: s = voxel_down_sample of the transformed pred points inside the volume at a tau,
    t = the same of the gt points inside the volume, T = icp(s, t, b tau).transformation T.  Then one round on the cropped clouds, each thinned by
    [::round(n / max_points)] only when it holds more than max_points, at the threshold uniform_round tau (None: no such round).  Then both cropped clouds
    thinned with voxel_down_sample(tau / 2) go to mesh_eval.fscore(s, t, tau).  Normals, histograms and plots are left out: they feed nothing into the score.

    -> dict: precision, recall, fscore, n_precision, n_pred, n_recall, n_gt, n_pred_cropped, n_gt_cropped, transformation (4 x 4 f64), rounds (ICPResults).
    Host read-backs: those of crop, voxel_down_sample, icp and fscore, and one per boolean selection (torch sizes it)."""
    pred_points, gt_points = _device.check_points("pred_points", pred_points), _device.check_points("gt_points", gt_points)
    T = _check_T("init_trans", init_trans)
    _check_volume(volume)
    tau = _device.check_positive("tau", tau)
    rounds = []
    for r in voxel_rounds:
        a, b = r
        rounds.append((_device.check_positive("voxel_rounds voxel factor", a), _device.check_positive("voxel_rounds threshold factor", b)))
    if uniform_round is not None:
        uniform_round = _device.check_positive("uniform_round", uniform_round)
    max_points = int(max_points)
    if max_points < 1:
        raise ValueError("max_points must be >= 1, got %d" % max_points)
    pred_points, gt_points = _device.check_cuda("registration", ("pred_points", pred_points), ("gt_points", gt_points))
    dev = pred_points.device
    eye = np.identity(4)

    def moved_pred(T):
        with torch.cuda.device(dev):
            inside = pred_points[crop(pred_points, volume, T)]
        return transform(inside, T)

    with torch.cuda.device(dev):
        gt_crop = gt_points[crop(gt_points, volume)]
    results = []
    for a, b in rounds:
        r = icp(voxel_down_sample(moved_pred(T), a * tau), voxel_down_sample(gt_crop, a * tau), b * tau, eye, max_iter=max_iter)
        T = r.transformation @ T
        results.append(r)
    if uniform_round is not None:
        r = icp(_uniform(moved_pred(T), max_points), _uniform(gt_crop, max_points), uniform_round * tau, eye, max_iter=max_iter)
        T = r.transformation @ T
        results.append(r)
    s_crop = moved_pred(T)
    s, t = voxel_down_sample(s_crop, tau / 2), voxel_down_sample(gt_crop, tau / 2)
    f = mesh_eval.fscore(s, t, tau)
    return {"precision": f.precision, "recall": f.recall, "fscore": f.fscore, "n_precision": f.n_precision, "n_pred": f.n_pred, "n_recall": f.n_recall,
            "n_gt": f.n_gt, "n_pred_cropped": int(s_crop.shape[0]), "n_gt_cropped": int(gt_crop.shape[0]), "transformation": T, "rounds": results}
