"""Mesh evaluation on the MI355X: the number `tsdf_fusion_post.ply` is made for.  The stages of the reference's scripts/eval_dtu/eval.py -- sample the
mesh's surface, thin the cloud to a minimum spacing, nearest distances in both directions -- and the precision / recall / F-score of
scripts/tnt_eval/evaluation.py:176-180, which run on the host through Open3D, a multiprocessing pool and sklearn's kd-tree.  With tsdf and mesh:

    post = mesh.post_process_mesh(volume.extract_mesh(), num_cluster)
    scores = mesh_eval.evaluate_mesh(post, gt_points, density=0.2, max_dist=20.0)          # {"mean_d2s", "mean_s2d", "overall", ...}

The contract is this project's own statement of those stages ("Mesh evaluation"; header of ibgs_amd/csrc/mesh_eval.hip);
tests/mesh_eval_ref.py restates it.  Sample positions, the thinning mask, nearest distances and indices are a pure function of the inputs (bit-identical
from run to run); the f64 means are summed with atomics and may differ in their last bits.

HIP only (C ABI include/ibgs_mesh_eval.h): CPU tensors are refused, every argument is checked before any GPU work, every kernel runs on torch's current
stream, inputs are never written.  The two orderings (Morton keys of the points, for the search hierarchy) are torch.sort calls; everything else is the
library's kernels.  Each call reads a few words back (it waits for the stream): the docstrings say which."""
from typing import NamedTuple

import torch

from . import _device, _lib
from ._device import MAX_POINTS

MAX_FACES = (1 << 30) - 1
THIN_FIRST_BATCH = 8          # rounds issued before the first read-back of the undecided count; every further batch is twice as long, up to
THIN_MAX_BATCH = 1024


class NearestResult(NamedTuple):
    dist: torch.Tensor          # (Q,) f32: distance to the nearest target, +inf when none is nearer than max_dist
    index: torch.Tensor         # (Q,) int32: its index (the smallest among equals), -1 when none


class ChamferResult(NamedTuple):
    mean_d2s: float             # mean of the pred -> gt distances below max_dist (NaN when there is none)
    mean_s2d: float             # mean of the gt -> pred distances below max_dist
    overall: float              # their mean
    n_d2s: int                  # how many distances each mean is over
    n_s2d: int
    n_pred_queries: int
    n_gt_queries: int


class FScoreResult(NamedTuple):
    precision: float            # share of the pred points nearer than tau to gt
    recall: float               # share of the gt points nearer than tau to pred
    fscore: float
    n_precision: int
    n_pred: int
    n_recall: int
    n_gt: int


class MeshEvalError(RuntimeError):
    pass


def _check_mask(name, m, n):
    if m is None:
        return None
    if not torch.is_tensor(m):
        raise TypeError("%s must be a tensor, got %s" % (name, type(m).__name__))
    if m.dtype != torch.bool or m.dim() != 1 or m.shape[0] != n:
        raise ValueError("%s must be (%d,) bool, got %s %s" % (name, n, tuple(m.shape), m.dtype))
    return m


def new_state(dev):
    return _device.zeros_state(dev, _lib.MEVAL_STATE_WORDS)


def raise_on(s, what):
    """s: the state words on the host."""
    if s[_lib.MEVAL_BAD_FACES]:
        raise MeshEvalError("%s: mesh.faces holds %d triangle(s) with a vertex index out of range" % (what, s[_lib.MEVAL_BAD_FACES]))
    if s[_lib.MEVAL_SAMPLE_OVERFLOW]:
        raise ValueError("%s: %d triangle(s) would be sampled more than %d times along a side: density is too small for this mesh"
                         % (what, s[_lib.MEVAL_SAMPLE_OVERFLOW], _lib.MEVAL_MAX_SIDE))
    if s[_lib.MEVAL_BAD_POINTS]:
        raise ValueError("%s: %d point(s) with a non-finite coordinate" % (what, s[_lib.MEVAL_BAD_POINTS]))
    if s[_lib.MEVAL_OVERRUN]:
        raise MeshEvalError("%s: library fault: %d write(s) out of range" % (what, s[_lib.MEVAL_OVERRUN]))


# ---- surface sampling --------------------------------------------------------------------------------------------------------------------------------
def _check_mesh(mesh):
    try:
        v, f = mesh.vertices, mesh.faces
    except AttributeError:
        raise TypeError("mesh must have .vertices and .faces (a tsdf.TriangleMesh), got %s" % type(mesh).__name__) from None
    for name, t in (("vertices", v), ("faces", f)):
        if not torch.is_tensor(t):
            raise TypeError("mesh.%s must be a tensor, got %s" % (name, type(t).__name__))
    if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
        raise ValueError("mesh.vertices must be (V, 3) float32, got %s %s" % (tuple(v.shape), v.dtype))
    if f.dtype != torch.int32 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("mesh.faces must be (F, 3) int32, got %s %s" % (tuple(f.shape), f.dtype))
    if v.shape[0] > MAX_POINTS or f.shape[0] > MAX_FACES:
        raise ValueError("mesh too large: V %d, F %d (limits: V < 2^31, F < 2^30)" % (v.shape[0], f.shape[0]))
    return v, f


def sample_surface(mesh, density, include_vertices=True, max_points=None):
    """The point cloud eval.py:54-71 draws from a mesh: for every triangle with a non-zero area, thr = density sqrt(|v1| |v2| / |v1 x v2|),
    n1 = floor(|v1| / thr), n2 = floor(|v2| / thr), and the points p0 + a v1 + b v2 with a = (i + 1/2) / n1, b = (j + 1/2) / n2, a + b < 1 (i-major,
    triangles in index order; none when n1 or n2 is 0), evaluated in f64 from the f32 vertices and rounded once.  -> (N, 3) f32 on the device: the
    vertices (if include_vertices) followed by the samples.

    One host read-back sizes the output: the 64-bit total and the state words.  `max_points` (default: what fits in 90 % of the device's free memory) is
    enforced on that total BEFORE anything is allocated: ValueError with the count.  A second read-back of the state follows the emit."""
    v, f = _check_mesh(mesh)
    density = _device.check_positive("density", density)
    if max_points is not None:
        max_points = int(max_points)
        if max_points < 0:
            raise ValueError("max_points must be >= 0, got %d" % max_points)
    v, f = _device.check_cuda("mesh_eval", ("mesh.vertices", v), ("mesh.faces", f))
    V, F, dev = int(v.shape[0]), int(f.shape[0]), v.device
    lib = _lib.load()
    nbytes = lib.ibgs_meval_required_sample_scratch(F)
    if nbytes == 0:
        raise ValueError("mesh too large: F %d" % F)
    scratch, state = _device.scratch(dev, nbytes), new_state(dev)
    with torch.cuda.device(dev):
        total = torch.zeros(1, dtype=torch.int64, device=dev)
    _device.call(dev, "ibgs_meval_sample_count", V, F, v.data_ptr(), f.data_ptr(), density, scratch.data_ptr(), nbytes, total.data_ptr(), state.data_ptr())
    back = torch.cat([total, state.to(torch.int64)]).cpu().tolist()          # (waits for the stream)
    raise_on(back[1:], "sample_surface")
    n_samples = back[0]
    n = n_samples + (V if include_vertices else 0)
    if max_points is not None and n > max_points:
        raise ValueError("sample_surface: %d points at density %g, max_points = %d" % (n, density, max_points))
    if max_points is None:
        free = torch.cuda.mem_get_info(dev)[0]
        if n * 12 > 0.9 * free:
            raise ValueError("sample_surface: %d points at density %g need %.1f GB, %.1f GB are free" % (n, density, n * 12 / 1e9, free / 1e9))
    if n > MAX_POINTS:
        raise ValueError("sample_surface: %d points at density %g (limit: N < 2^31)" % (n, density))
    with torch.cuda.device(dev):
        out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    first = 0
    if include_vertices:
        out[:V].copy_(v)
        first = V
    if n_samples:
        _device.call(dev, "ibgs_meval_sample_emit", V, F, v.data_ptr(), f.data_ptr(), density, scratch.data_ptr(), nbytes, n_samples,
                     out.data_ptr() + first * 12, state.data_ptr())
        raise_on(state.cpu().tolist(), "sample_surface")
    return out


# ---- the search hierarchy ----------------------------------------------------------------------------------------------------------------------------
class Index:
    """Hierarchy of boxes over a point set (N > 0), its scratch owned here; `points` stays referenced (registration's moments read the targets through it).
    `tag`: the int32 that travels with every point (default: its index)."""

    def __init__(self, points, state, tag=None):
        self.points, self.N, self.dev, self.state = points, int(points.shape[0]), points.device, state
        lib = _lib.load()
        self.nbytes = lib.ibgs_meval_required_tree(self.N)
        with torch.cuda.device(self.dev):
            self.bounds = torch.cat([points.amin(0), points.amax(0)])
            self.order = torch.sort(self.keys(points), stable=True).indices
        self.tree = _device.scratch(self.dev, self.nbytes)
        _device.call(self.dev, "ibgs_meval_build", self.N, points.data_ptr(), self.order.data_ptr(), tag.data_ptr() if tag is not None else None,
                     self.tree.data_ptr(), self.nbytes, state.data_ptr())

    def keys(self, points):
        with torch.cuda.device(self.dev):
            k = torch.empty(points.shape[0], dtype=torch.int64, device=self.dev)
        _device.call(self.dev, "ibgs_meval_keys", int(points.shape[0]), points.data_ptr(), self.bounds.data_ptr(), k.data_ptr(), self.state.data_ptr())
        return k

    def query(self, q, max_dist):
        """(dist, index) of every row of q; nothing is read back."""
        Q = int(q.shape[0])
        with torch.cuda.device(self.dev):
            dist = torch.empty(Q, dtype=torch.float32, device=self.dev)
            index = torch.empty(Q, dtype=torch.int32, device=self.dev)
            if Q == 0:
                return dist, index
            qorder = torch.sort(self.keys(q)).indices          # neighbouring lanes walk neighbouring boxes
        _device.call(self.dev, "ibgs_meval_nearest", Q, q.data_ptr(), qorder.data_ptr(), self.N, self.tree.data_ptr(), self.nbytes, max_dist, dist.data_ptr(),
                     index.data_ptr(), self.state.data_ptr())
        return dist, index


_Index = Index          # (the name tests/test_gpu_mesh_eval.py and tools/bench_tsdf.py know it by)


def _no_match(Q, dev):
    with torch.cuda.device(dev):
        return (torch.full((Q,), float("inf"), dtype=torch.float32, device=dev), torch.full((Q,), -1, dtype=torch.int32, device=dev))


def _nearest_async(query, target, max_dist, state):
    if target.shape[0] == 0:
        return _no_match(int(query.shape[0]), query.device)
    return Index(target, state).query(query, max_dist)


def nearest(query, target, max_dist):
    """Exact nearest neighbour of every query point among the target points, cut off at max_dist.  d2 = (dx dx + dy dy) + dz dz in f32; dist = the
    correctly rounded f32 square root of the smallest d2, index = the smallest target index attaining it; when that d2 is not below max_dist max_dist
    (formed in f32), or the target is empty, dist = +inf and index = -1.  -> NearestResult(dist (Q,) f32, index (Q,) int32) on the device.

    A query with nothing within max_dist costs a few dozen box tests, whatever max_dist is in units of the point spacing.
    One host read-back, at the end: the state words (a non-finite coordinate raises ValueError).  Nothing before it waits for the device."""
    query, target = _device.check_points("query", query), _device.check_points("target", target)
    max_dist = _device.check_positive("max_dist", max_dist, allow_zero=True)
    query, target = _device.check_cuda("mesh_eval", ("query", query), ("target", target))
    state = new_state(query.device)
    dist, index = _nearest_async(query, target, max_dist, state)
    raise_on(state.cpu().tolist(), "nearest")          # (waits for the stream)
    return NearestResult(dist, index)


# ---- thinning ----------------------------------------------------------------------------------------------------------------------------------------
def downsample(points, radius, order=None):
    """The thinning loop of eval.py:86-94: visiting the points in `order` (a permutation of their indices, (N,) int64; default: index order), a point is
    kept iff no point kept before it lies within `radius` (d2 <= radius radius, both in f32).  -> (N,) bool keep mask on the device, in index order.

    Computed in parallel rounds: an undecided point is removed once an earlier neighbour is kept, and kept once all its earlier neighbours are removed.
    Both decisions are final, so the mask does not depend on scheduling: it is the same bits on every run.  The rounds are issued in batches of
    THIN_FIRST_BATCH = 8, 16, 32, ... up to THIN_MAX_BATCH = 1024 rounds, with ONE read-back per batch (the undecided count and the state words).  A
    shuffled cloud needs about 10 rounds (one batch or two); the worst case is a chain of points visited along its length, each within `radius` of
    the one before, which needs on the order of one round per point: n points cost about log2(n / 8) + n / 1024 read-backs."""
    points = _device.check_points("points", points)
    radius = _device.check_positive("radius", radius, allow_zero=True)
    N = int(points.shape[0])
    if order is not None:
        if not torch.is_tensor(order):
            raise TypeError("order must be a tensor, got %s" % type(order).__name__)
        if order.dtype != torch.int64 or order.dim() != 1 or order.shape[0] != N:
            raise ValueError("order must be (%d,) int64, got %s %s" % (N, tuple(order.shape), order.dtype))
        points, order = _device.check_cuda("mesh_eval", ("points", points), ("order", order))
    else:
        points, = _device.check_cuda("mesh_eval", ("points", points))
    dev = points.device
    with torch.cuda.device(dev):
        keep = torch.zeros(N, dtype=torch.bool, device=dev)
        if N == 0:
            return keep
        state = new_state(dev)
        if order is None:
            rank = torch.arange(N, dtype=torch.int32, device=dev)
        else:          # rank[order[k]] = k; whether `order` is a permutation is settled by the counts read back with the first batch
            rank = torch.full((N,), -1, dtype=torch.int32, device=dev)
            rank[order.clamp(0, N - 1)] = torch.arange(N, dtype=torch.int32, device=dev)
            unranked = ((rank < 0).sum() + ((order < 0) | (order >= N)).sum()).to(torch.int32)          # (0 iff `order` is a permutation)
        index = Index(points, state, tag=rank)
        status = torch.zeros(N, dtype=torch.int32, device=dev)
    batch, first = THIN_FIRST_BATCH, True
    while True:
        _device.call(dev, "ibgs_meval_thin_rounds", N, index.tree.data_ptr(), index.nbytes, radius, status.data_ptr(), batch, state.data_ptr())
        if first and order is not None:
            s = torch.cat([state, unranked.reshape(1)]).cpu().tolist()          # (waits for the stream)
            if s[-1]:
                raise ValueError("order is not a permutation of 0 .. %d (%d point(s) are never visited)" % (N - 1, s[-1]))
        else:
            s = state.cpu().tolist()
        first = False
        raise_on(s, "downsample")
        if s[_lib.MEVAL_UNDECIDED] == 0:
            break
        batch = min(2 * batch, THIN_MAX_BATCH)
    with torch.cuda.device(dev):
        keep[index.order] = status == _lib.MEVAL_THIN_KEPT
    return keep


# ---- the metrics -------------------------------------------------------------------------------------------------------------------------------------
class _Sums:
    """f64 sums and counts of `dist < threshold`, several at once, read back together with the state words."""

    def __init__(self, dev, state, n):
        self.dev, self.state = dev, state
        with torch.cuda.device(dev):
            self.sum = torch.zeros(n, dtype=torch.float64, device=dev)
            self.count = torch.zeros(n, dtype=torch.int64, device=dev)

    def add(self, slot, dist, threshold):
        _device.call(self.dev, "ibgs_meval_reduce", int(dist.shape[0]), dist.data_ptr(), threshold, self.sum.data_ptr() + 8 * slot, self.count.data_ptr() + 8 * slot)

    def read(self, what):
        with torch.cuda.device(self.dev):
            back = torch.cat([self.sum.view(torch.int64), self.count, self.state.to(torch.int64)]).cpu()          # (waits for the stream)
        n = self.sum.shape[0]
        raise_on(back[2 * n:].tolist(), what)
        return back[:n].view(torch.float64).tolist(), back[n:2 * n].tolist()


def _mean(s, n):
    return s / n if n else float("nan")


def chamfer(pred, gt, max_dist, pred_query_mask=None, gt_query_mask=None):
    """DTU's Chamfer distance (eval.py:118-134, 157): mean_d2s = the mean of the distances from the pred points (those selected by pred_query_mask, a
    (N,) bool tensor) to their nearest gt point, mean_s2d = the mean of the distances from the gt points (those selected by gt_query_mask) to their
    nearest pred point -- searched among ALL pred points, as in eval.py -- each over the distances below max_dist only; overall = their mean.  Sums in
    f64.  An empty selection gives NaN means and zero counts.  -> ChamferResult.

    One host read-back, at the end: the two sums, the two counts and the state words."""
    pred, gt = _device.check_points("pred", pred), _device.check_points("gt", gt)
    max_dist = _device.check_positive("max_dist", max_dist, allow_zero=True)
    pm = _check_mask("pred_query_mask", pred_query_mask, pred.shape[0])
    gm = _check_mask("gt_query_mask", gt_query_mask, gt.shape[0])
    pred, gt = _device.check_cuda("mesh_eval", ("pred", pred), ("gt", gt))
    _device.check_cuda("mesh_eval", *([("pred", pred)] + [(n, m) for n, m in (("pred_query_mask", pm), ("gt_query_mask", gm)) if m is not None]))
    dev = pred.device
    state = new_state(dev)
    sums = _Sums(dev, state, 2)
    with torch.cuda.device(dev):
        pq = pred if pm is None else pred[pm]          # (an element-wise selection; torch sizes it with a read-back of its own)
        gq = gt if gm is None else gt[gm]
    d2s, _ = _nearest_async(pq, gt, max_dist, state)
    s2d, _ = _nearest_async(gq, pred, max_dist, state)
    sums.add(0, d2s, max_dist)
    sums.add(1, s2d, max_dist)
    (a, b), (na, nb) = sums.read("chamfer")
    ma, mb = _mean(a, na), _mean(b, nb)
    return ChamferResult(ma, mb, (ma + mb) / 2, na, nb, int(pq.shape[0]), int(gq.shape[0]))


def _fscore_from(np_, n_pred, nr, n_gt):
    if n_pred == 0 or n_gt == 0:
        return FScoreResult(0.0, 0.0, 0.0, 0, n_pred, 0, n_gt)          # (evaluation.py:191-194)
    precision, recall = np_ / n_pred, nr / n_gt
    f = 2 * recall * precision / (recall + precision) if recall + precision > 0 else 0.0
    return FScoreResult(precision, recall, f, np_, n_pred, nr, n_gt)


def fscore(pred, gt, tau):
    """Precision, recall and F-score at `tau` (evaluation.py:176-180): precision = the share of the pred points whose nearest gt point is nearer than tau,
    recall = the share of the gt points whose nearest pred point is, fscore = 2 p r / (p + r) (0 when both are 0); integer counts and one division each.
    The nearest search is cut off at 2 tau and the comparison is dist < tau in f32.  An empty set gives 0, as the reference does.  -> FScoreResult.

    One host read-back, at the end: the two counts and the state words."""
    pred, gt = _device.check_points("pred", pred), _device.check_points("gt", gt)
    tau = _device.check_positive("tau", tau)
    pred, gt = _device.check_cuda("mesh_eval", ("pred", pred), ("gt", gt))
    n_pred, n_gt = int(pred.shape[0]), int(gt.shape[0])
    if n_pred == 0 or n_gt == 0:
        return _fscore_from(0, n_pred, 0, n_gt)
    state = new_state(pred.device)
    sums = _Sums(pred.device, state, 2)
    sums.add(0, _nearest_async(pred, gt, 2 * tau, state)[0], tau)
    sums.add(1, _nearest_async(gt, pred, 2 * tau, state)[0], tau)
    _, (a, b) = sums.read("fscore")
    return _fscore_from(a, n_pred, b, n_gt)


def evaluate_mesh(mesh, gt_points, density=0.2, max_dist=20.0, tau=None, seed=0, include_vertices=True, max_points=None, pred_query_filter=None,
                  gt_query_mask=None):
    """eval.py:43-134 on a device mesh: sample its surface at `density`, visit the points in the order of a torch.randperm seeded with `seed` (the
    reference's shuffle is unseeded), thin them to a spacing of `density`, and take the Chamfer distance to gt_points with the cut-off max_dist; with `tau`
    also the F-score at tau between the thinned cloud and gt_points.

    DTU's observation mask and bounding box are element-wise selections on the thinned points: `pred_query_filter` is a callable that maps the thinned
    (M, 3) cloud to an (M,) bool mask of the points to query from (eval.py:98-110); gt_query_mask selects the ground-truth points to query from
    (eval.py:126-130).  The gt -> pred direction searches the whole thinned cloud.

    -> dict: mean_d2s, mean_s2d, overall, n_d2s, n_s2d, n_sampled, n_thinned, and with tau: precision, recall, fscore.
    Host read-backs: those of sample_surface, downsample, chamfer and fscore."""
    gt_points = _device.check_points("gt_points", gt_points)
    max_dist = _device.check_positive("max_dist", max_dist, allow_zero=True)
    if tau is not None:
        tau = _device.check_positive("tau", tau)
    _check_mask("gt_query_mask", gt_query_mask, gt_points.shape[0])
    v, f = _check_mesh(mesh)
    _device.check_positive("density", density)
    _device.check_cuda("mesh_eval", ("gt_points", gt_points), ("mesh.vertices", v), ("mesh.faces", f))
    cloud = sample_surface(mesh, density, include_vertices=include_vertices, max_points=max_points)
    dev = cloud.device
    with torch.cuda.device(dev):
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed))
        order = torch.randperm(cloud.shape[0], generator=g, device=dev)
        thinned = cloud[downsample(cloud, density, order=order)]
    mask = None
    if pred_query_filter is not None:
        mask = pred_query_filter(thinned)
    c = chamfer(thinned, gt_points, max_dist, pred_query_mask=mask, gt_query_mask=gt_query_mask)
    out = {"mean_d2s": c.mean_d2s, "mean_s2d": c.mean_s2d, "overall": c.overall, "n_d2s": c.n_d2s, "n_s2d": c.n_s2d,
           "n_sampled": int(cloud.shape[0]), "n_thinned": int(thinned.shape[0])}
    if tau is not None:
        f = fscore(thinned, gt_points, tau)
        out.update(precision=f.precision, recall=f.recall, fscore=f.fscore)
    return out
