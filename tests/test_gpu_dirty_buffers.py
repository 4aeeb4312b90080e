"""The image-side units on dirty, guard-banded buffers (tests/dirty_alloc.py), through the Python entry points the trainer calls: the
hourglass CNN forward and backward, the per-view colour front end, fused SSIM and image evaluation, the photometric and normal-consistency terms, and the
glue units (activations, L1, depth normal).

THE CONTRACT: an output or a scratch arena may hold anything on entry, and nothing outside it is written.  Each case runs its unit plain and then with every
`torch.empty` / `torch.empty_like` of the wrapper served from a block of 0x00, 0xFF and 0x40 bytes between two 4 KiB guards (dirty_alloc.check): every
returned tensor and every gradient must have the same bits in all runs (none of these units uses float atomics: the same arguments give the same bits), no
NaN may appear, no guard byte may change, and at least as many allocations must have been intercepted as the wrapper makes for the call -- that number stands
beside each call below, counted in the wrapper's code (outputs + arenas; `_device.scratch` is one).  A stale read that reaches a result, an element nobody
stores, a store past an end: each fails a comparison here; nothing is meant to fault (the arenas of these units hold float, half and double data, the front
end's two counter words are cleared by the host ahead of the launch, and its device `levels` word is clamped to 0 .. S before use).

Inputs, parameters and upstream gradients come from the case builders of the units' own test files and are built outside the patched region.  Each case
prints its intercepted counts and "guards intact"."""
import functools

import pytest
import torch

from ibgs_amd import activations, coloragg, depthnormal, hourglass, image_eval, losses
from tests import dirty_alloc as da
from tests import glue_edges as ge
from tests import hourglass_ref as href
from tests import test_gpu_coloragg as cagg
from tests import test_gpu_geoloss as geo
from tests import test_gpu_glue_bounds as glue
from tests import test_gpu_hourglass as fwd
from tests import test_gpu_hourglass_train as bwd
from tests import test_gpu_ssim as ssim_t

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = fwd.T


def _clear():
    """The module-level cache that would hand back an earlier buffer: l1_loss keeps its arena per stream.  (No unit here goes through the renderer.)"""
    losses._scratch.clear()


@pytest.fixture(autouse=True)
def _no_dirty_block_outlives_its_test():
    yield
    _clear()


def _check(label, call, min_count):
    return da.check(label, call, DEV, min_count, before=_clear)


def _dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


# ---- 1. the hourglass forward, float32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "half_dead"])          # dead channels are where a skipped store hides: a stale 0 is the right answer there
@pytest.mark.parametrize("h,w", [(5, 7), (17, 67), (2 * T + 3, 2 * T + 5)])
def test_hourglass_forward(h, w, kind):
    assert (h, w) in fwd.FRAMES
    x = _dev(href.seeded_input(1000 * h + w, h, w))
    net = fwd._net(kind)

    def call():
        with torch.no_grad():
            # residual, image_pred, the arena (3)  +  residual, the arena (2)
            return {"burned 0.75": hourglass.hourglass_forward(x, net, render_scale=0.75, return_stages=True), "no image_pred": hourglass.hourglass_forward(x, net, return_stages=True)}
    base = dict(_check("hourglass_forward %dx%d %s" % (h, w, kind), call, 3 + 2))
    assert len(base) == 2 + 6 + 1 + 6 and tuple(base["['burned 0.75'][2]['b']"].shape) == (9, h // 4, w // 4)


# ---- 2. the hourglass backward ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _live_net(kind):
    net = hourglass.HourglassCNN()
    net.load_state_dict({k: torch.tensor(v) for k, v in fwd._params(kind).items()})
    return net.to(DEV)


@pytest.mark.parametrize("kind", ["default", "half_dead"])
@pytest.mark.parametrize("h,w", [(5, 7), (17, 67), (35, 37)])
def test_hourglass_backward(h, w, kind):
    """The decided cases of tests/test_hourglass_train_host.py (shared with tests/test_gpu_hourglass_train.py: computed once).  All 19 gradients are compared,
    raw and through autograd; then one group without the other, and one upstream only.  The nine weight-gradient launches share one `partial` region of the
    scratch arena, each with its own padded layout, and the un-pooling writes E2 and B in place: a word one launch leaves for the next to read shows here."""
    c = bwd._case(h, w, kind)
    tag = "%dx%d %s" % (h, w, kind)
    frozen, live = fwd._net(kind), _live_net(kind)
    x, g_res, g_ip = _dev(c["x"]), _dev(c["g_res"]), _dev(c["g_ip"])
    stages = {k: _dev(v) for k, v in c["stages32"].items()}
    raw = lambda *ups, **kw: (lambda: hourglass.hourglass_backward(x, frozen, stages, *ups, render_scale=c["burned"], **kw))

    def autograd():
        leaf = x.clone().requires_grad_(True)
        residual, image_pred = hourglass.hourglass_train(leaf, live, render_scale=c["burned"])
        grads = torch.autograd.grad([residual, image_pred], [leaf] + [getattr(live, k) for k in bwd.NAMES], [g_res, g_ip])
        return residual.detach(), image_pred.detach(), dict(zip(["x"] + bwd.NAMES, grads))
    # hourglass_backward on a dict of stages: the stages arena, grad_x, 18 parameter gradients, the scratch arena
    base = _check("hourglass_backward %s raw" % tag, raw(g_res, g_ip), 1 + 1 + 18 + 1)
    assert len(base) == 19
    # hourglass_train: residual, image_pred, the owned arena; its backward: grad_x, 18 gradients, the scratch arena
    through = _check("hourglass_train + autograd.grad %s" % tag, autograd, 3 + 20)
    assert len(through) == 2 + 19
    _check("hourglass_backward %s need_param_grads=False" % tag, raw(g_res, g_ip, need_param_grads=False), 1 + 1 + 1)
    _check("hourglass_backward %s need_input_grad=False" % tag, raw(g_res, g_ip, need_input_grad=False), 1 + 18 + 1)
    _check("hourglass_backward %s grad_residual only" % tag, raw(g_res, None), 1 + 1 + 18 + 1)
    _check("hourglass_backward %s grad_image_pred only" % tag, raw(None, g_ip), 1 + 1 + 18 + 1)


# ---- 3. the per-view colour front end ------------------------------------------------------------------------------------------------------------------------
# per_view_features with the levels counted on the device: the levels word, the counting arena, the output (3); its backward: six gradients, the arena (7)
FRONT_END = 3 + 7
CHUNK = cagg.CHUNK


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("frame", [(3, 5), (17, 67), (1, CHUNK + 1)], ids=lambda s: "x".join(map(str, s)))
def test_front_end_frames(frame, mode):
    case = cagg._case(3, *frame)
    base = _check("per_view_features %dx%d S3 %s" % (frame + (mode,)), lambda: cagg._fused(*case, cagg._params(), 3, mode), FRONT_END)
    assert int(dict(base)["[1]"]) == 3


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("live", [0, 3])
def test_front_end_levels_counted_on_the_device(live, mode):
    """The count is formed from two words of the arena that the host clears ahead of the launch; left dirty, the last ticket never comes and the levels word
    keeps what the block held."""
    case = cagg._case(5, 9, 11, live)
    base = _check("per_view_features 9x11 S5 live %d %s" % (live, mode), lambda: cagg._fused(*case, cagg._params(), 5, mode), FRONT_END)
    assert int(dict(base)["[1]"]) == live


def test_front_end_beyond_the_backward_grid():
    """520 rows of CHUNK pixels for 512 workgroups: workgroups walk more than one chunk, and the final sum reads every row of partials."""
    h, w = cagg.BWD_GROUPS + 8, CHUNK
    case = cagg._case(2, h, w)
    _check("per_view_features %dx%d S2 mean" % (h, w), lambda: cagg._fused(*case, cagg._params(), 2, "mean"), FRONT_END)


def test_fuse_color_inputs():
    h, w = 17, 67
    render, warped, feat, ray, up = cagg._case(3, h, w)
    front = coloragg.PerViewFrontEnd("mean").to(DEV)
    with torch.no_grad():
        for n, p in zip(("w1", "b1", "w2", "b2"), cagg._params()):
            getattr(front, n).copy_(p)
    depth_diff = torch.rand(1, h, w, generator=torch.Generator().manual_seed(4)).to(DEV) * 1.2

    def call():
        pkg = {"render": render.clone().requires_grad_(True), "warped_image": warped.reshape(9, h, w).clone().requires_grad_(True), "cam_feat": feat.reshape(12, h, w),
               "camera_ray": ray.reshape(3, h * w), "min_depth_diff": depth_diff}
        cnn_input, mask = coloragg.fuse_color_inputs(pkg, front, 3)
        grads = torch.autograd.grad((cnn_input * up).sum(), [pkg["render"], pkg["warped_image"], front.w1, front.b1, front.w2, front.b2])
        return cnn_input.detach(), mask, grads
    _check("fuse_color_inputs %dx%d S3" % (h, w), call, FRONT_END)


# ---- 4. SSIM and image evaluation --------------------------------------------------------------------------------------------------------------------------
TILE_H, TILE_W = ssim_t.TILE_H, ssim_t.TILE_W


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (1, 3, 11, 11), (1, 3, TILE_H + 1, TILE_W + 1), (2, 3, TILE_H + 3, TILE_W + 3)], ids=lambda s: "x".join(map(str, s)))
def test_ssim_and_image_metrics(shape):
    a, b = ssim_t._pair("near", shape)
    up = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    wt = torch.tensor([0.7, -1.3], device=DEV)[:shape[0]]
    tag = "x".join(map(str, shape))

    def value(wrt, **kw):
        def call():
            ins = ssim_t._leaves(a, b, wrt)
            v = losses.ssim(*ins, **kw)
            return v.detach(), torch.autograd.grad(v if v.dim() == 0 else (v * wt).sum(), [ins[k] for k in wrt])
        return call

    def the_map():
        ins = ssim_t._leaves(a, b, (0, 1))
        m = losses.ssim_map(*ins)
        return m.detach(), torch.autograd.grad((m * up).sum(), ins)

    def no_grad():
        with torch.no_grad():
            return losses.ssim(a, b), losses.ssim_map(a, b)
    # ssim: the mean, the derivative planes, the sums' arena; the backward's gradient
    _check("ssim %s wrt img1" % tag, value((0,)), 3 + 1)
    # both images: a second launch for the other side's derivative planes (no sums, no arena), two gradients
    _check("ssim %s wrt both" % tag, value((0, 1)), 3 + 1 + 2)
    # per image: the mean (unused), the per-image means, the planes, the arena, the gradient
    _check("ssim %s per image" % tag, value((0,), size_average=False), 4 + 1)
    # ssim_map: the map, two sets of derivative planes, two gradients (no sums: no arena)
    _check("ssim_map %s wrt both" % tag, the_map, 3 + 2)
    # under no_grad: the mean and the arena; the map
    _check("ssim, ssim_map %s no_grad" % tag, no_grad, 2 + 1)
    # image_metrics: three per-image vectors and the arena
    _check("image_metrics %s" % tag, lambda: image_eval.image_metrics(a, b), 3 + 1)


# ---- 5. the photometric and the normal-consistency term ------------------------------------------------------------------------------------------------------
T_H, T_W = geo.T_H, geo.T_W
GEO_FRAMES = [(1, 1), (11, 11), (T_H + 1, T_W + 1), (2 * T_H - 1, 2 * T_W + 5)]


@pytest.mark.parametrize("sources", [(1, 3), (4, 3)], ids=lambda s: "S%d_of_%d" % (min(s[1], s[0]), s[0]))          # (S_total, nb_visible_src_frames): one source read, three read
@pytest.mark.parametrize("frame", GEO_FRAMES, ids=lambda s: "x".join(map(str, s)))
def test_photometric_loss(frame, sources):
    st, nb = sources
    gt, warped, feat, _ = geo._case("near", st, *frame)
    tag = "%dx%d S%d/%d" % (frame + (min(nb, st), st))
    # the value, the valid-pixel count, the derivative planes, the tiles' arena; the backward's gradient
    _check("photometric_loss %s" % tag, lambda: geo._fused(gt, warped, feat, nb, 0.3, 1.0), 4 + 1)
    base = _check("photometric_loss %s, no valid pixel" % tag, lambda: geo._fused(gt, warped, torch.zeros_like(feat), nb, 0.3, 1.0), 4 + 1)
    assert float(base[0][1]) == 0.0 and float(base[1][1].abs().max()) == 0.0


@pytest.mark.parametrize("frame", GEO_FRAMES, ids=lambda s: "x".join(map(str, s)))
def test_normal_consistency(frame):
    n, dn = geo._normals("raw", *frame)
    up = torch.tensor(0.25, device=DEV)

    def call():
        a, b = n.clone().requires_grad_(True), dn.clone().requires_grad_(True)
        v = losses.normal_consistency(a, b)
        first = torch.autograd.grad(v, [a, b], up, retain_graph=True)
        return v.detach(), first, torch.autograd.grad(v, [a, b], up)          # a second backward through the same node: from n and dn again
    # the value, two unit gradients, the arena; the second backward's launch: the same four
    _check("normal_consistency %dx%d" % frame, call, 4 + 4)


# ---- 6. the glue units ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 65, 1000])
def test_fused_activations(P):
    s, r, o, gs, gr, go = glue._raw(P, P)

    def call():
        leaves = [t.clone().requires_grad_(True) for t in (s, r, o)]
        outs = activations.fused_activations(*leaves)
        return [t.detach() for t in outs], torch.autograd.grad(outs, leaves, [gs, gr, go])
    # three outputs; three gradients
    _check("fused_activations P=%d" % P, call, 3 + 3)


@pytest.mark.parametrize("n", [1, 5, 4097])
def test_l1_loss(n):
    gen = torch.Generator(device=DEV).manual_seed(n)
    a, b = torch.rand(n, device=DEV, generator=gen), torch.rand(n, device=DEV, generator=gen)
    up = torch.tensor(0.75, device=DEV)

    def call():
        x = a.clone().requires_grad_(True)
        v = losses.l1_loss(x, b)
        (first,) = torch.autograd.grad(v, x, up, retain_graph=True)          # the forward's unit gradient, scaled in place
        (second,) = torch.autograd.grad(v, x, up)                            # from x and y again
        return v.detach(), first, second
    # the value, the arena (its cache is emptied before each run), the unit gradient; the second backward's gradient
    base = _check("l1_loss n=%d" % n, call, 3 + 1)
    assert torch.equal(base[1][1], base[2][1])


@pytest.mark.parametrize("case", ["65x9", "2x2"])
def test_depth_normal(case):
    r = ge.reference(case)
    depth, cot = r.depth.to(DEV).contiguous(), r.cot.to(DEV).contiguous()

    def call():
        d = depth.clone().requires_grad_(True)
        normal = depthnormal.depth_normal(r.cam, d)
        return normal.detach(), torch.autograd.grad(normal, d, cot)
    # the normal map; the depth's gradient
    _check("depth_normal %s" % case, call, 1 + 1)
