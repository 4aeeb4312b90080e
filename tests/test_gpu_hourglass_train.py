"""The backward of the hourglass CNN (ibgs_amd.hourglass `hourglass_backward`, `hourglass_train`, `fuse_color_train`; csrc/hgtrain.hip) on the device.

The ARBITER is tests/hourglass_bwd_ref.backward_ref (float64 numpy) on the float64 forward's stages.  The YARDSTICK of each of the 19 gradient tensors is
d_ref = max(d_torch32, d_chain32): the max-abs distances from the arbiter of torch autograd of the float32 composition ON THE CPU and of
tests/hourglass_bwd_ref.backward_chain_f32 (on the float32 chain forward's stages).  THE BAR is the project's (DESIGN.md sections 12-15):
max |hip - f64| <= F64_K x d_ref (F64_K = 2); where d_ref is exactly 0: 2^-22 max |f64|.  Two yardsticks for section 15's reason: torch's blocked CPU sums
alone would refuse a correct chain, a chain alone would be a yardstick chosen here.  Every case is DECIDED (tests/test_hourglass_train_host.py: its seed is
searched on the CPU so that no ReLU or pool decision is within float32's reach of flipping): nothing is skipped or masked out of a comparison.  Every
comparison prints err, both distances and the ratio before it asserts; bit-for-bit properties are asserted with torch.equal."""
import functools
import time

import numpy as np
import pytest
import torch

from ibgs_amd import coloragg, hourglass
from tests import coloragg_ref
from tests import hourglass_bwd_ref as bref
from tests import hourglass_ref as ref
from tests import test_gpu_hourglass as fwd
from tests import test_hourglass_train_host as host

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
FRAMES = host.FRAMES + [f for f in host.wgrad_frames() if f not in host.FRAMES]
NAMES = [k for k in bref.GRADS if k != "x"]


def _distances(want, t32, chain):
    both = {k: (float(np.abs(t32[k].astype(np.float64) - want[k]).max()), float(np.abs(chain[k].astype(np.float64) - want[k]).max())) for k in bref.GRADS}
    return {k: max(v) for k, v in both.items()}, both


@functools.lru_cache(maxsize=None)
def _case(h, w, kind, upstream="both", burned=0.75):
    """Computed once and shared; nobody writes it.  -> dict: x, p, g_res, g_ip (float32 numpy or None), stages32 (the torch float32 CPU composition's, to
    upload), want (the arbiter's 19 gradients), d_ref, both."""
    seed = host.decided_seed(h, w, kind)
    p = fwd._params(kind)
    x = ref.seeded_input(seed, h, w)
    g = np.random.default_rng(seed + 7)
    g_res, g_ip = g.standard_normal((3, h, w)).astype(np.float32), g.standard_normal((3, h, w)).astype(np.float32)
    if upstream == "patch":          # zero outside one 3 x 3 patch that straddles a corner of the 16 x 16 tiles (and of the 8 x 16 ones)
        keep = np.zeros((1, h, w), dtype=np.float32)
        keep[:, 15:18, 15:18] = 1
        g_res, g_ip = g_res * keep, g_ip * keep
    if upstream == "residual":
        g_ip = None
    if upstream == "image_pred":
        g_res = None
    stages32 = {k: v.numpy() for k, v in ref.torch_composition(x, p, torch.float32).items() if k in ref.STAGES}
    want = bref.backward_ref(x, p, ref.forward_ref(x, p), g_res, g_ip, burned)
    t32 = bref.torch_grads(x, p, g_res, g_ip, burned, torch.float32)
    chain = bref.backward_chain_f32(x, p, ref.chain_f32(x, p), g_res, g_ip, burned)
    d_ref, both = _distances(want, t32, chain)
    return dict(x=x, p=p, g_res=g_res, g_ip=g_ip, stages32=stages32, want=want, d_ref=d_ref, both=both, burned=burned)


def _dev(a):
    return None if a is None else torch.as_tensor(a).cuda()


def _compare(tag, got, want, d_ref, both, failed=None):
    """got: {name: device tensor}.  Every tensor is printed before the first failure is raised; with a list `failed` the misses are appended to it instead."""
    collect = failed is not None
    failed = failed if collect else []
    for k in bref.GRADS:
        w64 = torch.as_tensor(want[k], dtype=torch.float64, device="cuda")
        t = got[k].reshape(w64.shape)
        assert t.dtype == torch.float32, (tag, k)
        err, d = float((t.double() - w64).abs().max()), d_ref[k]
        print("%-44s err %.3e  d_ref %.3e (torch %.3e, chain %.3e)  max|f64| %.3e  ratio %s" % (tag + " " + k, err, d, both[k][0], both[k][1], float(w64.abs().max()),
                                                                                            "%.2f" % (err / d) if d > 0 else "-"))
        ok = err <= F64_K * d if d > 0 else err <= FLOOR * float(w64.abs().max())
        if not ok:
            failed.append((tag, k, err, d))
    assert collect or not failed, failed


def _raw(c, net, **kw):
    x = _dev(c["x"])
    gx, gp = hourglass.hourglass_backward(x, net, {k: _dev(v) for k, v in c["stages32"].items()}, _dev(c["g_res"]), _dev(c["g_ip"]), render_scale=c["burned"], **kw)
    return gx, gp


def _autograd(c, net_kind, retain=False):
    net = hourglass.HourglassCNN()
    net.load_state_dict({k: torch.tensor(v) for k, v in c["p"].items()})
    net = net.cuda()
    x = _dev(c["x"]).requires_grad_(True)
    residual, image_pred = hourglass.hourglass_train(x, net, render_scale=c["burned"])
    outs = [o for o, g in ((residual, c["g_res"]), (image_pred, c["g_ip"])) if g is not None]
    ups = [_dev(g) for g in (c["g_res"], c["g_ip"]) if g is not None]
    grads = torch.autograd.grad(outs, [x] + [getattr(net, k) for k in NAMES], ups, retain_graph=retain)
    return dict(zip(["x"] + NAMES, grads)), (x, net, residual, image_pred)


# ---- 1. frames x parameter sets --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", host.KINDS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_gradients_against_float64(h, w, kind):
    """Both paths are printed before the first miss is raised.  The measured min - max (mean) of err / d_ref per tensor: DESIGN.md section 15.  (With the weight
    gradient's pixel sums kept in float32 over a whole strip, 4 x 33 default dec1_b came out at 2.16: a bias gradient's partial sums are several times its
    value, and their rounding is the error.  The sums are kept in double since.)"""
    c = _case(h, w, kind)
    tag = "%dx%d %s" % (h, w, kind)
    failed = []
    gx, gp = _raw(c, fwd._net(kind))
    torch.cuda.synchronize()
    assert tuple(gx.shape) == (38, h, w) and sorted(gp) == sorted(NAMES)
    _compare(tag + " raw", dict(gp, x=gx), c["want"], c["d_ref"], c["both"], failed)
    got, _ = _autograd(c, kind)          # ... and through autograd, where the stages are the forward kernel's
    assert tuple(got["x"].shape) == (1, 38, h, w)
    _compare(tag + " autograd", got, c["want"], c["d_ref"], c["both"], failed)
    assert not failed, failed


# ---- 2. one upstream, burned 1, a patch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream,burned", [("residual", 0.75), ("image_pred", 0.75), ("both", 1.0)])
def test_one_upstream_and_burned_one(upstream, burned):
    c = _case(16, 24, "default", upstream, burned)
    gx, gp = _raw(c, fwd._net("default"))
    _compare("16x24 %s %.2f raw" % (upstream, burned), dict(gp, x=gx), c["want"], c["d_ref"], c["both"])
    got, _ = _autograd(c, "default")
    _compare("16x24 %s %.2f autograd" % (upstream, burned), got, c["want"], c["d_ref"], c["both"])


def test_a_patch_of_upstream_leaves_exact_zeros_outside_its_reach():
    h, w = 35, 37
    c = _case(h, w, "default", "patch")
    gx, gp = _raw(c, fwd._net("default"))
    _compare("35x37 patch raw", dict(gp, x=gx), c["want"], c["d_ref"], c["both"])
    # where the arbiter's input gradient is exactly zero no term reaches the element (it lies outside the patch's receptive field: the last rows and columns
    # of the frame): exactly 0 here too
    zero = torch.as_tensor(c["want"]["x"] == 0, device="cuda")
    share = float(zero.float().mean())
    print("35x37 patch: %.3f of grad_x is outside the patch's reach" % share)
    assert share > 0.2 and bool(torch.all(gx[zero] == 0))


# ---- 3. ties and handed stages -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tied_case():
    """Hand-made stages whose pool windows hold equal positive values (quantised to 0, 1/4, 1/2), on a seed at which the recomputed d1 and f are decided."""
    h, w = 9, 11
    p = fwd._params("default")
    sides = {"e1": (38, h, w), "e2": (19, h // 2, w // 2), "b": (9, h // 4, w // 4), "u2": (19, h // 2, w // 2), "d2": (19, h // 2, w // 2), "u1": (38, h, w)}
    for seed in range(900, 932):
        g = np.random.default_rng(seed)
        stages = {k: (g.integers(0, 3, size=s) * 0.25).astype(np.float32) for k, s in sides.items()}
        x = ref.seeded_input(seed, h, w)
        relu = lambda t: np.maximum(t, 0)
        cat1 = np.concatenate([stages["u1"], stages["e1"]])
        pre1 = ref._conv_f64(cat1.astype(np.float64), p["dec1_w"], p["dec1_b"])
        pre0 = ref._conv_f64(np.concatenate([relu(pre1), x[0].astype(np.float64)]), p["fuse_input_w"], p["fuse_input_b"])
        c1 = ref._conv_chain(cat1, p["dec1_w"], p["dec1_b"])
        c0 = ref._conv_chain(np.concatenate([relu(c1), x[0]]), p["fuse_input_w"], p["fuse_input_b"])
        # decided as the cases above are: 4 x the float32 chain's distance from float64 (of the pre-activations themselves, which bounds that of d1 and f)
        if np.abs(pre1).min() >= 4 * np.abs(c1 - pre1).max() and np.abs(pre0).min() >= 4 * np.abs(c0 - pre0).max():
            break
    else:
        assert False, "no decided seed for the tied stages"
    g_res, g_ip = g.standard_normal((3, h, w)).astype(np.float32), g.standard_normal((3, h, w)).astype(np.float32)
    want = bref.backward_ref(x, p, stages, g_res, g_ip, 0.75)
    chain = bref.backward_chain_f32(x, p, stages, g_res, g_ip, 0.75)
    d_ref, both = _distances(want, chain, chain)
    win = stages["e1"][:, :8, :10].reshape(38, 4, 2, 5, 2).transpose(0, 1, 3, 2, 4).reshape(38, 4, 5, 4)
    top = win.max(-1)
    assert int((((win == top[..., None]).sum(-1) > 1) & (top > 0)).sum()) > 100          # many windows with a positive tie
    return dict(x=x, p=p, g_res=g_res, g_ip=g_ip, stages32=stages, want=want, d_ref=d_ref, both=both, burned=0.75)


def test_ties_go_to_the_first_maximum_on_handed_stages():
    c = _tied_case()
    gx, gp = _raw(c, fwd._net("default"))
    _compare("9x11 tied (d_ref: the chain's)", dict(gp, x=gx), c["want"], c["d_ref"], c["both"])


# ---- 4. exact ------------------------------------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    h, w = 17, 67
    c = _case(h, w, "default")
    frozen = fwd._net("default")
    got, (x, net, residual, image_pred) = _autograd(c, "default", retain=True)
    with torch.no_grad():
        r0, ip0 = hourglass.hourglass_forward(x.detach(), frozen, render_scale=0.75)
        plain = hourglass.hourglass_forward(x.detach(), frozen)
    assert torch.equal(residual, r0) and torch.equal(image_pred, ip0) and residual.requires_grad and image_pred.requires_grad
    lone = hourglass.hourglass_train(x, net)
    assert torch.is_tensor(lone) and torch.equal(lone, plain)
    # the gradients of the autograd path are hourglass_backward's on the arena the node saved
    saved = residual.grad_fn.saved_tensors
    arena = [t for t in saved if t.dtype == torch.uint8]
    assert len(arena) == 1
    arena = arena[0]
    arena0, x0, p0 = arena.clone(), x.detach().clone(), [q.detach().clone() for q in net.parameters()]
    g_res, g_ip = _dev(c["g_res"]), _dev(c["g_ip"])
    g0 = (g_res.clone(), g_ip.clone())
    gx, gp = hourglass.hourglass_backward(x.detach(), net, arena, g_res, g_ip, render_scale=0.75)
    assert torch.equal(gx, got["x"][0]) and all(torch.equal(gp[k], got[k]) for k in NAMES)
    # a second call, and a side stream
    gx2, gp2 = hourglass.hourglass_backward(x.detach(), net, arena, g_res, g_ip, render_scale=0.75)
    assert torch.equal(gx2, gx) and all(torch.equal(gp2[k], gp[k]) for k in NAMES)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gx3, gp3 = hourglass.hourglass_backward(x.detach(), net, arena, g_res, g_ip, render_scale=0.75)
    s.synchronize()
    assert torch.equal(gx3, gx) and all(torch.equal(gp3[k], gp[k]) for k in NAMES)
    # strides, channels last, float64
    xd = x.detach()
    wide = torch.zeros(1, 38, h, 2 * w + 1, device="cuda")
    wide[..., ::2][..., :w] = xd
    views = {"(38, H, W)": xd[0], "every other column": wide[..., ::2][..., :w], "channels last": xd.contiguous(memory_format=torch.channels_last), "float64": xd.double()}
    for what, v in views.items():
        gv = g_res.double() if what == "float64" else g_res.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        a, b = hourglass.hourglass_backward(v, net, arena, gv, g_ip, render_scale=0.75)
        assert torch.equal(a, gx) and all(torch.equal(b[k], gp[k]) for k in NAMES), what
    # one group without the other
    only_x, none = hourglass.hourglass_backward(xd, net, arena, g_res, g_ip, render_scale=0.75, need_param_grads=False)
    none2, only_p = hourglass.hourglass_backward(xd, net, arena, g_res, g_ip, render_scale=0.75, need_input_grad=False)
    assert none is None and none2 is None and torch.equal(only_x, gx) and all(torch.equal(only_p[k], gp[k]) for k in NAMES)
    with pytest.raises(ValueError, match="neither"):
        hourglass.hourglass_backward(xd, net, arena, g_res, need_input_grad=False, need_param_grads=False)
    with pytest.raises(ValueError, match="both None"):
        hourglass.hourglass_backward(xd, net, arena)
    # a dict of the stages is packed into the same arena
    a, b = hourglass.hourglass_backward(xd, net, hourglass._arena_views(arena, h, w), g_res, g_ip, render_scale=0.75)
    assert torch.equal(a, gx) and all(torch.equal(b[k], gp[k]) for k in NAMES)
    torch.cuda.synchronize()
    assert torch.equal(arena, arena0) and torch.equal(xd, x0) and all(torch.equal(q, q0) for q, q0 in zip(net.parameters(), p0))
    assert torch.equal(g_res, g0[0]) and torch.equal(g_ip, g0[1])
    # double backward raises
    x2 = xd.clone().requires_grad_(True)
    r2 = hourglass.hourglass_train(x2, net)
    (gx_graph,) = torch.autograd.grad(r2, x2, g_res, create_graph=True)
    with pytest.raises(RuntimeError):
        gx_graph.sum().backward()


@pytest.mark.parametrize("h,w", [(5, 7), (17, 67)])
def test_writer_reader_and_views_share_one_layout(h, w):
    """The six stages `hourglass_forward` returns -- the Python views of the arena its kernels wrote, cloned -- handed to `hourglass_backward` as a dict give, bit
    for bit, the gradients autograd obtains through `hourglass_train`, whose backward reads the forward's arena as it lies: the forward's carve, the
    backward's and hourglass._arena_views are one layout (csrc/shared/hg_net.h; odd sides: the H / 2 / 2 rounding)."""
    c = _case(h, w, "default")
    got, (x, net, _, _) = _autograd(c, "default")
    with torch.no_grad():
        _, _, views = hourglass.hourglass_forward(x.detach(), net, render_scale=c["burned"], return_stages=True)
        stages = {k: v.clone() for k, v in views.items()}
    assert list(stages) == [n for n, _, _ in hourglass.STAGES]
    gx, gp = hourglass.hourglass_backward(x.detach(), net, stages, _dev(c["g_res"]), _dev(c["g_ip"]), render_scale=c["burned"])
    assert torch.equal(gx, got["x"].reshape(gx.shape)) and all(torch.equal(gp[k], got[k]) for k in NAMES)


# ---- 5. pruning ------------------------------------------------------------------------------------------------------------------------------------------------
def test_only_what_autograd_needs():
    c = _case(16, 24, "default")
    full, _ = _autograd(c, "default")
    frozen = fwd._net("default")          # requires_grad_(False)
    x = _dev(c["x"]).requires_grad_(True)
    r, ip = hourglass.hourglass_train(x, frozen, render_scale=0.75)
    torch.autograd.backward([r, ip], [_dev(c["g_res"]), _dev(c["g_ip"])])
    assert torch.equal(x.grad, full["x"]) and all(q.grad is None for q in frozen.parameters())
    live = hourglass.HourglassCNN()
    live.load_state_dict({k: torch.tensor(v) for k, v in c["p"].items()})
    live = live.cuda()
    x = _dev(c["x"])
    r, ip = hourglass.hourglass_train(x, live, render_scale=0.75)
    torch.autograd.backward([r, ip], [_dev(c["g_res"]), _dev(c["g_ip"])])
    assert x.grad is None and all(torch.equal(getattr(live, k).grad, full[k]) for k in NAMES)
    # only one output used: the other's gradient is absent, not a plane of zeros
    x = _dev(c["x"]).requires_grad_(True)
    r, ip = hourglass.hourglass_train(x, live, render_scale=0.75)
    want = hourglass.hourglass_backward(x.detach(), live, ip.grad_fn.saved_tensors[1], None, _dev(c["g_ip"]), render_scale=0.75, need_param_grads=False)[0]
    (g_only,) = torch.autograd.grad(ip, x, _dev(c["g_ip"]))
    assert torch.equal(g_only[0], want)
    with torch.no_grad():          # nothing requires grad under no_grad: the forward alone
        r2 = hourglass.hourglass_train(_dev(c["x"]), live)
    assert not r2.requires_grad and torch.equal(r2, r)


# ---- 6. the call never waits -------------------------------------------------------------------------------------------------------------------------------
def test_the_backward_never_waits():
    c = _case(17, 67, "default")
    net = fwd._net("default")
    x, g_res, g_ip = _dev(c["x"]), _dev(c["g_res"]), _dev(c["g_ip"])
    stages = {k: _dev(v) for k, v in c["stages32"].items()}
    want = hourglass.hourglass_backward(x, net, stages, g_res, g_ip, render_scale=0.75)
    a = torch.rand(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    start, queued, done = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    start.record()
    for _ in range(40):
        a = (a @ a).clamp_(0, 1)
    queued.record()
    t0 = time.perf_counter()
    got = hourglass.hourglass_backward(x, net, stages, g_res, g_ip, render_scale=0.75)
    host_ms = (time.perf_counter() - t0) * 1e3
    still_running = not queued.query()
    done.record()
    torch.cuda.synchronize()
    print("backward: host %.3f ms; the queue in front of it %.3f ms on the device, its own kernels %.3f ms" % (host_ms, start.elapsed_time(queued), queued.elapsed_time(done)))
    assert still_running, "hourglass_backward returned only after the work queued in front of it had finished: something in it waits for the device"
    assert host_ms < start.elapsed_time(queued)
    assert torch.equal(got[0], want[0]) and all(torch.equal(got[1][k], want[1][k]) for k in NAMES)


# ---- 7. end to end: the rasterizer's outputs in, gradients out ---------------------------------------------------------------------------------------------
def _torch_tail(pkg, sd_front, sd_cnn, g, burned, dtype):
    """fuse_color_inputs -> the CNN -> image_pred in torch ops on the CPU at `dtype`; -> gradients of (image_pred g).sum() in the CNN's and the front end's
    parameters and in render, and the forward's pre-activation facts for the decidedness check."""
    cpu = lambda t: t.detach().cpu()
    render = cpu(pkg["render"]).to(dtype).requires_grad_(True)
    fp = {k: cpu(v).to(dtype).requires_grad_(True) for k, v in sd_front.items()}
    h, w = render.shape[1:]
    cnn_input = coloragg_ref.torch_composition(render, cpu(pkg["warped_image"]), cpu(pkg["cam_feat"]), cpu(pkg["camera_ray"]).view(3, h, w), fp["w1"], fp["b1"], fp["w2"], fp["b2"],
                                               3, "mean", dtype)
    cp = {k: cpu(v).to(dtype).requires_grad_(True) for k, v in sd_cnn.items()}
    F = torch.nn.functional
    conv = lambda v, name, pad: F.conv2d(v, cp[name + "_w"], cp[name + "_b"], padding=pad)
    x = cnn_input
    e1 = F.relu(conv(x, "enc1", 1))
    e2 = F.relu(conv(F.max_pool2d(e1, 2), "enc2", 1))
    b = F.relu(conv(F.max_pool2d(e2, 2), "enc3", 1))
    u2 = F.relu(conv(F.interpolate(b, size=e2.shape[-2:], mode="nearest"), "up2_conv", 1))
    d2 = F.relu(conv(torch.cat([u2, e2], 1), "dec2", 1))
    u1 = F.relu(conv(F.interpolate(d2, size=e1.shape[-2:], mode="nearest"), "up1_conv", 1))
    d1 = F.relu(conv(torch.cat([u1, e1], 1), "dec1", 1))
    f = F.relu(conv(torch.cat([d1, x], 1), "fuse_input", 0))
    image_pred = burned * render + conv(f, "final", 0)[0]
    names = list(cp) + list(fp)
    grads = torch.autograd.grad((image_pred * cpu(g).to(dtype)).sum(), [cp[k] for k in cp] + [fp[k] for k in fp] + [render])
    out = {k: v.numpy() for k, v in zip(names + ["render"], grads)}
    return out, cnn_input.detach().numpy()


def test_end_to_end_from_the_rasterizer():
    from ibgs_amd import renderer, simple_scene, synthetic as syn
    dev = torch.device("cuda")
    W, H, P = 48, 32, 700
    g = syn.make_gaussians(P, 61, sh_degree=1, max_coeffs=4, opacity="trained")
    g["scales"] = (g["scales"] * 2.2).astype(np.float32)
    rng = np.random.default_rng(61)
    g["normal"] = rng.normal(size=(P, 3)).astype(np.float32)
    g["offset"] = (0.02 * rng.normal(size=(P, 1))).astype(np.float32)
    cams = simple_scene.orbit_cameras(W, H, n_views=4, device=dev, nearest=3)
    pc = simple_scene.SimpleGaussians(g, sh_degree=1, device=dev)
    imgs = torch.rand(4, 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(61))
    scn = simple_scene.SimpleScene(cams, images=imgs, device=dev)
    pipe, args = simple_scene.default_pipe(), simple_scene.default_args()
    cam = cams[0]
    up = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(62))
    renderer.clear_caches()
    try:
        with torch.no_grad():
            for j in cam.nearest_id:
                scn.rendered_depth_list[j] = renderer.render_depth(cams[j], pc, scn, pipe, args, torch.zeros(3, device=dev), True, 3, 4)
            pkg = renderer.render(cam, pc, scn, pipe, args, torch.zeros(3, device=dev), learnt_normal=True, nb_src_frames=3, buffer_length=4, render_geo=True)
        pkg = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in pkg.items()}
        for key in ("render", "warped_image"):
            pkg[key].requires_grad_(True)
        torch.manual_seed(7)
        net = hourglass.ColorAggregationNet().to(dev)
        with torch.no_grad():
            cnn_input, _ = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
        p = {k: v.detach().cpu().numpy() for k, v in net.cnn.state_dict().items()}
        xin = cnn_input.cpu().numpy()
        # (for the record: a rendered frame is smooth, its pool windows' gaps small -- this case is not searched for decidedness as the seeded ones are)
        print("end to end: decided in the sense of tests/test_hourglass_train_host.py: %s" % bref.decided(xin, p, host.forward_yardsticks(xin, p)[1]))
        sd_front = {k: getattr(net.front_end, k) for k in ("w1", "b1", "w2", "b2")}
        sd_cnn = {k: getattr(net.cnn, k) for k in NAMES}
        want, _ = _torch_tail(pkg, sd_front, sd_cnn, up, 1.0, torch.float64)
        t32, _ = _torch_tail(pkg, sd_front, sd_cnn, up, 1.0, torch.float32)
        chain = bref.backward_chain_f32(xin, p, ref.chain_f32(xin, p), None, up.cpu().numpy(), 1.0)          # the CNN's tensors have the second yardstick too
        # burned_in_gauss = 1 (iter_count >= burn_end): everything receives a gradient
        out = hourglass.fuse_color_train(pkg, net, 3, iter_count=20, burn_start=0, burn_end=10)
        assert sorted(out) == ["burned_in_gauss", "image_pred", "nb_valid_warp_level", "residual", "valid_warp_mask", "warped_image_list"] and out["burned_in_gauss"] == 1.0
        with torch.no_grad():
            test_time = hourglass.fuse_color(pkg, net, 3, burned_in_gauss=1.0)
        assert torch.equal(out["image_pred"], test_time["image_pred"]) and torch.equal(out["residual"], test_time["residual"])
        (out["image_pred"] * up).sum().backward()
        failed = []
        for k in list(sd_cnn) + list(sd_front) + ["render"]:
            got = pkg["render"].grad if k == "render" else (sd_cnn.get(k) if k in sd_cnn else sd_front[k]).grad
            assert got is not None, k
            w64 = torch.as_tensor(want[k], dtype=torch.float64, device=dev)
            err, d = float((got.double() - w64).abs().max()), float(np.abs(t32[k].astype(np.float64) - want[k]).max())
            if k in sd_cnn:
                d = max(d, float(np.abs(chain[k].astype(np.float64) - want[k]).max()))
            print("end to end %-16s err %.3e  d_ref %.3e  max|f64| %.3e  ratio %s" % (k, err, d, float(w64.abs().max()), "%.2f" % (err / d) if d > 0 else "-"))
            if not (err <= F64_K * d if d > 0 else err <= FLOOR * float(w64.abs().max())):
                failed.append((k, err, d))
        assert not failed, failed
        assert pkg["warped_image"].grad is not None and bool(torch.isfinite(pkg["warped_image"].grad).all())
        # during the burn-in nothing reaches render_pkg's tensors, and the parameters still train
        for t in list(net.parameters()) + [pkg["render"], pkg["warped_image"]]:
            t.grad = None
        out = hourglass.fuse_color_train(pkg, net, 3, iter_count=5, burn_start=0, burn_end=10)
        assert out["burned_in_gauss"] == 0.75
        (out["image_pred"] * up).sum().backward()
        assert pkg["render"].grad is None and pkg["warped_image"].grad is None and all(q.grad is not None and bool(q.grad.abs().sum() > 0) for q in net.parameters())
        # every source slot zeroed: nothing raises
        empty = dict(pkg, warped_image=torch.zeros_like(pkg["warped_image"]))
        none = hourglass.fuse_color_train(empty, net, 3)
        assert int(none["nb_valid_warp_level"]) == 0 and hourglass.fuse_color_train(empty, net, 3, none_if_no_level=True) is None
        (none["image_pred"] * up).sum().backward()
    finally:
        renderer.clear_caches()
