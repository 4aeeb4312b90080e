"""Half-precision training of the hourglass CNN (ibgs_amd.hourglass `hourglass_backward`, `hourglass_train` with precision="float16", `fuse_color_train` and
resample_train.fuse_color_train_scaled inside `train_precision("float16")`; csrc/hghtrain.hip) on the device.

The ARBITER is tests/hghalf_bwd_ref.backward_decided: float64 numpy on the unrounded float32 parameters and the float64 forward's values, with all eight ReLU
decision sets and the pools' routing HANDED to it (a preactivation within binary16's reach of zero occurs in every frame: no input exists on which float64
and binary16 take the same decisions).  The YARDSTICK is torch's own CPU autocast(float16) forward and backward with the loss scaled by the same 2^k:
per tensor d_ref = max |autocast - arbiter(on autocast's own decisions)|, err = max |hip - arbiter(on the device's own decisions)|.  THE BAR is the project's
(F64_K = 2, DESIGN.md sections 12-19): err <= 2 d_ref; where d_ref is exactly 0: 2^-22 max |f64|.  Every ratio is printed before the first miss is raised
(DESIGN.md section 15 quotes the ranges).  Bit-for-bit properties are asserted with torch.equal."""
import functools
import time

import numpy as np
import pytest
import torch

from ibgs_amd import _device, _lib, coloragg, hourglass, resample, resample_train
from tests import hghalf_bwd_ref as hbref
from tests import hourglass_bwd_ref as bref
from tests import hourglass_ref as ref
from tests import test_gpu_hourglass as fwd
from tests import test_hourglass_train_host as host

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
FRAMES = host.FRAMES + [f for f in host.wgrad_frames() if f not in host.FRAMES]
NAMES = [k for k in bref.GRADS if k != "x"]
HALF = dict(precision="float16")


def _dev(a):
    return None if a is None else torch.as_tensor(a).cuda()


def _k_of(g_res, g_ip):
    g = (0 if g_res is None else g_res) + (0 if g_ip is None else g_ip)
    return hbref.scale_k(np.abs(np.asarray(g, dtype=np.float32)).max())


def _yardstick(x, p, want_stages, g_res, g_ip, burned):
    """-> (k, {tensor: d_ref}): torch's autocast backward against the arbiter on autocast's own decisions."""
    k = _k_of(g_res, g_ip)
    auto, dec, pool = hbref.autocast_backward(x, p, g_res, g_ip, burned, k)
    want = hbref.backward_decided(x, p, want_stages, dec, pool, g_res, g_ip, burned)
    return k, {n: float(np.abs(auto[n].astype(np.float64) - want[n]).max()) for n in bref.GRADS}


@functools.lru_cache(maxsize=None)
def _case(h, w, kind, upstream="both", burned=0.75, magnitude=1.0):
    """Computed once and shared; nobody writes it."""
    seed = host.decided_seed(h, w, kind)
    p = fwd._params(kind)
    x = ref.seeded_input(seed, h, w)
    g = np.random.default_rng(seed + 7)
    g_res, g_ip = (np.float32(magnitude) * g.standard_normal((3, h, w))).astype(np.float32), (np.float32(magnitude) * g.standard_normal((3, h, w))).astype(np.float32)
    if upstream == "residual":
        g_ip = None
    if upstream == "image_pred":
        g_res = None
    stages64 = ref.forward_ref(x, p)
    k, d_ref = _yardstick(x, p, stages64, g_res, g_ip, burned)
    return dict(x=x, p=p, kind=kind, g_res=g_res, g_ip=g_ip, stages64=stages64, k=k, d_ref=d_ref, burned=burned)


def _device_arbiter(c, stages, decisions):
    """The arbiter on the device's own decisions: the six binary16 stages (device tensors) and the planes (d1 > 0, f > 0) the backward returned."""
    host_stages = {n: v.float().cpu().numpy() for n, v in stages.items()}
    dec = {n: v > 0 for n, v in host_stages.items()}
    dec["d1"], dec["f"] = decisions[0].cpu().numpy(), decisions[1].cpu().numpy()
    return hbref.backward_decided(c["x"], c["p"], c["stages64"], dec, host_stages, c["g_res"], c["g_ip"], c["burned"])


def _compare(tag, got, want, d_ref, failed=None):
    collect = failed is not None
    failed = failed if collect else []
    for n in bref.GRADS:
        w64 = torch.as_tensor(want[n], dtype=torch.float64, device="cuda")
        t = got[n].reshape(w64.shape)
        assert t.dtype == torch.float32, (tag, n)
        err, d = float((t.double() - w64).abs().max()), d_ref[n]
        print("%-44s err %.3e  d_ref %.3e  max|f64| %.3e  ratio %s" % (tag + " " + n, err, d, float(w64.abs().max()), "%.2f" % (err / d) if d > 0 else "-"))
        ok = err <= F64_K * d if d > 0 else err <= FLOOR * float(w64.abs().max())
        if not ok:
            failed.append((tag, n, err, d))
    assert collect or not failed, failed


def _forward_stages(x, net):
    with torch.no_grad():
        _, stages = hourglass.hourglass_forward(x, net, return_stages=True, **HALF)
        return {n: v.clone() for n, v in stages.items()}


def _raw(c, net, **kw):
    x = _dev(c["x"])
    stages = _forward_stages(x, net)
    out = hourglass.hourglass_backward(x, net, stages, _dev(c["g_res"]), _dev(c["g_ip"]), render_scale=c["burned"], return_decisions=True, **HALF, **kw)
    return out, stages


def _autograd(c, retain=False, **kw):
    net = hourglass.HourglassCNN()
    net.load_state_dict({k: torch.tensor(v) for k, v in c["p"].items()})
    net = net.cuda()
    x = _dev(c["x"]).requires_grad_(True)
    residual, image_pred = hourglass.hourglass_train(x, net, render_scale=c["burned"], **HALF, **kw)
    outs = [o for o, g in ((residual, c["g_res"]), (image_pred, c["g_ip"])) if g is not None]
    ups = [_dev(g) for g in (c["g_res"], c["g_ip"]) if g is not None]
    grads = torch.autograd.grad(outs, [x] + [getattr(net, k) for k in NAMES], ups, retain_graph=retain)
    return dict(zip(["x"] + NAMES, grads)), (x, net, residual, image_pred)


def _both_paths(tag, c, failed=None):
    status = torch.full((2,), -99, dtype=torch.int32, device="cuda")
    (gx, gp, decisions), stages = _raw(c, fwd._net(c["kind"]), status=status)
    torch.cuda.synchronize()
    h, w = c["x"].shape[-2:]
    assert tuple(gx.shape) == (38, h, w) and sorted(gp) == sorted(NAMES)
    assert decisions[0].dtype == torch.bool and tuple(decisions[0].shape) == (38, h, w) == tuple(decisions[1].shape)
    assert status.tolist() == [c["k"], 0], (status.tolist(), c["k"])          # the automatic rule is tests/hghalf_bwd_ref.scale_k's; nothing overflowed
    want = _device_arbiter(c, stages, decisions)
    _compare(tag + " raw", dict(gp, x=gx), want, c["d_ref"], failed)
    got, _ = _autograd(c)          # ... and through autograd: the same forward kernel wrote the stages, so the same decisions
    assert tuple(got["x"].shape) == (1, 38, h, w)
    _compare(tag + " autograd", got, want, c["d_ref"], failed)
    return gx, gp, got


# ---- 1. frames x parameter sets --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", host.KINDS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_gradients_against_float64(h, w, kind):
    """All 19 tensors, the raw call and autograd, automatic scale.  The measured min - max (mean) of err / d_ref per tensor: DESIGN.md section 15."""
    c = _case(h, w, kind)
    failed = []
    gx, gp, got = _both_paths("%dx%d %s" % (h, w, kind), c, failed)
    assert torch.equal(gx, got["x"][0]) and all(torch.equal(gp[n], got[n]) for n in NAMES)
    assert not failed, failed


# ---- 2. one upstream, burned 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream,burned", [("residual", 0.75), ("image_pred", 0.75), ("both", 1.0)])
def test_one_upstream_and_burned_one(upstream, burned):
    _both_paths("16x24 %s %.2f" % (upstream, burned), _case(16, 24, "default", upstream, burned))


# ---- 3. exact ------------------------------------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    h, w = 17, 67
    c = _case(h, w, "default")
    frozen = fwd._net("default")
    got, (x, net, residual, image_pred) = _autograd(c, retain=True)
    xd = x.detach()
    with torch.no_grad():
        r0, ip0 = hourglass.hourglass_forward(xd, frozen, render_scale=0.75, **HALF)
        plain = hourglass.hourglass_forward(xd, frozen, **HALF)
    assert torch.equal(residual, r0) and torch.equal(image_pred, ip0) and residual.requires_grad and image_pred.requires_grad
    lone = hourglass.hourglass_train(x, net, **HALF)
    assert torch.is_tensor(lone) and torch.equal(lone, plain)
    arena = [t for t in residual.grad_fn.saved_tensors if t.dtype == torch.uint8]
    assert len(arena) == 1 and arena[0].numel() == _lib.load().ibgs_hgh_required_scratch(h, w)
    arena = arena[0]
    arena0, x0, p0 = arena.clone(), xd.clone(), [q.detach().clone() for q in net.parameters()]
    g_res, g_ip = _dev(c["g_res"]), _dev(c["g_ip"])
    g0 = (g_res.clone(), g_ip.clone())
    call = lambda xin=xd, a=g_res, b=g_ip, **kw: hourglass.hourglass_backward(xin, net, arena, a, b, render_scale=0.75, **HALF, **kw)
    same = lambda a, b, gx, gp: torch.equal(a, gx) and all(torch.equal(b[n], gp[n]) for n in NAMES)
    gx, gp = call()
    assert same(gx, gp, got["x"][0], got)          # autograd's gradients are hourglass_backward's on the arena the node saved
    assert same(*call(), gx, gp)                   # a second call
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gx3, gp3 = call()
    s.synchronize()
    assert same(gx3, gp3, gx, gp)                  # a side stream
    wide = torch.zeros(1, 38, h, 2 * w + 1, device="cuda")
    wide[..., ::2][..., :w] = xd
    views = {"(38, H, W)": xd[0], "every other column": wide[..., ::2][..., :w], "channels last": xd.contiguous(memory_format=torch.channels_last), "float64": xd.double()}
    for what, v in views.items():
        gv = g_res.double() if what == "float64" else g_res.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert same(*call(v, gv), gx, gp), what
    only_x, none = call(need_param_grads=False)
    none2, only_p = call(need_input_grad=False)
    assert none is None and none2 is None and torch.equal(only_x, gx) and all(torch.equal(only_p[n], gp[n]) for n in NAMES)
    # a dict of the stages is packed into the same layout
    a, b = hourglass.hourglass_backward(xd, net, hourglass._arena_views(arena, h, w, True), g_res, g_ip, render_scale=0.75, **HALF)
    assert same(a, b, gx, gp)
    torch.cuda.synchronize()
    assert torch.equal(arena, arena0) and torch.equal(xd, x0) and all(torch.equal(q, q0) for q, q0 in zip(net.parameters(), p0))
    assert torch.equal(g_res, g0[0]) and torch.equal(g_ip, g0[1])
    # the recomputed d1 and f are the forward's (the head's loop restates hgh_conv3_kernel's): `final` applied to the backward arena's f, in float64 on the rounded
    # operands, is the forward's residual to within a float32 accumulation of 39 terms (64 x 2^-24 of the sum of magnitudes); one binary16 ulp of one f is 2^-11 of it
    flat = [getattr(net, layer + s).detach().contiguous() for layer, _, _, _ in hourglass.LAYERS for s in ("_w", "_b")]
    sc = hourglass._backward_call_half(xd.device, h, w, xd[0].contiguous(), flat, 0.75, arena, g_res, g_ip, True, False, None, None)[2]
    d1h, fh = hourglass._head_stages(sc, h, w)
    wf, bf = net.final_w.detach()[:, :, 0, 0].half().double(), net.final_b.detach().half().double()
    again = torch.einsum("oc,chw->ohw", wf, fh.double()) + bf[:, None, None]
    reach = 64 * 2.0 ** -24 * (torch.einsum("oc,chw->ohw", wf.abs(), fh.double().abs()) + bf.abs()[:, None, None])
    assert bool(((again - residual.detach().double()).abs() <= reach).all()) and float(fh.max()) > 0 and float(d1h.max()) > 0 and float(reach.max()) < 2.0 ** -17
    # precision="float32" is the call without the keyword
    with torch.no_grad():
        _, _, st32 = hourglass.hourglass_forward(xd, frozen, render_scale=0.75, return_stages=True)
        st32 = {n: v.clone() for n, v in st32.items()}
    a32, b32 = hourglass.hourglass_backward(xd, net, st32, g_res, g_ip, render_scale=0.75)
    c32, d32 = hourglass.hourglass_backward(xd, net, st32, g_res, g_ip, render_scale=0.75, precision="float32")
    assert same(c32, d32, a32, b32)
    xa, xb = xd.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    ra, rb = hourglass.hourglass_train(xa, net, render_scale=0.75), hourglass.hourglass_train(xb, net, render_scale=0.75, precision="float32")
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    (ga,), (gb,) = torch.autograd.grad(ra[1], xa, g_ip), torch.autograd.grad(rb[1], xb, g_ip)
    assert torch.equal(ga, gb) and not torch.equal(ga[0], gx)
    # inside train_precision("float16") hourglass_train is the call with the keyword; the keyword overrides the block; outside it nothing is left of it
    xc, xe = xd.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    with hourglass.train_precision("float16"):
        rc = hourglass.hourglass_train(xc, net, render_scale=0.75)
        re_ = hourglass.hourglass_train(xe, net, render_scale=0.75, precision="float32")
    assert torch.equal(rc[0], residual) and torch.equal(rc[1], image_pred) and torch.equal(re_[0], ra[0])
    (gc,) = torch.autograd.grad([rc[0], rc[1]], xc, [g_res, g_ip])
    assert torch.equal(gc, got["x"]) and torch.equal(hourglass.hourglass_train(xd, net), hourglass.hourglass_train(xd, net, precision="float32"))
    # an upstream scaled by a power of two, automatic mode: every output scaled by exactly that factor, k moved the other way
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    call(status=st)
    k0 = int(st[0])
    assert k0 == c["k"]
    for e in (5, -7):
        factor = 2.0 ** e
        sx, sp = call(a=g_res * factor, b=g_ip * factor, status=st)
        assert st.tolist() == [k0 - e, 0], (e, st.tolist())
        assert torch.equal(sx, gx * factor) and all(torch.equal(sp[n], gp[n] * factor) for n in NAMES), e


# ---- 4. the scale does its job ---------------------------------------------------------------------------------------------------------------------------------
def test_the_scale_does_its_job():
    h, w = 16, 24
    tiny = _case(h, w, "default", "both", 0.75, 1e-9)
    assert tiny["k"] > 30
    gx, gp, _ = _both_paths("16x24 upstream 1e-9", tiny)          # the bar of test 1, automatic mode
    assert all(float(gp[n].abs().max()) > 0 for n in NAMES)
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    (zx, zp, _), _ = _raw(tiny, fwd._net("default"), grad_scale_log2=0, status=st)          # unscaled, the upstream rounds to binary16 zeros
    assert st.tolist() == [0, 0] and all(bool((zp[n] == 0).all()) for n in NAMES)
    assert bool((zx[:35] == 0).all()) and torch.equal(zx[35:], 0.75 * _dev(tiny["g_ip"]))          # what is left of grad_x is the float32, unscaled burned-in term
    unit = _case(h, w, "default")
    (ox, op, _), _ = _raw(unit, fwd._net("default"), grad_scale_log2=20, status=st)          # 2^20 times an upstream of magnitude 1 overflows binary16: reported, not hidden
    torch.cuda.synchronize()
    assert int(st[0]) == 20 and int(st[1]) > 0
    assert not bool(torch.isfinite(ox).all()) and not bool(torch.isfinite(op["final_w"]).all()) and not bool(torch.isfinite(op["enc1_w"]).all())


# ---- 5. uninitialised arenas -----------------------------------------------------------------------------------------------------------------------------------
def test_arenas_of_0xff_through_the_c_abi():
    h, w = 17, 67
    c = _case(h, w, "default")
    net = fwd._net("default")
    x, g_res, g_ip = _dev(c["x"])[0].contiguous(), _dev(c["g_res"]), _dev(c["g_ip"])
    lib = _lib.load()
    fwd_arena = torch.full((lib.ibgs_hgh_required_scratch(h, w),), 0xFF, dtype=torch.uint8, device="cuda")
    sc = torch.full((lib.ibgs_hgh_train_required_scratch(h, w),), 0xFF, dtype=torch.uint8, device="cuda")
    assert bool(torch.isnan(sc[:4096].view(torch.float16)).all()) and bool(torch.isnan(sc[:4096].view(torch.float32)).all())
    flat = [getattr(net, layer + s).detach().contiguous() for layer, _, _, _ in hourglass.LAYERS for s in ("_w", "_b")]
    r, ip = torch.full((3, h, w), float("nan"), device="cuda"), torch.full((3, h, w), float("nan"), device="cuda")
    dev = x.device
    _device.call(dev, "ibgs_hgh_forward", h, w, x.data_ptr(), *[t.data_ptr() for t in flat], 0.75, r.data_ptr(), ip.data_ptr(), fwd_arena.data_ptr(), fwd_arena.numel())
    gx = torch.full((38, h, w), float("nan"), device="cuda")
    grads = [torch.full_like(t, float("nan")) for t in flat]
    st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    _device.call(dev, "ibgs_hgh_train_backward", h, w, x.data_ptr(), *[t.data_ptr() for t in flat], 0.75, fwd_arena.data_ptr(), g_res.data_ptr(), g_ip.data_ptr(),
                 _lib.HGHT_SCALE_AUTO, 0, st.data_ptr(), gx.data_ptr(), *[t.data_ptr() for t in grads], sc.data_ptr(), sc.numel())
    torch.cuda.synchronize()
    stages = _forward_stages(_dev(c["x"]), net)
    wx, wp = hourglass.hourglass_backward(_dev(c["x"]), net, stages, g_res, g_ip, render_scale=0.75, **HALF)
    assert torch.equal(gx, wx) and all(torch.equal(g, wp[n]) for g, n in zip(grads, NAMES))
    assert not bool(torch.isnan(gx).any()) and not any(bool(torch.isnan(g).any()) for g in grads) and st.tolist() == [c["k"], 0]


# ---- 6. end to end: the rasterizer's outputs in, gradients out ---------------------------------------------------------------------------------------------
def _cnn_bar(tag, net, xin, arena, g_res, g_ip, burned, got):
    """The CNN's eighteen gradients of an end-to-end run against the arbiter on the device's decisions, with the bar of test 1."""
    p = {k: v.detach().cpu().numpy() for k, v in net.cnn.state_dict().items()}
    x = xin.detach().cpu().numpy()
    h, w = x.shape[-2:]
    npy = lambda t: None if t is None else t.detach().cpu().numpy()
    stages64 = ref.forward_ref(x, p)
    _, d_ref = _yardstick(x, p, stages64, npy(g_res), npy(g_ip), burned)
    _, _, decisions = hourglass.hourglass_backward(xin.detach(), net.cnn, arena, g_res, g_ip, render_scale=burned, return_decisions=True, **HALF)
    c = dict(x=x, p=p, stages64=stages64, g_res=npy(g_res), g_ip=npy(g_ip), burned=burned)
    want = _device_arbiter(c, hourglass._arena_views(arena, h, w, True), decisions)
    failed = []
    for n in NAMES:
        w64 = torch.as_tensor(want[n], dtype=torch.float64, device="cuda")
        err, d = float((got[n].double() - w64).abs().max()), d_ref[n]
        print("%-36s err %.3e  d_ref %.3e  max|f64| %.3e  ratio %s" % (tag + " " + n, err, d, float(w64.abs().max()), "%.2f" % (err / d) if d > 0 else "-"))
        if not (err <= F64_K * d if d > 0 else err <= FLOOR * float(w64.abs().max())):
            failed.append((n, err, d))
    assert not failed, failed


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
        front = [net.front_end.w1, net.front_end.b1, net.front_end.w2, net.front_end.b2]

        def reached(tag):
            for q in list(net.cnn.parameters()) + front + [pkg["render"], pkg["warped_image"]]:
                assert q.grad is not None and bool(torch.isfinite(q.grad).all()), tag
            assert all(float(q.grad.abs().max()) > 0 for q in list(net.cnn.parameters()) + front + [pkg["render"]]), tag
            got = {n: getattr(net.cnn, n).grad.clone() for n in NAMES}
            for q in list(net.parameters()) + [pkg["render"], pkg["warped_image"]]:
                q.grad = None
            return got

        # full resolution, burned_in_gauss = 1: everything receives a gradient
        with hourglass.train_precision("float16"):
            out = hourglass.fuse_color_train(pkg, net, 3, iter_count=20, burn_start=0, burn_end=10)
        assert out["burned_in_gauss"] == 1.0          # (the graph keeps its precision: its backward runs outside the block)
        with torch.no_grad():
            test_time = hourglass.fuse_color(pkg, net, 3, burned_in_gauss=1.0, **HALF)
            cnn_input, _ = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
        assert torch.equal(out["image_pred"], test_time["image_pred"]) and torch.equal(out["residual"], test_time["residual"])
        arena = [t for t in out["image_pred"].grad_fn.saved_tensors if t.dtype == torch.uint8][0]
        (out["image_pred"] * up).sum().backward()
        _cnn_bar("48x32", net, cnn_input, arena, None, up, 1.0, reached("full resolution"))

        # residual_resolution_scale 0.5: the public call against its pieces, whose low-resolution upstream the arbiter is handed
        with hourglass.train_precision("float16"):
            out = resample_train.fuse_color_train_scaled(pkg, net, 0.5, 3, iter_count=20, burn_start=0, burn_end=10)
        (out["image_pred"] * up).sum().backward()
        got = reached("scaled")
        reduced = resample.scaled_size(H, W, 0.5)
        levels = resample.count_levels(pkg["warped_image"], 3)
        fe = net.front_end
        x_lr = resample_train.resized_features_train(pkg["render"], pkg["warped_image"], pkg["cam_feat"], hourglass._ray_planes(pkg["camera_ray"], H, W), fe.w1, fe.b1, fe.w2, fe.b2,
                                                     reduced, levels, fe.mode)
        r_lr = hourglass.hourglass_train(x_lr, net.cnn, **HALF)
        _, ip = resample_train.upsample_residual_train(r_lr, pkg["render"], 1.0)
        assert torch.equal(ip, out["image_pred"])
        arena = [t for t in r_lr.grad_fn.saved_tensors if t.dtype == torch.uint8][0]
        (g_lr,) = torch.autograd.grad((ip * up).sum(), r_lr, retain_graph=True)
        (ip * up).sum().backward()
        mine = reached("scaled, from its pieces")
        assert all(torch.equal(mine[n], got[n]) for n in NAMES)
        _cnn_bar("24x16 (s = 0.5)", net, x_lr, arena, g_lr.reshape(3, *reduced), None, 1.0, got)
    finally:
        renderer.clear_caches()


# ---- 7. the call never waits -------------------------------------------------------------------------------------------------------------------------------
def test_the_backward_never_waits():
    c = _case(17, 67, "default")
    net = fwd._net("default")
    x, g_res, g_ip = _dev(c["x"]), _dev(c["g_res"]), _dev(c["g_ip"])
    stages = _forward_stages(x, net)
    want = hourglass.hourglass_backward(x, net, stages, g_res, g_ip, render_scale=0.75, **HALF)
    a = torch.rand(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    start, queued, done = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    start.record()
    for _ in range(40):
        a = (a @ a).clamp_(0, 1)
    queued.record()
    t0 = time.perf_counter()
    got = hourglass.hourglass_backward(x, net, stages, g_res, g_ip, render_scale=0.75, **HALF)          # automatic scale: the reduction's k stays on the device
    host_ms = (time.perf_counter() - t0) * 1e3
    still_running = not queued.query()
    done.record()
    torch.cuda.synchronize()
    print("backward: host %.3f ms; the queue in front of it %.3f ms on the device, its own kernels %.3f ms" % (host_ms, start.elapsed_time(queued), queued.elapsed_time(done)))
    assert still_running, "hourglass_backward returned only after the work queued in front of it had finished: something in it waits for the device"
    assert host_ms < start.elapsed_time(queued)
    assert torch.equal(got[0], want[0]) and all(torch.equal(got[1][k], want[1][k]) for k in NAMES)
