"""The fused colour aggregation front end (ibgs_amd.coloragg; csrc/coloragg.hip) on the device.

The ARBITER is tests/coloragg_ref.forward_ref / backward_ref (float64 numpy).  The YARDSTICK d_ref of a tensor is the max-abs distance from the arbiter of
tests/coloragg_ref.torch_composition at float32 on the same device inputs (forward, and torch's own backward of it).  THE BAR, as in
tests/test_gpu_geoloss.py and test_gpu_ssim.py::_grad_bar: max |hip - f64| <= F64_K x d_ref (F64_K = 2); where d_ref is exactly 0: 2^-22 max |f64|.  Every
comparison prints its ratio before it asserts (DESIGN.md section 14 quotes the range).  Bit-for-bit properties are asserted with torch.equal.

The mask of a slot is the float32 sum ((f0 + f1) + f2) + f3 > 0 in all three, so inputs may hold sums that round to exactly zero."""
import functools
import os
import time

import numpy as np
import pytest
import torch

from ibgs_amd import coloragg
from tests import coloragg_ref as ref

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
CHUNK = 128          # pixels of one workgroup's step (csrc/coloragg.hip: CHUNK; tests/test_coloragg_host.py checks the constant)
FRAMES = [(1, 1), (3, 5), (16, 24), (17, 67), (1, CHUNK + 1), (CHUNK + 1, 1)]
NAMES = ("render", "warped", "w1", "b1", "w2", "b2")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coloragg.npz")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _params(seed=3):
    """nn.Linear's initialisation range, seeded.  Shared: nobody writes them."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, fan: ((torch.rand(shape, generator=g) * 2 - 1) / fan ** 0.5)
    return tuple(t.cuda() for t in (u((32, 7), 7), u((32,), 7), u((32, 32), 32), u((32,), 32)))


@functools.lru_cache(maxsize=None)
def _case(s, h, w, live=None, seed=0):
    """-> render (3, H, W), warped (S, 3, H, W), feat (S, 4, H, W), ray (3, H, W), upstream (1, 38, H, W) on the device.  Slots from `live` on are zero.
    About 55 % of the slots of a pixel are valid; of the rest half are all-zero (as the rasterizer writes an invalid slot), a quarter have a negative sum and
    a quarter a sum that rounds to exactly 0 in float32 although it is positive.  Shared: nobody writes them."""
    live = s if live is None else live
    g = torch.Generator().manual_seed(seed * 7919 + 131 * s + 17 * h + w + 3 * live)
    render = torch.rand(3, h, w, generator=g)
    warped = (render[None] + 0.15 * torch.randn(s, 3, h, w, generator=g)).clamp(0, 1)
    warped[live:] = 0
    f = torch.randn(s, 4, h, w, generator=g) * 0.2 + 0.5
    f[:, 0][f.sum(1) < 0.3] += 1.0
    kind = torch.rand(s, 1, h, w, generator=g)
    feat = torch.where(kind < 0.55, f, torch.zeros(()))
    feat = torch.where((kind >= 0.775) & (kind < 0.8875), -f, feat)
    cancel = torch.tensor([1.0, 2.0 ** -30, -1.0, 0.0]).view(1, 4, 1, 1).expand(s, 4, h, w)          # (1 + 2^-30) rounds to 1: the float32 sum is 0, the exact one is not
    feat = torch.where(kind >= 0.8875, cancel, feat)
    ray = torch.nn.functional.normalize(torch.randn(3, h, w, generator=g), dim=0)
    up = torch.randn(1, 38, h, w, generator=g)
    return tuple(t.float().cuda().contiguous() for t in (render, warped, feat, ray, up))


# ---- the three evaluations ---------------------------------------------------------------------------------------------------------------------------
def _fused(render, warped, feat, ray, up, params, nb, mode, levels=None, which=NAMES):
    """-> (out, levels tensor, {name: gradient or None})."""
    leaves = dict(zip(NAMES, [t.detach().clone().requires_grad_(n in which) for n, t in zip(NAMES, (render, warped) + tuple(params))]))
    out, lv = coloragg.per_view_features(leaves["render"], leaves["warped"], feat, ray, leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], nb, mode, levels)
    assert out.shape == (1, 38) + tuple(render.shape[1:]) and out.dtype == torch.float32 and lv.dtype == torch.int32 and lv.dim() == 0 and lv.is_cuda
    grads = torch.autograd.grad((out * up).sum(), [leaves[n] for n in which], allow_unused=True) if which else ()
    got = dict.fromkeys(NAMES)
    got.update(zip(which, grads))
    return out.detach(), lv, got


def _arbiter(render, warped, feat, ray, up, params, nb, mode, levels=None):
    out, cache = ref.forward_ref(render, warped, feat, ray, *params, nb_visible_src_frames=nb, mode=mode, levels=levels)
    return out, ref.backward_ref(cache, up), cache["levels"]


def _yardstick(render, warped, feat, ray, up, params, nb, mode, levels=None):
    leaves = [t.detach().clone().requires_grad_(True) for t in (render, warped) + tuple(params)]
    out = ref.torch_composition(leaves[0], leaves[1], feat, ray, *leaves[2:], nb_visible_src_frames=nb, mode=mode, dtype=torch.float32, levels=levels)
    grads = torch.autograd.grad((out * up).sum(), leaves, allow_unused=True)
    return out.detach(), {n: (torch.zeros_like(l) if g is None else g) for n, l, g in zip(NAMES, leaves, grads)}


def _check(name, got, want64, yard):
    want = torch.as_tensor(np.asarray(want64), dtype=torch.float64, device=got.device).reshape(got.shape)
    assert got.dtype == torch.float32
    err = float((got.double() - want).abs().max())
    d = float((yard.double().reshape(got.shape) - want).abs().max())
    print("%-64s err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= F64_K * d, (name, err, d)
    else:
        assert err <= FLOOR * float(want.abs().max()), (name, err)
    return err, d


def _parity(name, case, nb, mode, levels=None, params=None):
    params = _params() if params is None else params
    out, lv, g = _fused(*case, params, nb, mode, levels)
    out64, g64, lv64 = _arbiter(*case, params, nb, mode, levels)
    out32, g32 = _yardstick(*case, params, nb, mode, levels)
    assert int(lv) == lv64, (name, int(lv), lv64)
    _check(name + " out", out, out64, out32)
    assert torch.equal(out[0, 32:35], case[3]) and torch.equal(out[0, 35:], case[0])          # the ray and the colour pass through
    for n in NAMES:
        _check(name + " d" + n, g[n], g64[n], g32[n])
    if lv64 < case[1].shape[0]:
        assert float(g["warped"][lv64:].abs().max()) == 0.0
    return out, g


# ---- 1. frames, sources, levels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda s: "x".join(map(str, s)))
def test_frames(frame, mode):
    _parity("%dx%d S3 %s" % (frame + (mode,)), _case(3, *frame), 3, mode)


@pytest.mark.parametrize("nb", [1, 3, 5])
@pytest.mark.parametrize("s", [1, 3, 5])
def test_source_counts(s, nb):
    case = _case(s, 5, 7)
    _parity("5x7 S%d nb%d mean" % (s, nb), case, nb, "mean")
    _parity("5x7 S%d nb%d max" % (s, nb), case, nb, "max")


@pytest.mark.parametrize("live", [0, 1, 2, 3, 5])
def test_levels_counted_on_the_device_and_given(live):
    """Trailing slots zeroed: the device count finds `live`; the same number passed as an int gives the same bits."""
    case = _case(5, 9, 11, live)
    for mode in ("mean", "max"):
        out, g = _parity("9x11 S5 live %d %s" % (live, mode), case, 5, mode)
        out_i, lv_i, g_i = _fused(*case, _params(), 5, mode, levels=live)
        assert int(lv_i) == live and torch.equal(out, out_i) and all(torch.equal(g[n], g_i[n]) for n in NAMES)
        if live == 0:          # exact zeros, and the colour's gradient is the upstream's own planes
            assert float(out[0, :32].abs().max()) == 0.0 and float(g["warped"].abs().max()) == 0.0 and torch.equal(g["render"], case[4][0, 35:])
            assert all(float(g[n].abs().max()) == 0.0 for n in NAMES[2:])
    # a level the caller caps: the first two slots of three live ones
    _parity("9x11 S5 live 3 levels=2", _case(5, 9, 11, 3), 5, "mean", levels=2)
    # a middle slot zeroed: the count is 4, and the FIRST four slots are used (the zeroed one among them), as in the reference
    render, warped, feat, ray, up = _case(5, 9, 11)
    holed = warped.clone()
    holed[1] = 0
    assert int(_fused(render, holed, feat, ray, up, _params(), 5, "mean", which=())[1]) == 4
    _parity("9x11 S5 slot 1 zeroed", (render, holed, feat, ray, up), 5, "mean")


# ---- 2. masks, layouts ---------------------------------------------------------------------------------------------------------------------------------
def test_slot_masks_layouts_and_memory():
    render, warped, feat, ray, up = case = _case(3, 17, 67)
    v = torch.as_tensor(ref.valid_ref(feat))
    f = feat.cpu()
    zero, neg = (f == 0).all(1), f.double().sum(1) < -0.1
    cancel = (f.double().sum(1) > 0) & ~v          # positive in exact arithmetic, exactly 0 as the float32 sum
    assert bool(zero.any()) and bool(neg.any()) and bool(cancel.any()) and bool(v.any()) and not bool((v & (zero | neg)).any())
    out, g = _parity("17x67 masks", case, 3, "mean")
    # an invalid slot takes no colour gradient and gives none to the rendered colour -- but it is not skipped: its features still reach the output
    assert float(g["warped"][~v.cuda()[:, None].expand_as(g["warped"])].abs().max()) == 0.0
    out_nofeat, _, _ = _fused(render, warped, torch.where(v.cuda()[:, None], feat, torch.zeros(())), ray, up, _params(), 3, "mean", which=())
    assert not torch.equal(out, out_nofeat)
    # both layouts, and inputs that are not contiguous: the same bits
    p = _params()
    flat = (render, warped.reshape(9, 17, 67), feat.reshape(12, 17, 67), ray, up)
    strided = (render.permute(1, 2, 0).contiguous().permute(2, 0, 1), warped.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2),
               torch.stack([feat, feat], -1)[..., 0], ray, up)
    assert not strided[0].is_contiguous() and not strided[1].is_contiguous() and not strided[2].is_contiguous()
    wide = tuple(torch.stack([t, t], -1)[..., 0] for t in p)
    for other, params in ((flat, p), (strided, p), (case, wide)):
        o, _, go = _fused(*other, params, 3, "mean")
        assert torch.equal(o, out) and all(torch.equal(go[n].reshape(g[n].shape), g[n]) for n in NAMES)
    assert g["warped"].shape == warped.shape and _fused(*flat, p, 3, "mean")[2]["warped"].shape == (9, 17, 67)


# ---- 3. the maximum ------------------------------------------------------------------------------------------------------------------------------------
def test_max_ties_go_to_the_first_slot():
    render, warped, feat, ray, up = _case(3, 9, 11)
    w1, b1, w2, b2 = _params()
    # half of the channels die in every slot (a bias far below anything the layer can add): the slots tie at 0 there
    dead = b2.clone()
    dead[::2] = -50.0
    params = (w1, b1, w2, dead)
    out, g = _parity("9x11 max, channels tied at 0", (render, warped, feat, ray, up), 3, "max", params=params)
    assert float(out[0, 0:32:2].abs().max()) == 0.0 and float(g["w2"][::2].abs().max()) == 0.0 and float(g["b2"][::2].abs().max()) == 0.0
    # slot 1 a copy of slot 0: every channel's maximum is attained by slot 0 first, slot 1 gets nothing
    twin_w, twin_f = warped.clone(), feat.clone()
    twin_w[1], twin_f[1] = warped[0], feat[0]
    case = (render, twin_w, twin_f, ray, up)
    out, g = _parity("9x11 max, slot 1 a copy of slot 0", case, 3, "max")          # (torch may hand a tie to another slot: its distance from the arbiter is then the tie's)
    assert float(g["warped"][1].abs().max()) == 0.0 and float(g["warped"][0].abs().max()) > 0.0


# ---- 4. which gradients -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_parameter_gradients_only_no_grad_and_bits(mode):
    case = _case(3, 17, 67)
    out, _, g = _fused(*case, _params(), 3, mode)
    # the reference's burn-in: render and warped_image detached
    out_p, _, g_p = _fused(*case, _params(), 3, mode, which=NAMES[2:])
    assert torch.equal(out, out_p) and g_p["render"] is None and g_p["warped"] is None
    assert all(torch.equal(g[n], g_p[n]) for n in NAMES[2:])
    # the other way round: frozen parameters
    _, _, g_i = _fused(*case, _params(), 3, mode, which=NAMES[:2])
    assert all(torch.equal(g[n], g_i[n]) for n in NAMES[:2]) and all(g_i[n] is None for n in NAMES[2:])
    # a second run: the same bits, outputs and every gradient
    out2, _, g2 = _fused(*case, _params(), 3, mode)
    assert torch.equal(out, out2) and all(torch.equal(g[n], g2[n]) for n in NAMES)
    with torch.no_grad():
        o, lv = coloragg.per_view_features(case[0], case[1], case[2], case[3], *_params(), 3, mode)
    assert torch.equal(o, out) and not o.requires_grad and int(lv) == 3


# ---- 4b. frames beyond the capped grids: the workgroups walk several chunks ------------------------------------------------------------------------------
BWD_GROUPS, FWD_GROUPS = 512, 4096          # csrc/coloragg.hip: CAGG_MAX_GROUPS, CAGG_FWD_MAX_GROUPS (tests/test_coloragg_host.py checks the constants)


def _rows(case, r0, r1):
    return tuple(t[..., r0:r1, :].contiguous() for t in case)


def test_frames_larger_than_the_grids_equal_their_pieces():
    """Per pixel the kernels do the same arithmetic wherever the pixel lies, so a frame a workgroup walks in several steps gives, bit for bit, what its row
    blocks give as frames of their own (each small enough for one step per workgroup).  With rows of CHUNK pixels every chunk of the whole is a chunk of a
    piece: each chunk's f32 chain of dW2 is the same, everything behind it is f64, and the parameter gradients differ only by the final roundings to
    float32 -- one per piece and one of the whole: |whole - sum pieces| <= 2^-24 (sum |piece| + |whole|), with 2^-40 of that for the f64 orders.
    (A frame of this size against float64 under the bar would be a coin toss: among 10^7 pre-activations one is close enough to 0 for some float32
    evaluation to take the other branch of the ReLU, and the gradient is not continuous there.)"""
    w = CHUNK
    h = BWD_GROUPS + 8                                # 520 rows = 520 chunks > 512 workgroups
    case = _case(2, h, w)
    out, _, g = _fused(*case, _params(), 2, "mean")
    total = {n: torch.zeros_like(g[n], dtype=torch.float64) for n in NAMES[2:]}
    mag = {n: g[n].double().abs() for n in NAMES[2:]}
    for r0 in range(0, h, 130):
        o, _, gp = _fused(*_rows(case, r0, r0 + 130), _params(), 2, "mean")
        assert torch.equal(o, out[..., r0:r0 + 130, :]) and torch.equal(gp["render"], g["render"][..., r0:r0 + 130, :])
        assert torch.equal(gp["warped"], g["warped"][..., r0:r0 + 130, :])
        for n in NAMES[2:]:
            total[n] += gp[n].double()
            mag[n] += gp[n].double().abs()
    for n in NAMES[2:]:
        excess = float(((g[n].double() - total[n]).abs() - 2.0 ** -24 * (1 + 2.0 ** -16) * mag[n]).max())
        print("520x128 whole against four pieces d%-3s max |d| %.3e of max %.3e" % (n, float((g[n].double() - total[n]).abs().max()), float(total[n].abs().max())))
        assert excess <= 0.0, (n, excess)
    # the forward's grid: FWD_GROUPS workgroups of CHUNK pixels
    h = FWD_GROUPS + 4
    case = _case(1, h, w)
    with torch.no_grad():
        whole = coloragg.per_view_features(*case[:4], *_params(), 1, "max")[0]
        for r0 in range(0, h, 1025):
            piece = coloragg.per_view_features(*[t[..., r0:r0 + 1025, :].contiguous() for t in case[:4]], *_params(), 1, "max")[0]
            assert torch.equal(piece, whole[..., r0:r0 + 1025, :]), r0


# ---- 5. the fixture: what the reference's own network received and returned ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_reference_fixture(mode):
    z = np.load(GOLDEN)
    dev = lambda a: torch.as_tensor(a).float().cuda().contiguous()
    render, warped, feat, ray, up = dev(z["in_color"]), dev(z["in_warped_image"]), dev(z["in_cam_feat"]), dev(z["in_camera_ray"]), dev(z["upstream"])
    params = tuple(dev(z[n]) for n in ("w1", "b1", "w2", "b2"))
    front = coloragg.PerViewFrontEnd(mode).cuda()
    front.load_state_dict({"per_view_mlp.0.weight": params[0], "per_view_mlp.0.bias": params[1], "per_view_mlp.2.weight": params[2], "per_view_mlp.2.bias": params[3]})
    pkg = {"render": render.clone().requires_grad_(True), "warped_image": warped.clone().requires_grad_(True), "cam_feat": feat, "camera_ray": ray,
           "min_depth_diff": dev(z["in_min_depth_diff"])}
    out, mask = coloragg.fuse_color_inputs(pkg, front, 3)
    assert torch.equal(mask.cpu(), torch.as_tensor(z[mode + "_valid_warp_mask"]))
    grads = torch.autograd.grad((out * up).sum(), [pkg["render"], pkg["warped_image"], front.w1, front.b1, front.w2, front.b2])
    out64, g64, lv = _arbiter(render, warped, feat, ray, up, params, 3, mode)
    out32, g32 = _yardstick(render, warped, feat, ray, up, params, 3, mode)
    assert lv == 3
    # the bar of every other case: the float32 torch composition on this device.  The reference's own float32 run on the CPU, as recorded, is printed beside
    # it (its distance from the arbiter), not used.  Every tensor is printed before the first failure is raised.
    failed = []
    pairs = [("out", out.detach(), out64, out32, z[mode + "_cnn_input"])]
    pairs += [("d" + n, got, g64[n], g32[n], z[mode + "_grad_" + key]) for n, got, key in zip(NAMES, grads, ("render", "warped_image", "w1", "b1", "w2", "b2"))]
    for name, got, want, mine, theirs in pairs:
        want_t = torch.as_tensor(np.asarray(want), dtype=torch.float64).cuda().reshape(got.shape)
        print("fixture %s %-8s the reference's recorded float32 run is %.3e from float64" % (mode, name, float((dev(theirs).double().reshape(got.shape) - want_t).abs().max())))
        try:
            _check("fixture %s %s" % (mode, name), got, want, mine)
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]
    assert coloragg.fuse_color_inputs(pkg, front, 3, none_if_no_level=True) is not None
    pkg["warped_image"] = torch.zeros_like(warped)
    assert coloragg.fuse_color_inputs(pkg, front, 3, none_if_no_level=True) is None and coloragg.fuse_color_inputs(pkg, front, 3) is not None


# ---- 6. streams and the host ---------------------------------------------------------------------------------------------------------------------------
def test_side_stream_gives_the_same_bits_and_the_forward_never_waits():
    case = _case(5, 17, 67, 3)
    want = [_fused(*case, _params(), 5, mode) for mode in ("mean", "max")]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = [_fused(*case, _params(), 5, mode) for mode in ("mean", "max")]
    s.synchronize()
    for (o0, l0, g0), (o1, l1, g1) in zip(want, got):
        assert torch.equal(o0, o1) and int(l0) == int(l1) == 3 and all(torch.equal(g0[n], g1[n]) for n in NAMES)
    # the forward behind a queue of other work: it returns while that work is still running, i.e. it waited for nothing -- not even for its level count
    a = torch.rand(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    start, queued, done = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    start.record()
    for _ in range(40):
        a = (a @ a).clamp_(0, 1)
    queued.record()
    t0 = time.perf_counter()
    with torch.no_grad():
        out, lv = coloragg.per_view_features(case[0], case[1], case[2], case[3], *_params(), 5, "mean")
    host_ms = (time.perf_counter() - t0) * 1e3
    still_running = not queued.query()
    done.record()
    torch.cuda.synchronize()
    print("forward: host %.3f ms; the queue in front of it %.3f ms on the device, its own kernels %.3f ms" % (host_ms, start.elapsed_time(queued), queued.elapsed_time(done)))
    assert still_running, "per_view_features returned only after the work queued in front of it had finished: something in it waits for the device"
    assert host_ms < start.elapsed_time(queued)
    assert torch.equal(out, want[0][0]) and int(lv) == 3


# ---- 7. end to end: through the rasterizer's backward ---------------------------------------------------------------------------------------------------
def test_end_to_end_gaussian_gradients():
    """render() -> fuse_color_inputs -> a seeded sum -> backward at the consumer scene's size.  The rasterizer's backward is linear in the two image gradients
    it is handed, so the bar carries through it: the same backward is run from the fused front end's image gradients, from the float32 torch composition's
    and from the float64 composition's (rounded to float32), and each Gaussian gradient of the first is within F64_K x the second's distance from the third."""
    from ibgs_amd import rasterizer, renderer, simple_scene, synthetic as syn
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
    front = coloragg.PerViewFrontEnd().to(dev)
    with torch.no_grad():
        for n, p in zip(("w1", "b1", "w2", "b2"), _params()):
            getattr(front, n).copy_(p)
    up = torch.randn(1, 38, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    old = rasterizer.DETERMINISTIC
    try:
        rasterizer.DETERMINISTIC = True
        renderer.clear_caches()
        with torch.no_grad():
            for j in cam.nearest_id:
                scn.rendered_depth_list[j] = renderer.render_depth(cams[j], pc, scn, pipe, args, torch.zeros(3, device=dev), True, 3, 4)
        pkg = renderer.render(cam, pc, scn, pipe, args, torch.zeros(3, device=dev), learnt_normal=True, nb_src_frames=3, buffer_length=4, render_geo=True)
        leaves = [p for p in pc.parameters() if p.requires_grad]
        cnn_input, mask = coloragg.fuse_color_inputs(pkg, front, 3)
        assert cnn_input.shape == (1, 38, H, W) and mask.shape[-2:] == (H, W)
        fused = torch.autograd.grad((cnn_input * up).sum(), leaves, retain_graph=True, allow_unused=True)

        def image_grads(dtype):
            r, x = pkg["render"].detach().clone().requires_grad_(True), pkg["warped_image"].detach().clone().requires_grad_(True)
            out = ref.torch_composition(r, x, pkg["cam_feat"].detach(), pkg["camera_ray"].detach().view(3, H, W), front.w1.detach(), front.b1.detach(), front.w2.detach(),
                                        front.b2.detach(), 3, "mean", dtype)
            return [t.float() for t in torch.autograd.grad((out * up.to(dtype)).sum(), [r, x])]
        through = lambda gs: torch.autograd.grad([pkg["render"], pkg["warped_image"]], leaves, grad_outputs=gs, retain_graph=True, allow_unused=True)
        yard, arbiter = through(image_grads(torch.float32)), through(image_grads(torch.float64))
    finally:
        rasterizer.DETERMINISTIC = old
        renderer.clear_caches()
    live = 0
    for i, (a, b, c) in enumerate(zip(fused, yard, arbiter)):
        assert (a is None) == (c is None)
        if a is None or float(c.abs().max()) == 0.0:
            continue
        live += 1
        _check("end to end, Gaussian parameter %d %s" % (i, tuple(a.shape)), a, c.double().cpu().numpy(), b)
    assert live >= 4
