"""The exposure correction (ibgs_amd.exposure; csrc/exposure.hip) on the device.

The ARBITER is tests/exposure_ref (float64 numpy: numpy.linalg.lstsq on the masked pixels, the apply, the transposed apply).  The YARDSTICK d_ref of a tensor
is the max-abs distance from the arbiter of the reference's own formulation in float32 torch on the CPU (exposure_ref.yardstick: boolean gather, cat,
torch.linalg.lstsq with the driver the reference runs, einsum, autograd).  THE BAR, as in tests/test_gpu_coloragg.py: max |hip - f64| <= F64_K x d_ref
(F64_K = 2); where d_ref is exactly 0: 2^-22 max |f64|.  Every comparison prints its ratio before it asserts (DESIGN.md section 18 quotes the range).
Bit-for-bit properties are asserted with torch.equal."""
import functools
import os
import time

import numpy as np
import pytest
import torch

from ibgs_amd import _lib, coloragg, exposure, hourglass
from tests import exposure_ref as ref
from tests import scenes

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consumer.npz")
IDENTITY = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


def _large_frame():
    """A frame every workgroup of the moments kernel walks more than once, with the partial count at its cap: the cap is read off the arena's size, one
    sweep of the capped grid off the header's constants; two sweeps and a row."""
    cap = (_lib.load().ibgs_expo_required_scratch(_lib.EXPO_MAX_SIDE, _lib.EXPO_MAX_SIDE) - 128) // (8 * _lib.EXPO_SUMS)
    sweep = cap * _lib.EXPO_THREADS * _lib.EXPO_PIXELS_PER_THREAD
    w = 1024
    h = 2 * sweep // w + 1
    assert cap == _lib.EXPO_MAX_GROUPS and sweep % w == 0 and 2 * sweep < h * w < 600000
    assert _lib.load().ibgs_expo_required_scratch(h, w) == 128 + cap * 8 * _lib.EXPO_SUMS
    return h, w


FRAMES = [(1, 1), (4, 4), (5, 7), (33, 65), (32, 48), "large"]


def _dev(a):
    return torch.as_tensor(a).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _case(h, w, density, grey):
    """-> numpy inputs, the upstream gradient, the arbiter's and the yardstick's results (computed once; nobody writes them), and the device tensors."""
    render, warped, mask = ref.case(h, w, density, grey)
    up = np.random.default_rng(h * w + 5).standard_normal((3, h, w)).astype(np.float32)
    c64, a64, ok = ref.correct_ref(render, warped, mask)
    c32 = a32 = None
    if ok:
        c32, a32 = ref.yardstick(render, warped, mask)
    return dict(render=render, warped=warped, mask=mask, up=up, c64=c64, a64=a64, ok=ok, c32=c32, a32=a32, dev=tuple(_dev(t) for t in (render, warped, mask, up)))


def _run(render, warped, mask, up=None):
    """-> (corrected, affine, fit_ok, d render or None) from exposure_correct on device tensors."""
    r = render.detach().clone().requires_grad_(up is not None)
    c, a, ok = exposure.exposure_correct(r, warped, mask)
    assert c.shape == render.shape[-3:] and c.dtype == torch.float32 and a.shape == (3, 4) and a.dtype == torch.float32
    assert ok.dim() == 0 and ok.dtype == torch.int32 and ok.is_cuda and not a.requires_grad and not ok.requires_grad
    g = None
    if up is not None:
        g, = torch.autograd.grad((c * up).sum(), r)
    return c.detach(), a, ok, g


def _check(name, got, want64, yard):
    want = torch.as_tensor(np.asarray(want64), dtype=torch.float64).reshape(got.shape)
    got = got.detach().cpu()
    assert got.dtype == torch.float32
    err = float((got.double() - want).abs().max())
    d = float((torch.as_tensor(np.asarray(yard)).double().reshape(got.shape) - want).abs().max())
    print("%-64s err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.3f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= F64_K * d, (name, err, d)
    else:
        assert err <= FLOOR * float(want.abs().max()), (name, err)


def _gradient_check(name, affine, render, up, got):
    """d render: the float64 transposed apply WITH THE SAME float32 matrix is the arbiter, torch autograd through the float32 einsum the yardstick."""
    a = affine.detach().cpu()
    r = torch.tensor(render, requires_grad=True)
    out = torch.einsum("ij,jhw->ihw", a, torch.cat([r, torch.ones((1,) + r.shape[1:])], 0))
    g32, = torch.autograd.grad((out * torch.tensor(up)).sum(), r)
    _check(name + " d render", got, ref.apply_backward_ref(a.numpy(), up), g32.numpy())


def _undetermined(name, c, a, ok, g, render, up):
    assert int(ok) == 0, name
    assert torch.equal(a.cpu(), IDENTITY), name
    assert torch.equal(c.view(torch.int32), render.view(torch.int32)), name          # bit for bit, -0.0 and NaN included
    if g is not None:
        assert torch.equal(g.view(torch.int32), up.view(torch.int32)), name


# ---- 1. frames, masks, conditioning ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grey", [False, True], ids=["colourful", "near_grey"])
@pytest.mark.parametrize("density", [0.3, 1.0])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_frames(frame, density, grey):
    h, w = _large_frame() if frame == "large" else frame
    z = _case(h, w, density, grey)
    render, warped, mask, up = z["dev"]
    name = "%dx%d density %.1f %s" % (h, w, density, "grey" if grey else "colour")
    words = set(np.unique(z["mask"]).tolist())
    assert words <= {0, 1, 2} and (h * w < 100 or density == 1.0 or words == {0, 1, 2})
    c, a, ok, g = _run(render, warped, mask, up)
    n = int((z["mask"] == 1).sum())
    if not z["ok"]:
        assert n < 4, "the seeded cases are undetermined only for want of pixels"
        _undetermined(name, c, a, ok, g, render, up)
        return
    print("%s: %d pixels under the mask, cond(X) %.3g" % (name, n, ref.cond(z["render"], z["mask"])))
    assert int(ok) == 1
    _check(name + " affine", a, z["a64"], z["a32"])
    _check(name + " corrected", c, z["c64"], z["c32"])
    _gradient_check(name, a, z["render"], z["up"], g)


def test_reference_fixture():
    """The reference's own fuse_color with the correction on, as recorded: the device must lie at most twice as far from float64 as the recording does."""
    z = np.load(GOLDEN)
    h, w = int(z["H"]), int(z["W"])
    render, warped, mask = z["oracle_color"], z["oracle_warped_image"], z["oracle_use_first_src_frame_mask"]
    c64, a64, ok64 = ref.correct_ref(render, warped, mask)
    c, a, ok, _ = _run(_dev(render), _dev(warped), _dev(mask))
    assert ok64 and int(ok) == 1
    recorded = z["exposure_c_3dgs"].T.reshape(3, h, w)
    _check("fixture corrected (d_ref: the recording)", c, c64, recorded)
    feats = lambda img: scenes.fuse_color_inputs(img, z["oracle_cam_feat"], z["oracle_warped_image"], z["oracle_camera_ray"], nb_visible_src_frames=3)[0]
    _check("fixture features (d_ref: the recording)", torch.as_tensor(feats(c.cpu().numpy()).astype(np.float32)), feats(c64), z["exposure_x_views"])
    assert float((c.cpu() - torch.as_tensor(recorded)).abs().max()) <= 1e-6


# ---- 2. exact properties -----------------------------------------------------------------------------------------------------------------------------------
def test_second_run_side_stream_layouts_strides_and_alignment():
    z = _case(33, 65, 0.3, False)
    render, warped, mask, up = z["dev"]
    want = _run(render, warped, mask, up)
    same = lambda got: all(torch.equal(x, y) for x, y in zip(got, want))
    assert same(_run(render, warped, mask, up))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _run(render, warped, mask, up)
    s.synchronize()
    assert same(got)
    # both layouts of warped_image and of the mask; inputs that are not contiguous; float64 inputs holding the same values
    assert same(_run(render, warped.reshape(-1, 33, 65), mask[0], up))
    strided = render.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    wide = torch.stack([warped, warped], -1)[..., 0]
    assert not strided.is_contiguous() and not wide.is_contiguous()
    assert same(_run(strided, wide, torch.stack([mask, mask], -1)[..., 0], up))
    got = _run(render.double(), warped.double(), mask, up)
    assert got[3].dtype == torch.float64 and same(got[:3] + (got[3].float(),))
    # planes the 16-byte loads cannot take (an odd float offset into a larger buffer) give the bits of the planes they can: 32 x 48 is a multiple of 4
    z = _case(32, 48, 0.3, True)
    render, warped, mask, up = z["dev"]
    want = _run(render, warped, mask, up)
    shifted = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape)
    r1, w1, m1 = shifted(render), shifted(warped), shifted(mask)
    assert r1.data_ptr() % 16 == 4 and r1.is_contiguous() and torch.equal(r1, render)
    got = _run(r1, w1, m1, shifted(up))
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # no argument is written
    for t, a in zip(z["dev"], (z["render"], z["warped"], z["mask"], z["up"])):
        assert torch.equal(t.cpu(), torch.as_tensor(a))


def test_pixels_outside_the_mask_and_other_slots_do_not_reach_the_fit():
    z = _case(33, 65, 0.3, False)
    render, warped, mask, up = z["dev"]
    c, a, ok, _ = _run(render, warped, mask)
    out = (mask != 1)[0]
    assert bool((mask == 2).any()) and bool((mask == 0).any())
    for poison in (float("nan"), float("inf"), -7.5):
        r2, w2 = render.clone(), warped.clone()
        r2[:, out] = poison
        w2[0][:, out] = poison
        w2[1:] = float("nan")          # slots 1 and above are never read
        c2, a2, ok2, _ = _run(r2, w2, mask)
        assert int(ok2) == 1 and torch.equal(a2, a), poison
        assert torch.equal(c2[:, ~out], c[:, ~out]) and not torch.equal(c2[:, out], c[:, out])
    # a mask word of 2 does not count as 1: turning the 2s into 0s changes nothing
    assert all(torch.equal(x, y) for x, y in zip(_run(render, warped, torch.where(mask == 2, 0, mask).int())[:3], (c, a, ok)))
    # ... and the mask does matter
    assert not torch.equal(_run(render, warped, torch.ones_like(mask))[1], a)


def test_undetermined_fits_return_the_image_unchanged():
    z = _case(33, 65, 0.3, False)
    render, warped, mask, up = z["dev"]
    render = render.clone()
    render[0, 0, 0], render[1, 0, 1] = -0.0, float("nan")          # outside every mask below but the constant-colour one: "bit for bit" is about such values
    flat = lambda idx: torch.zeros(33 * 65, dtype=torch.int32).index_fill_(0, torch.tensor(idx), 1).view(1, 33, 65).cuda()
    constant = render.clone()
    constant[:, (mask == 1)[0]] = torch.tensor([0.3, 0.5, 0.7]).cuda()[:, None]
    black = render.clone()
    black[:, (mask == 1)[0]] = 0.0
    twin = render.clone()
    twin[2] = twin[0]
    m_safe = mask.clone()
    m_safe[0, 0, :2] = 0
    cases = [("empty mask", render, torch.zeros_like(mask)), ("mask of 0 and 2", render, torch.where(mask == 1, 2, mask).int()), ("3 pixels", render, flat([70, 700, 1500])),
             ("constant colour", constant, m_safe), ("black", black, m_safe), ("duplicated channel", twin, m_safe)]
    for name, r, m in cases:
        assert not ref.determined(np.nan_to_num(r.cpu().numpy()), m.cpu().numpy()), name
        c, a, ok, g = _run(r, warped, m, up)
        _undetermined(name, c, a, ok, g, r, up)
    # NaN under the mask: no fit either
    poisoned = render.clone()
    poisoned[1, 5, 5] = float("nan")
    m = mask.clone()
    m[0, 5, 5] = 1
    c, a, ok, g = _run(poisoned, warped, m, up)
    _undetermined("NaN under the mask", c, a, ok, g, poisoned, up)
    # 4 pixels in general position: determined, and the fit passes through the four warped colours
    four = flat([70, 700, 1500, 2001])
    rn, wn, mn = z["render"], z["warped"], four.cpu().numpy()
    assert ref.determined(rn, mn) and ref.cond(rn, mn) < 1e3
    c64, a64, _ = ref.correct_ref(rn, wn, mn)
    sel = mn[0] == 1
    assert np.abs(c64[:, sel] - wn[0][:, sel]).max() < 1e-12
    c32, a32 = ref.yardstick(rn, wn, mn)
    c, a, ok, _ = _run(z["dev"][0], warped, four)
    assert int(ok) == 1
    _check("4 pixels affine", a, a64, a32)
    _check("4 pixels corrected", c, c64, c32)
    _check("4 pixels: the four warped colours", c[:, four[0] == 1], wn[0][:, sel], c32[:, sel])


# ---- 3. the keyword of the fuse_color entry points -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _package():
    z = np.load(GOLDEN)
    pkg = {"render": _dev(z["oracle_color"]), "warped_image": _dev(z["oracle_warped_image"]), "cam_feat": _dev(z["oracle_cam_feat"]),
           "camera_ray": _dev(z["oracle_camera_ray"]), "min_depth_diff": _dev(z["oracle_min_depth_diff"]), "use_first_src_frame_mask": _dev(z["oracle_use_first_src_frame_mask"])}
    torch.manual_seed(11)
    return pkg, hourglass.ColorAggregationNet().cuda()


KEYS = ["burned_in_gauss", "image_pred", "nb_valid_warp_level", "residual", "valid_warp_mask", "warped_image_list"]


def _same_dict(a, b, extra):
    assert sorted(a) == sorted(KEYS + extra) and sorted(b) == KEYS
    for k in KEYS:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_keyword_equals_the_manual_composition():
    pkg, net = _package()
    extra = ["exposure_affine", "exposure_fit_ok"]
    with torch.no_grad():
        corrected, affine, ok = exposure.exposure_correct(pkg["render"], pkg["warped_image"], pkg["use_first_src_frame_mask"])
        manual = dict(pkg, render=corrected)
        assert int(ok) == 1 and not torch.equal(corrected, pkg["render"])
        for kw in (dict(), dict(precision="float16"), dict(burned_in_gauss=0.75, nb_visible_src_frames=2)):
            on = hourglass.fuse_color(pkg, net, enable_exposure_correction=True, **kw)
            _same_dict(on, hourglass.fuse_color(manual, net, **kw), extra)
            assert torch.equal(on["exposure_affine"], affine) and torch.equal(on["exposure_fit_ok"], ok)
            via_module = net(pkg, enable_exposure_correction=True, **kw)
            assert sorted(via_module) == sorted(on) and torch.equal(via_module["image_pred"], on["image_pred"])
        a, b = coloragg.fuse_color_inputs(pkg, net.front_end, 3, enable_exposure_correction=True), coloragg.fuse_color_inputs(manual, net.front_end, 3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0][0, 35:], corrected)
        # without the keyword: the call as it was -- the front end and the hourglass on the uncorrected image, and the six keys
        plain, off = hourglass.fuse_color(pkg, net), hourglass.fuse_color(pkg, net, enable_exposure_correction=False)
        _same_dict(plain, off, [])
        x, levels = net.front_end(pkg["render"], pkg["warped_image"], pkg["cam_feat"], pkg["camera_ray"], 3)
        residual, image_pred = hourglass.hourglass_forward(x, net.cnn, render_scale=1.0)
        assert torch.equal(plain["image_pred"], image_pred) and torch.equal(plain["residual"], residual) and not torch.equal(plain["image_pred"], on["image_pred"])
        c0, c1 = coloragg.fuse_color_inputs(pkg, net.front_end, 3), coloragg.fuse_color_inputs(pkg, net.front_end, 3, enable_exposure_correction=False)
        assert torch.equal(c0[0], x) and torch.equal(c1[0], x)
    for burn in (dict(), dict(iter_count=3, burn_start=0, burn_end=10)):
        on = hourglass.fuse_color_train(pkg, net, enable_exposure_correction=True, **burn)
        _same_dict(on, hourglass.fuse_color_train(manual, net, **burn), extra)
        assert torch.equal(on["exposure_affine"], affine) and on["burned_in_gauss"] == (0.65 if burn else 1.0)
        _same_dict(hourglass.fuse_color_train(pkg, net, **burn), hourglass.fuse_color_train(pkg, net, enable_exposure_correction=False, **burn), [])
    no_mask = {k: v for k, v in pkg.items() if k != "use_first_src_frame_mask"}
    with pytest.raises(KeyError, match="fuse_color_train: render_pkg lacks 'use_first_src_frame_mask'"):
        hourglass.fuse_color_train(no_mask, net, enable_exposure_correction=True)
    assert sorted(hourglass.fuse_color_train(no_mask, net)) == KEYS


def test_training_gradient_is_the_chain_of_the_pieces():
    pkg, net = _package()
    h, w = pkg["render"].shape[1:]
    up = torch.randn(3, h, w, generator=torch.Generator().manual_seed(9)).cuda()
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    r, x = leaf(pkg["render"]), leaf(pkg["warped_image"])
    whole = hourglass.fuse_color_train(dict(pkg, render=r, warped_image=x), net, enable_exposure_correction=True)
    g_r, g_x = torch.autograd.grad((whole["image_pred"] * up).sum(), [r, x])
    # the pieces: the correction alone, then the uncorrected entry point on its output as a leaf
    r2 = leaf(pkg["render"])
    corrected, affine, ok = exposure.exposure_correct(r2, pkg["warped_image"], pkg["use_first_src_frame_mask"])
    c, x2 = leaf(corrected), leaf(pkg["warped_image"])
    tail = hourglass.fuse_color_train(dict(pkg, render=c, warped_image=x2), net)
    assert torch.equal(tail["image_pred"], whole["image_pred"])
    g_c, g_x2 = torch.autograd.grad((tail["image_pred"] * up).sum(), [c, x2])
    g_r2, = torch.autograd.grad(corrected, r2, grad_outputs=g_c)
    assert torch.equal(g_r, g_r2) and float(g_r.abs().max()) > 0
    assert torch.equal(g_x, g_x2), "warped_image receives the front end's gradient only: the fit is a constant of the backward"
    _check("chain: d render through the correction", g_r, ref.apply_backward_ref(affine.cpu().numpy(), g_c.cpu().numpy()),
           torch.einsum("ij,ihw->jhw", affine[:, :3], g_c).cpu().numpy())
    # during the burn-in nothing reaches the rasterizer's tensors, with the correction or without
    r3, x3 = leaf(pkg["render"]), leaf(pkg["warped_image"])
    burn = hourglass.fuse_color_train(dict(pkg, render=r3, warped_image=x3), net, iter_count=3, burn_start=0, burn_end=10, enable_exposure_correction=True)
    grads = torch.autograd.grad((burn["image_pred"] * up).sum(), [r3, x3, net.front_end.w1, net.cnn.enc1_w], allow_unused=True)
    assert grads[0] is None and grads[1] is None and grads[2] is not None and grads[3] is not None


# ---- 4. the host ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_call_never_waits_for_the_device():
    z = _case(33, 65, 0.3, False)
    render, warped, mask, up = z["dev"]
    want = _run(render, warped, mask)
    a = torch.rand(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    start, queued, done = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    start.record()
    for _ in range(40):
        a = (a @ a).clamp_(0, 1)
    queued.record()
    t0 = time.perf_counter()
    with torch.no_grad():
        c, aff, ok = exposure.exposure_correct(render, warped, mask)
    host_ms = (time.perf_counter() - t0) * 1e3
    still_running = not queued.query()
    done.record()
    torch.cuda.synchronize()
    print("exposure_correct: host %.3f ms; the queue in front of it %.3f ms on the device, its own kernels %.3f ms" % (host_ms, start.elapsed_time(queued), queued.elapsed_time(done)))
    assert still_running, "exposure_correct returned only after the work queued in front of it had finished: something in it waits for the device"
    assert host_ms < start.elapsed_time(queued)
    assert torch.equal(c, want[0]) and torch.equal(aff, want[1]) and int(ok) == 1
