"""The fused geometry loss terms (ibgs_amd.losses.photometric_loss / normal_consistency; csrc/geoloss.hip) on the device.

The ARBITER is tests/geoloss_ref at float64 with the "shift2d" window.  The YARDSTICK d_ref of a quantity is the larger max-abs distance from the arbiter of
the whole expression at float32 in the "conv2d" form (inside ssim_ref.torch_own_conv(), forward and backward) and in the "separable" form, as
tests/test_gpu_ssim.py::_grad_bar does.  THE BAR: gradient max |hip - f64| <= F64_K x d_ref (F64_K = 2); value |hip - f64| <= F64_K x photo_weight x
(w_s d_map + (1 - w_s) 2^-22) with d_map the yardstick of the channel-mean map of (gt, masked) -- a weighted mean of bounded errors cannot exceed their
maximum.  Where d_ref is exactly 0: 2^-22 max |g64|.  For the normal term the yardstick is the float32 torch expression of train.py:310-315.  Every
comparison prints its ratio before it asserts (DESIGN.md section 13 has the table).

Every input keeps |sum f| > 2^-20 sum |f| in every feature slot (geoloss_ref.assert_decided, on the CPU, when the input is made): the reference's torch.sum
and the kernels' ((f0 + f1) + f2) + f3 then decide `valid` alike.  Bit-for-bit properties are asserted with torch.equal."""
import functools

import pytest
import torch

from ibgs_amd import losses
from tests import geoloss_ref as ref
from tests import ssim_ref

pytestmark = pytest.mark.gpu

T_H, T_W = losses.geoloss_tile()
FRAMES = [(1, 1), (1, 23), (23, 1), (11, 11), (T_H + 1, T_W + 1), (2 * T_H - 1, 2 * T_W + 5), (40, 70)]
SOURCES = [(4, 3), (2, 3), (1, 3), (5, 5)]          # (S_total, nb_visible_src_frames)
KINDS = ["near", "all_valid", "unclamped", "smooth"]
WEIGHTS = [(0.3, 1.0), (0.3, 0.0), (0.7, 0.35)]          # (photo_weight, photo_ssim_weight)
FLOOR = 2.0 ** -22


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def _features(mask, g):
    """(S, 4, H, W) for a (S, 1, H, W) bool mask: signed features whose sum is >= 0.3 where valid; elsewhere zeros, as the rasterizer writes an invalid slot,
    and in a quarter of those slots signed features whose sum is <= -0.3."""
    shape = (mask.shape[0], 4) + tuple(mask.shape[2:])
    f = torch.randn(shape, generator=g) * 0.2 + 0.5
    low = f.sum(1) < 0.3
    f[:, 0][low] += 1.0
    neg = (torch.rand(mask.shape, generator=g) < 0.25) & ~mask
    feat = torch.where(mask, f, torch.where(neg, -f, torch.zeros(())))
    ref.assert_decided(feat)
    assert bool(((((feat[:, 0] + feat[:, 1]) + feat[:, 2]) + feat[:, 3] > 0) == mask[:, 0]).all()) and bool(((feat.sum(1) > 0) == mask[:, 0]).all())
    return feat


@functools.lru_cache(maxsize=None)
def _case(kind, st, h, w, seed=0):
    """-> gt (3, H, W), warped (S_total, 3, H, W), feat (S_total, 4, H, W), mask (S_total, 1, H, W) bool, on the device.  Shared: nobody writes them."""
    g = torch.Generator().manual_seed(seed * 7919 + 131 * st + 17 * h + w + len(kind))
    gt = torch.rand(3, h, w, generator=g)
    mask = torch.rand(st, 1, h, w, generator=g) < 0.4
    if kind == "near":
        warped = (gt[None] + 0.08 * torch.randn(st, 3, h, w, generator=g)).clamp(0, 1)
    elif kind == "all_valid":
        warped = (gt[None] + 0.08 * torch.randn(st, 3, h, w, generator=g)).clamp(0, 1)
        mask = torch.ones_like(mask)
    elif kind == "unclamped":          # what an unclamped render can produce: [-0.3, 1.4]
        warped = torch.rand(st, 3, h, w, generator=g) * 1.7 - 0.3
    elif kind == "smooth":          # the ramp of tests/test_gpu_ssim.py: s1 = p - u^2 cancels and the bar follows d_ref
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        ramp = 0.5 + 0.4 * torch.sin(0.11 * xx + 0.07 * yy)
        gt = ramp.expand(3, h, w) + 0.01 * torch.randn(3, h, w, generator=g)
        warped = ramp.expand(st, 3, h, w) + 0.01 * torch.randn(st, 3, h, w, generator=g)
    else:
        raise ValueError(kind)
    feat = _features(mask, g)
    return gt.float().cuda().contiguous(), warped.float().cuda().contiguous(), feat.float().cuda().contiguous(), mask.cuda()


def _layout(warped, feat, flat):
    if not flat:
        return warped, feat
    return warped.reshape((-1,) + tuple(warped.shape[-2:])), feat.reshape((-1,) + tuple(feat.shape[-2:]))


# ---- the arbiter and the yardsticks ------------------------------------------------------------------------------------------------------------------
def _bars(gt, warped, feat, nb, pw, ws):
    """-> (l64, g64, d_grad, d_map) of the term at these arguments; warped: (S_total, 3, H, W)."""
    def of(dtype, form):
        leaf = warped.detach().to(dtype).requires_grad_(True)
        with ssim_ref.torch_own_conv():          # (forward and backward: tests/ssim_ref.py, "conv2d")
            loss = ref.photometric_ref(gt, leaf, feat, nb, pw, ws, dtype, form)
            g, = torch.autograd.grad(loss, leaf)
            m = ref.mean_map_ref(gt, warped, feat, nb, dtype, form)
        return loss.detach().double(), g.double(), m.double()
    l64, g64, m64 = of(torch.float64, "shift2d")
    d_grad = d_map = 0.0
    for form in ("conv2d", "separable"):
        _, g, m = of(torch.float32, form)
        d_grad = max(d_grad, float((g - g64).abs().max()))
        d_map = max(d_map, float((m - m64).abs().max()))
    return l64, g64, d_grad, d_map


def _check_grad(name, got, g64, d):
    assert got.shape == g64.shape and got.dtype == torch.float32
    err = float((got.double() - g64).abs().max())
    print("%-58s grad  err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= ssim_ref.F64_K * d, (name, err, d)
    else:
        assert float(got.abs().max()) == 0.0 or err <= FLOOR * float(g64.abs().max()), (name, err)


def _check_value(name, got, l64, pw, ws, d_map):
    assert got.shape == () and got.dtype == torch.float32
    bar = ssim_ref.F64_K * pw * (ws * d_map + (1 - ws) * FLOOR)
    err = abs(float(got.detach().double()) - float(l64))
    print("%-58s value err %.3e  bar %.3e  ratio %s" % (name, err, bar, "%.2f" % (err / bar) if bar > 0 else "-"))
    assert err <= bar, (name, err, bar)


def _fused(gt, warped, feat, nb, pw, ws):
    x = warped.detach().clone().requires_grad_(True)
    v = losses.photometric_loss(gt, x, feat, nb, pw, ws)
    g, = torch.autograd.grad(v, x)
    assert g.shape == warped.shape
    return v.detach(), g


def _parity(name, kind, frame, sources, weights, flat):
    st, nb = sources
    gt, warped, feat, mask = _case(kind, st, *frame)
    l64, g64, d_grad, d_map = _bars(gt, warped, feat, nb, *weights)
    w_in, f_in = _layout(warped, feat, flat)
    v, g = _fused(gt, w_in, f_in, nb, *weights)
    _check_value(name, v, l64, weights[0], weights[1], d_map)
    _check_grad(name, g.reshape(warped.shape), g64, d_grad)
    s = min(st, nb)
    g = g.reshape(warped.shape)
    assert float(g[s:].abs().max()) == 0.0 if s < st else True
    if not bool(mask[:s].all()):
        assert float(g[:s][~mask[:s].expand_as(g[:s])].abs().max()) == 0.0


# ---- 1. value and gradient against the arbiter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda s: "x".join(map(str, s)))
def test_arbiter_parity(frame, kind):
    """Every frame with every content; the source counts, weight pairs and layouts go round with them (each combination of those three: the next test)."""
    i = FRAMES.index(frame) + KINDS.index(kind)
    sources, weights, flat = SOURCES[i % 4], WEIGHTS[i % 3], bool(i % 2)
    _parity("%s %s S%d/%d w%s %s" % ("x".join(map(str, frame)), kind, sources[1], sources[0], weights, "3-D" if flat else "4-D"), kind, frame, sources, weights, flat)


@pytest.mark.parametrize("flat", [False, True], ids=["4-D", "3-D"])
@pytest.mark.parametrize("weights", WEIGHTS, ids=str)
@pytest.mark.parametrize("sources", SOURCES, ids=lambda s: "S%d_of_%d" % (s[1], s[0]))
def test_sources_weights_and_layouts(sources, weights, flat):
    frame = (T_H + 1, T_W + 1)
    _parity("%dx%d near S%d/%d w%s %s" % (frame + (sources[1], sources[0], weights, "3-D" if flat else "4-D")), "near", frame, sources, weights, flat)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weights", WEIGHTS, ids=str)
def test_weights_with_every_content(weights, kind):
    _parity("40x70 %s S3/4 w%s" % (kind, weights), kind, (40, 70), (4, 3), weights, False)


# ---- 2. exact properties -----------------------------------------------------------------------------------------------------------------------------
def test_no_valid_pixel_is_zero_without_asking_the_host():
    gt, warped, feat, _ = _case("near", 4, T_H + 1, T_W + 1)
    for empty in (torch.zeros_like(feat), -feat.abs()):
        for weights in WEIGHTS:
            v, g = _fused(gt, warped, empty, 3, *weights)
            assert float(v) == 0.0 and float(g.abs().max()) == 0.0 and not bool(torch.isnan(g).any())
    # the same bits on a non-blocking side stream, for an empty and a non-empty mask: nothing in the call depends on the host seeing Nv
    want = [_fused(gt, warped, f, 3, 0.3, 1.0) for f in (torch.zeros_like(feat), feat)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = [_fused(gt, warped, f, 3, 0.3, 1.0) for f in (torch.zeros_like(feat), feat)]
    s.synchronize()
    for (v0, g0), (v1, g1) in zip(want, got):
        assert torch.equal(v0, v1) and torch.equal(g0, g1)


@pytest.mark.parametrize("weights", WEIGHTS, ids=str)
def test_single_valid_pixels_at_a_corner_and_a_seam(weights):
    h, w = T_H + 8, 2 * T_W + 3
    gt, warped, _, _ = _case("near", 2, h, w)
    warped = warped.clone()
    spots = [(0, 0, 0), (0, h - 1, w - 1), (1, T_H - 1, T_W), (1, T_H, T_W - 1)]          # (source, row, column): two frame corners, both sides of both seams
    feat = torch.zeros(2, 4, h, w, device="cuda")
    for s, r, c in spots:
        feat[s, :, r, c] = torch.tensor([0.9, -0.2, 0.3, 0.1], device="cuda")
        warped[s, :, r, c] = (gt[:, r, c] + torch.tensor([0.2, -0.15, 0.1], device="cuda"))
    ref.assert_decided(feat)
    v, g = _fused(gt, warped, feat, 3, *weights)
    hit = torch.zeros_like(g, dtype=torch.bool)
    for s, r, c in spots:
        hit[s, :, r, c] = True
    assert float(g[~hit].abs().max()) == 0.0 and float(g[hit].abs().min()) > 0.0 and float(v) > 0.0
    l64, g64, d_grad, d_map = _bars(gt, warped, feat, 3, *weights)
    _check_value("four valid pixels w%s" % (weights,), v, l64, weights[0], weights[1], d_map)
    _check_grad("four valid pixels w%s" % (weights,), g, g64, d_grad)


@pytest.mark.parametrize("weights", WEIGHTS, ids=str)
def test_warped_equal_to_gt_where_valid_is_exactly_zero(weights):
    gt, warped, feat, mask = _case("near", 4, 2 * T_H - 1, 2 * T_W + 5)
    same = torch.where(mask.expand_as(warped), gt[None].expand_as(warped), warped)          # anything at the invalid pixels
    v, g = _fused(gt, same, feat, 3, *weights)
    assert float(v) == 0.0 and float(g.abs().max()) == 0.0


def test_unread_sources_are_never_read():
    gt, warped, feat, _ = _case("near", 4, T_H + 1, T_W + 1)
    for nb in (1, 3):
        v0, g0 = _fused(gt, warped, feat, nb, 0.7, 0.35)
        w_nan, f_nan = warped.clone(), feat.clone()
        w_nan[nb:] = float("nan")
        f_nan[nb:] = float("nan")
        v1, g1 = _fused(gt, w_nan, f_nan, nb, 0.7, 0.35)
        assert torch.equal(v0, v1) and torch.equal(g0, g1) and float(g1[nb:].abs().max()) == 0.0 and float(g1[:nb].abs().max()) > 0.0


def test_no_grad_second_backward_and_reproducible_bits():
    gt, warped, feat, _ = _case("near", 4, 2 * T_H - 1, 2 * T_W + 5)
    x = warped.clone().requires_grad_(True)
    v = losses.photometric_loss(gt, x, feat, 3, 0.7, 0.35)
    assert v.requires_grad
    g1, = torch.autograd.grad(v, x, retain_graph=True)
    g2, = torch.autograd.grad(v, x)
    assert torch.equal(g1, g2)
    with torch.no_grad():
        v0 = losses.photometric_loss(gt, x, feat, 3, 0.7, 0.35)
    assert torch.equal(v0, v.detach()) and not v0.requires_grad
    assert not losses.photometric_loss(gt, warped, feat, 3, 0.7, 0.35).requires_grad          # nothing to differentiate
    for _ in range(2):
        va, ga = _fused(gt, warped, feat, 3, 0.7, 0.35)
        assert torch.equal(va, v.detach()) and torch.equal(ga, g1)
    # an upstream factor: read on the device
    x2 = warped.clone().requires_grad_(True)
    (losses.photometric_loss(gt, x2, feat, 3, 0.7, 0.35) * 0.25).backward()
    l64, g64, d_grad, _ = _bars(gt, warped, feat, 3, 0.7, 0.35)
    _check_grad("0.25 x photometric", x2.grad, 0.25 * g64, 0.25 * d_grad)
    # cam_feat gets no gradient
    f = feat.clone().requires_grad_(True)
    x3 = warped.clone().requires_grad_(True)
    losses.photometric_loss(gt, x3, f, 3).backward()
    assert f.grad is None and x3.grad is not None
    with pytest.raises(ValueError, match="gt_image requires grad"):
        losses.photometric_loss(gt.clone().requires_grad_(True), warped, feat)


def test_a_source_does_not_see_the_others():
    gt, warped, feat, mask = _case("near", 4, T_H + 1, T_W + 1)
    v0, g0 = _fused(gt, warped, feat, 3, 0.7, 0.35)
    # one source's colours at its INVALID pixels only: nothing moves
    other = warped.clone()
    noise = torch.rand(other[1].shape, generator=torch.Generator().manual_seed(3)).cuda()
    other[1] = torch.where(mask[1].expand_as(other[1]), other[1], noise)
    assert not torch.equal(other, warped)
    v1, g1 = _fused(gt, other, feat, 3, 0.7, 0.35)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    # one source's colours at its valid pixels, masks fixed (so Nv is): the other sources' gradients keep their bits
    other = warped.clone()
    other[1] = noise
    v2, g2 = _fused(gt, other, feat, 3, 0.7, 0.35)
    assert torch.equal(g0[0], g2[0]) and torch.equal(g0[2], g2[2]) and not torch.equal(g0[1], g2[1]) and not torch.equal(v0, v2)


def _composed(gt, warped, feat, nb, pw, ws):
    """What a user composes on the fused map alone: tests/test_gpu_ssim.py::_photometric over losses.ssim_map plus the L1 line of train.py:332-333."""
    warped = warped[:nb]
    mask = (torch.sum(feat[:nb], dim=1, keepdim=True) > 0).float()
    masked = mask * warped + (1 - mask) * gt
    loss = 1 - torch.stack([losses.ssim_map(gt, masked[i]).mean(0) for i in range(len(masked))])
    ssim_term = torch.sum(loss * mask[:, 0]) / torch.sum(mask[:, 0])
    l1 = torch.sum(torch.abs(gt[None] - masked).mean(1) * mask[:, 0]) / torch.sum(mask[:, 0])
    return ((1 - ws) * l1 + ws * ssim_term) * pw


@pytest.mark.parametrize("weights", WEIGHTS, ids=str)
def test_fused_and_composed_agree(weights):
    gt, warped, feat, _ = _case("near", 4, 40, 70)
    l64, g64, d_grad, d_map = _bars(gt, warped, feat, 3, *weights)
    v, g = _fused(gt, warped, feat, 3, *weights)
    x = warped.clone().requires_grad_(True)
    vc = _composed(gt, x, feat, 3, *weights)
    gc, = torch.autograd.grad(vc, x)
    _check_value("fused against composed w%s" % (weights,), v, vc.detach().double(), weights[0], weights[1], d_map)
    _check_grad("fused against composed w%s" % (weights,), g, gc.double(), d_grad)
    _check_grad("composed against the arbiter w%s" % (weights,), gc, g64, d_grad)


# ---- 3. normal consistency ---------------------------------------------------------------------------------------------------------------------------
def _normals(kind, h, w, seed=0):
    g = torch.Generator().manual_seed(seed * 31 + 7 * h + w + len(kind))
    n, dn = torch.randn(3, h, w, generator=g), torch.randn(3, h, w, generator=g)
    if kind == "unit":
        n, dn = torch.nn.functional.normalize(n, dim=0), torch.nn.functional.normalize(dn, dim=0)
    elif kind == "same":
        n = 0.7 * n
        dn = n.clone()
    elif kind != "raw":
        raise ValueError(kind)
    return n.float().cuda().contiguous(), dn.float().cuda().contiguous()


def _normal_bars(n, dn, weight, factor=1.0):
    def of(dtype):
        a, b = n.detach().to(dtype).requires_grad_(True), dn.detach().to(dtype).requires_grad_(True)
        loss = ref.normal_ref(a, b, weight, dtype) * factor
        ga, gb = torch.autograd.grad(loss, [a, b])
        return loss.detach().double(), ga.double(), gb.double()
    l64, ga64, gb64 = of(torch.float64)
    l32, ga32, gb32 = of(torch.float32)
    return l64, (ga64, gb64), abs(float(l32 - l64)), (float((ga32 - ga64).abs().max()), float((gb32 - gb64).abs().max()))


def _check_normal_value(name, got, l64, d):
    assert got.shape == () and got.dtype == torch.float32
    err = abs(float(got.detach().double()) - float(l64))
    bar = ssim_ref.F64_K * d if d > 0 else FLOOR * abs(float(l64))
    print("%-58s value err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.2f" % (err / d) if d > 0 else "-"))
    assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("kind", ["unit", "raw", "same"])
@pytest.mark.parametrize("frame", [(1, 1), (5, 7), (40, 70), (9, 13)], ids=lambda s: "x".join(map(str, s)))
def test_normal_consistency_parity(frame, kind):
    h, w = frame
    n, dn = _normals(kind, h, w + 1 if frame == (9, 13) else w)
    if frame == (9, 13):          # a plane of 117 elements, no multiple of 4, seen through a view that starts 4 bytes off
        n, dn = n[:, :, 1:], dn[:, :, 1:]
        assert not n.is_contiguous() and n.data_ptr() % 16 == 4 and n.shape == (3, 9, 13)
    name = "normal %dx%d %s" % (h, w, kind)
    l64, g64, d_val, d_grad = _normal_bars(n, dn, 0.03)
    a, b = n.detach().clone().requires_grad_(True), dn.detach().clone().requires_grad_(True)
    if frame == (9, 13):
        a, b = n.detach().requires_grad_(True), dn.detach().requires_grad_(True)          # the views themselves
    v = losses.normal_consistency(a, b)
    ga, gb = torch.autograd.grad(v, [a, b])
    _check_normal_value(name, v, l64, d_val)
    _check_grad(name + " wrt normal", ga, g64[0], d_grad[0])
    _check_grad(name + " wrt depth normal", gb, g64[1], d_grad[1])
    if kind == "same":
        k = 0.03 / (h * w)
        # the L1 part's gradient is exactly 0 x sign: what is left is the f32 rounding of k (-0.6 other)
        assert torch.equal(ga, (k * (-0.6 * dn.double())).float()) and torch.equal(gb, (k * (-0.6 * n.double())).float())
        closed = 0.03 * 0.6 * float((1 - (n.double() ** 2).sum(0)).mean())
        _check_normal_value(name + " closed form", v, closed, d_val)


def test_normal_consistency_upstream_forms_and_bits():
    n, dn = _normals("unit", 40, 70, seed=2)
    l64, g64, d_val, d_grad = _normal_bars(n, dn, 0.05)
    runs = []
    for _ in range(2):
        a, b = n.clone().requires_grad_(True), dn.clone().requires_grad_(True)
        v = losses.normal_consistency(a, b, weight=0.05)
        ga, gb = torch.autograd.grad(v, [a, b], retain_graph=True)
        ga, gb = ga.clone(), gb.clone()
        ga2, gb2 = torch.autograd.grad(v, [a, b])          # a second backward through the same node gives the first's bits
        assert torch.equal(ga, ga2) and torch.equal(gb, gb2)
        runs.append((v.detach(), ga, gb))
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    _check_normal_value("normal weight 0.05", runs[0][0], l64, d_val)
    _check_grad("normal weight 0.05 wrt normal", runs[0][1], g64[0], d_grad[0])
    # the gradient into one input only
    a = n.clone().requires_grad_(True)
    v = losses.normal_consistency(a, dn, weight=0.05)
    assert torch.equal(torch.autograd.grad(v, a)[0], runs[0][1]) and torch.equal(v.detach(), runs[0][0])
    b = dn.clone().requires_grad_(True)
    v = losses.normal_consistency(n, b, weight=0.05)
    assert torch.equal(torch.autograd.grad(v, b)[0], runs[0][2])
    # an upstream factor other than 1
    l64q, g64q, _, d_gradq = _normal_bars(n, dn, 0.05, factor=0.25)
    a, b = n.clone().requires_grad_(True), dn.clone().requires_grad_(True)
    (0.25 * losses.normal_consistency(a, b, weight=0.05)).backward()
    _check_grad("0.25 x normal wrt normal", a.grad, g64q[0], d_gradq[0])
    _check_grad("0.25 x normal wrt depth normal", b.grad, g64q[1], d_gradq[1])
    assert torch.equal(a.grad, 0.25 * runs[0][1]) and torch.equal(b.grad, 0.25 * runs[0][2])
    # under no_grad: the grad-mode value, and nothing recorded
    with torch.no_grad():
        v0 = losses.normal_consistency(a, b, weight=0.05)
    assert torch.equal(v0, runs[0][0]) and not v0.requires_grad
    # on a side stream
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a2 = n.clone().requires_grad_(True)
        v2 = losses.normal_consistency(a2, dn, weight=0.05)
        g2, = torch.autograd.grad(v2, a2)
    s.synchronize()
    assert torch.equal(v2.detach(), runs[0][0]) and torch.equal(g2, runs[0][1])
