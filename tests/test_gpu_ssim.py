"""The fused SSIM (ibgs_amd.losses.ssim / ssim_map, ibgs_amd.image_eval; csrc/ssim.hip) on the device.

The ARBITER is tests/ssim_ref.ssim_map_ref at float64 (the reference's float32 2-D window, 121 shifted adds).  The YARDSTICK d_ref of a quantity is the larger
max-abs distance from the arbiter of (i) the reference's formulation at float32 (F.conv2d, groups=C, on the GPU, through torch's own depthwise kernels: tests/ssim_ref.py
says why not through MIOpen) and (ii) the separable form at float32.  THE BAR, for the map and for each gradient: max |hip - f64| <= F64_K x d_ref, F64_K = 2 (tests/test_gpu_anisotropic.py).  The scalar
value's bar is the map's: a mean accumulated in f64 cannot be further off than the largest map error.  Where d_ref is exactly 0 the map must be equal, and a
gradient exactly 0 or within 2^-22 max|grad_f64|.  Every comparison prints its ratio err / d_ref before it asserts ("Fused SSIM", has the table).

Bit-for-bit properties (plane isolation, symmetry, layouts, streams, reproducibility) are asserted with torch.equal."""
import os

import numpy as np
import pytest
import torch

from ibgs_amd import image_eval, losses
from tests import ssim_ref as ref

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = losses.ssim_tile()
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEAN = lambda m: m.mean()


def _pair(kind, shape, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape) + len(kind))
    rand = lambda: torch.rand(shape, generator=g)
    randn = lambda: torch.randn(shape, generator=g)
    if kind == "rand":
        a, b = rand(), rand()
    elif kind == "near":
        a = rand()
        b = (a + 0.05 * randn()).clamp(0, 1)
    elif kind == "smooth":          # s1 = p - u^2 cancels: the float32 forms are 1e-4 .. 1e-3 from float64 in the map, and the bar follows d_ref
        h, w = shape[-2:]
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        ramp = (0.5 + 0.4 * torch.sin(0.11 * xx + 0.07 * yy)).expand(shape)
        a, b = ramp + 0.01 * randn(), ramp + 0.01 * randn()
    elif kind == "unclamped":          # what an unclamped render can produce
        a, b = rand() * 1.7 - 0.3, rand() * 1.7 - 0.3
    else:
        raise ValueError(kind)
    return a.float().cuda().contiguous(), b.float().cuda().contiguous()


def _leaves(a, b, wrt):
    return [t.detach().clone().requires_grad_(k in wrt) for k, t in enumerate((a, b))]


def _check_map(name, got, m64, d):
    err = float((got.double() - m64).abs().max())
    print("%-34s map   err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= ref.F64_K * d, (name, err, d)
    else:
        assert err == 0.0, (name, err)


def _check_value(name, got, l64, d_map):
    err = abs(float(got.detach().double()) - float(l64))
    print("%-34s value err %.3e  bar (map) %.3e" % (name, err, ref.F64_K * d_map))
    assert err <= ref.F64_K * d_map, (name, err, d_map)


def _check_grad(name, got, g64, d):
    assert got.shape == g64.shape and got.dtype == torch.float32
    err = float((got.double() - g64).abs().max())
    print("%-34s grad  err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= ref.F64_K * d, (name, err, d)
    else:
        assert float(got.abs().max()) == 0.0 or err <= 2.0 ** -22 * float(g64.abs().max()), (name, err)


def _parity(name, a, b, wrt=(0,)):
    """value, map and the gradients of ssim(a, b) against the arbiter."""
    m64, l64, g64, d_map, d_grad = ref.arbiter_and_yardstick(a, b, MEAN, wrt)
    ins = _leaves(a, b, wrt)
    v = losses.ssim(*ins)
    grads = torch.autograd.grad(v, [ins[k] for k in wrt])
    with torch.no_grad():
        m = losses.ssim_map(a, b)
    assert m.shape == a.shape and m.dtype == torch.float32 and v.shape == () and v.dtype == torch.float32
    _check_map(name, m, m64, d_map)
    _check_value(name, v, l64, d_map)
    for k, g, gr, d in zip(wrt, grads, g64, d_grad):
        _check_grad("%s wrt img%d" % (name, k + 1), g, gr, d)


# ---- 1. the reference's own numbers ----------------------------------------------------------------------------------------------------------------------
def test_reference_produced_numbers():
    d = np.load(os.path.join(G, "metrics.npz"))
    a, b = torch.from_numpy(d["a"]).cuda(), torch.from_numpy(d["b"]).cuda()
    assert abs(float(losses.ssim(a, b)) - float(d["ssim"])) < 2e-6
    np.testing.assert_allclose(losses.ssim(a, b, size_average=False).cpu().numpy(), d["ssim_per_image"], atol=2e-6)
    m = image_eval.image_metrics(a, b)
    assert all(m[k].shape == (4,) and m[k].dtype == torch.float32 and m[k].is_cuda for k in ("ssim", "psnr", "l1"))
    np.testing.assert_allclose(m["psnr"].cpu().numpy(), d["psnr"].reshape(-1), rtol=1e-5)
    assert abs(float(m["l1"].double().mean()) - float(d["l1"])) < 1e-7          # (images of one size: the mean of the per-image means)
    np.testing.assert_allclose(m["ssim"].cpu().numpy(), d["ssim_per_image"], atol=2e-6)
    # the library's overall sums, from the same launch
    x, y = a.contiguous(), b.contiguous()
    mean, l1 = torch.empty((), device="cuda"), torch.empty((), device="cuda")
    losses._ssim_forward((4, 3, 24, 32), x, y, mean=mean, l1=l1)
    assert abs(float(l1) - float(d["l1"])) < 1e-7 and torch.equal(mean, losses.ssim(a, b))
    # a single (C, H, W) image is a batch of one
    assert torch.equal(losses.ssim(a[1], b[1]), losses.ssim(a[1:2], b[1:2])) and torch.equal(losses.ssim(a[1:2], b[1:2], size_average=False)[0], losses.ssim(a[1], b[1]))


# ---- 2. value, map and gradient against the arbiter ------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1), (1, 3, 1, 23), (1, 3, 23, 1), (1, 3, 5, 7), (1, 3, 10, 12), (1, 3, 11, 11), (1, 3, TILE_H + 1, TILE_W + 1),
          (1, 1, 2 * TILE_H - 1, 2 * TILE_W + 5), (2, 3, 40, 70)]


@pytest.mark.parametrize("kind", ["rand", "near", "smooth", "unclamped"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_arbiter_parity(shape, kind):
    a, b = _pair(kind, shape)
    _parity("%s %s" % ("x".join(map(str, shape)), kind), a, b)


# ---- 3. plane isolation and tile independence ------------------------------------------------------------------------------------------------------------
def test_planes_are_isolated_bit_for_bit():
    shape = (2, 3, TILE_H + 3, TILE_W + 3)
    a, b = _pair("near", shape, seed=3)
    a[0, 1] += 0.3          # six different planes, neighbours of clearly different level: a halo that read into the next plane would show
    b[1, 2] *= 0.5
    up = torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda()
    wt = torch.tensor([0.7, -1.3], device="cuda")
    x = a.clone().requires_grad_(True)
    m = losses.ssim_map(x, b)
    g_map, = torch.autograd.grad((m * up).sum(), x)
    x2 = a.clone().requires_grad_(True)
    per = losses.ssim(x2, b, size_average=False)
    g_per, = torch.autograd.grad((per * wt).sum(), x2)
    for n in range(2):
        xi = a[n:n + 1].clone().requires_grad_(True)
        pi = losses.ssim(xi, b[n:n + 1], size_average=False)
        gi, = torch.autograd.grad((pi * wt[n:n + 1]).sum(), xi)
        assert torch.equal(pi[0], per[n]) and torch.equal(gi[0], g_per[n])
        for c in range(3):
            xp = a[n, c][None, None].clone().requires_grad_(True)
            mp = losses.ssim_map(xp, b[n, c][None, None])
            gp, = torch.autograd.grad((mp * up[n, c][None, None]).sum(), xp)
            assert torch.equal(mp[0, 0], m[n, c]) and torch.equal(gp[0, 0], g_map[n, c]), (n, c)


# ---- 4. the padding edges by closed form -----------------------------------------------------------------------------------------------------------------
def test_padding_edges_closed_forms():
    shape = (1, 2, TILE_H + 5, TILE_W + 7)
    c = 0.37
    const = torch.full(shape, c, device="cuda")
    m = losses.ssim_map(const, const.clone())
    assert torch.equal(m, torch.ones_like(m))          # A == C and B == D bit for bit, at the edges too
    assert float(losses.ssim(const, const.clone())) == 1.0
    # zeros against a constant: u = p = r = 0, m = C1 C2 / ((v^2 + C1)(q - v^2 + C2)) with v = w * y, q = w * y^2 under zero padding
    zeros = torch.zeros(shape, device="cuda")
    v, q = ref.blur(const.double(), "shift2d"), ref.blur(const.double() ** 2, "shift2d")
    closed = ref.C1 * ref.C2 / ((v * v + ref.C1) * (q - v * v + ref.C2))
    m64, _, _, d_map, _ = ref.arbiter_and_yardstick(zeros, const, MEAN, ())
    assert float((closed - m64).abs().max()) < 1e-12
    got = losses.ssim_map(zeros, const)
    _check_map("zeros vs constant", got, closed, d_map)
    inner = ref.C1 * ref.C2 / ((c * c + ref.C1) * ref.C2)          # away from the edges the window sums to 1 and q == v^2
    assert abs(float(got[0, 0, 20, 20]) - inner) < 1e-5 * inner + 1e-7 and float(got[0, 0, 0, 0]) != float(got[0, 0, 20, 20])
    # x == y: the gradient is zero
    a, _ = _pair("rand", shape, seed=9)
    _, _, g64, _, d_grad = ref.arbiter_and_yardstick(a, a.clone(), MEAN, (0,))
    x = a.clone().requires_grad_(True)
    g, = torch.autograd.grad(losses.ssim(x, a.clone()), x)
    print("x == y: max |grad| %.3e (float64: %.3e)" % (float(g.abs().max()), float(g64[0].abs().max())))
    _check_grad("x == y", g, g64[0], d_grad[0])


# ---- 5. symmetry -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["near", "unclamped"])
def test_symmetry_and_the_second_images_gradient(kind):
    shape = (1, 3, TILE_H + 1, TILE_W + 1)
    a, b = _pair(kind, shape, seed=2)
    assert torch.equal(losses.ssim_map(a, b), losses.ssim_map(b, a)) and torch.equal(losses.ssim(a, b), losses.ssim(b, a))
    _parity("img2 only %s" % kind, a, b, wrt=(1,))          # a detached, b requiring grad: the form of train.py:330
    _parity("both %s" % kind, a, b, wrt=(0, 1))
    # the value does not depend on which gradients were prepared
    v = [losses.ssim(*_leaves(a, b, wrt)).detach() for wrt in ((), (0,), (1,), (0, 1))]
    assert all(torch.equal(v[0], t) for t in v[1:])


# ---- 6. upstream forms -----------------------------------------------------------------------------------------------------------------------------------
def _photometric(mapfn, ref_image, warped, mask):
    """train.py:324-331 for three sources: ref_image (3, H, W), warped (3, 3, H, W), mask (3, 1, H, W) in warped's dtype."""
    masked = mask * warped + (1 - mask) * ref_image
    loss = 1 - torch.stack([mapfn(ref_image, masked[i]).mean(0) for i in range(len(masked))])
    return torch.sum(loss * mask[:, 0]) / torch.sum(mask[:, 0])


def _grad_bar(name, expr, leaf32):
    """expr(mapfn, leaf) -> a scalar; the gradient with respect to the leaf: hip against the arbiter, with the yardstick of the two float32 forms."""
    def of(dtype, form):
        leaf = leaf32.detach().to(dtype).requires_grad_(True)
        with ref.torch_own_conv():          # (forward and backward: tests/ssim_ref.py, "conv2d")
            loss = expr(lambda x, y: ref.ssim_map_ref(x, y, dtype, form), leaf)
            return loss.detach().double(), torch.autograd.grad(loss, leaf)[0].double()
    l64, g64 = of(torch.float64, "shift2d")
    d = max(float((of(torch.float32, form)[1] - g64).abs().max()) for form in ("conv2d", "separable"))
    leaf = leaf32.detach().clone().requires_grad_(True)
    loss = expr(losses.ssim_map, leaf)
    g, = torch.autograd.grad(loss, leaf, retain_graph=True)
    _check_grad(name, g, g64, d)
    g_again, = torch.autograd.grad(loss, leaf)          # a second backward through the same nodes gives the first's bits
    assert torch.equal(g, g_again)
    assert abs(float(loss.detach()) - float(l64)) <= 1e-4 * max(1.0, abs(float(l64)))
    return g


def test_upstream_forms():
    shape = (2, 3, 40, 70)
    a, b = _pair("near", shape, seed=4)
    # (ssim * 0.2).backward(), and a second backward through the same node
    m64, l64, g64, d_map, d_grad = ref.arbiter_and_yardstick(a, b, lambda m: m.mean() * 0.2, (0,))
    x = a.clone().requires_grad_(True)
    v = losses.ssim(x, b) * 0.2
    v.backward(retain_graph=True)
    g1 = x.grad.clone()
    _check_grad("0.2 x ssim", g1, g64[0], d_grad[0])
    x.grad = None
    v.backward()
    assert torch.equal(x.grad, g1)
    # under no_grad the value is the grad-mode value, bit for bit (and nothing is recorded)
    with torch.no_grad():
        v0 = losses.ssim(x, b)
        m0 = losses.ssim_map(x, b)
    assert torch.equal(v0 * 0.2, v.detach()) and not v0.requires_grad and torch.equal(m0, losses.ssim_map(x, b).detach())
    # size_average=False with a weight per image
    wt = torch.tensor([0.6, -1.7], device="cuda")
    per_loss = lambda m: (m.mean(dim=(1, 2, 3)) * wt.to(m.dtype)).sum()
    m64, l64, g64, d_map, d_grad = ref.arbiter_and_yardstick(a, b, per_loss, (0,))
    x = a.clone().requires_grad_(True)
    per = losses.ssim(x, b, size_average=False)
    assert per.shape == (2,)
    for n in range(2):
        _check_value("per image %d" % n, per[n], m64[n].mean(), d_map)
    g, = torch.autograd.grad((per * wt).sum(), x)
    _check_grad("per-image weights", g, g64[0], d_grad[0])
    # ssim_map under a random upstream map
    up = torch.randn(shape, generator=torch.Generator().manual_seed(8)).cuda()
    _grad_bar("random upstream map", lambda mapfn, leaf: (mapfn(leaf, b.to(leaf.dtype)) * up.to(leaf.dtype)).sum(), a)
    # the photometric term of train.py:324-331: the gradient flows into the second argument
    gen = torch.Generator().manual_seed(11)
    ref_image = torch.rand((3, 40, 70), generator=gen).cuda()
    warped = (ref_image[None] + 0.08 * torch.randn((3, 3, 40, 70), generator=gen).cuda()).clamp(0, 1)
    mask = (torch.rand((3, 1, 40, 70), generator=gen) < 0.4).cuda()
    assert 0.3 < float(mask.float().mean()) < 0.5
    g = _grad_bar("photometric, 3 sources", lambda mapfn, leaf: _photometric(mapfn, ref_image.to(leaf.dtype), leaf, mask.to(leaf.dtype)), warped)
    assert float(g[~mask.expand_as(g)].abs().max()) == 0.0 and float(g[mask.expand_as(g)].abs().max()) > 0.0


# ---- 7. memory layout ------------------------------------------------------------------------------------------------------------------------------------
def _all_three(a, b, up):
    x = a.detach().requires_grad_(True)
    v = losses.ssim(x, b)
    gv, = torch.autograd.grad(v, x)
    m = losses.ssim_map(x, b)
    gm, = torch.autograd.grad((m * up).sum(), x)
    return v.detach(), m.detach(), gv, gm


def test_memory_layouts_give_the_contiguous_bits():
    shape = (2, 3, 19, 53)          # odd W: no row starts where the previous one did modulo 16 bytes
    a, b = _pair("near", shape, seed=6)
    up = torch.randn(shape, generator=torch.Generator().manual_seed(7)).cuda()
    want = _all_three(a, b, up)
    # permuted views
    ap, bp = a.permute(2, 3, 0, 1).contiguous().permute(2, 3, 0, 1), b.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not ap.is_contiguous() and not bp.is_contiguous() and torch.equal(ap, a) and torch.equal(bp, b)
    for w, g in zip(want, _all_three(ap, bp, up)):
        assert torch.equal(w, g)
    # storage that starts 4 bytes off a 16-byte boundary
    n = a.numel()
    off = []
    for t in (a, b):
        buf = torch.empty(n + 8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + n].view(shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        off.append(view)
    for w, g in zip(want, _all_three(off[0], off[1], up)):
        assert torch.equal(w, g)
    assert torch.equal(image_eval.image_metrics(off[0], off[1])["psnr"], image_eval.image_metrics(a, b)["psnr"])


# ---- 8. reproducibility ----------------------------------------------------------------------------------------------------------------------------------
def test_reproducible_and_on_the_callers_stream():
    shape = (2, 3, 2 * TILE_H + 9, 3 * TILE_W - 4)
    a, b = _pair("near", shape, seed=12)
    up = torch.randn(shape, generator=torch.Generator().manual_seed(13)).cuda()
    runs = [_all_three(a, b, up) for _ in range(3)]
    for r in runs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(runs[0], r))
    # on a side stream, right after the ops that produce the inputs there: the kernels are ordered after them by the stream alone
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a2 = (a * 2.0 - a).clone()          # == a, produced on s
        b2 = b + 0.0
        got = _all_three(a2, b2, up)
        mt = image_eval.image_metrics(a2, b2)
    s.synchronize()
    assert torch.equal(a2, a)
    assert all(torch.equal(p, q) for p, q in zip(runs[0], got))
    ref_mt = image_eval.image_metrics(a, b)
    assert all(torch.equal(mt[k], ref_mt[k]) for k in mt)


# ---- 9. full size, one case ------------------------------------------------------------------------------------------------------------------------------
def test_full_size_near_and_evaluate_images():
    a, b = _pair("near", (1, 3, 1080, 1920), seed=1)
    _parity("1x3x1080x1920 near", a, b)
    # evaluate_images on a list of two sizes: the per-view numbers of per-image calls
    small_a, small_b = _pair("near", (3, 37, 53), seed=2)
    views_a, views_b = [a[0], small_a, small_b[None]], [b[0], small_b, small_a[None]]
    out = image_eval.evaluate_images(views_a, views_b, names=["big", "small", "flipped"])
    assert set(out) == {"SSIM", "PSNR", "per_view"} and list(out["per_view"]["SSIM"]) == ["big", "small", "flipped"]
    for name, x, y in zip(("big", "small", "flipped"), views_a, views_b):
        x, y = x.reshape((-1,) + x.shape[-3:]), y.reshape((-1,) + y.shape[-3:])
        m = image_eval.image_metrics(x, y)
        assert out["per_view"]["SSIM"][name] == float(m["ssim"][0]) == float(losses.ssim(x, y))
        assert out["per_view"]["PSNR"][name] == float(m["psnr"][0])
    assert abs(out["SSIM"] - np.mean(list(out["per_view"]["SSIM"].values()))) < 1e-6 and abs(out["PSNR"] - np.mean(list(out["per_view"]["PSNR"].values()))) < 1e-4
    assert out["per_view"]["SSIM"]["small"] == out["per_view"]["SSIM"]["flipped"]          # symmetric in its arguments
    stacked = image_eval.evaluate_images(torch.stack([small_a, small_b]), torch.stack([small_b, small_a]))
    assert list(stacked["per_view"]["PSNR"]) == ["00000", "00001"] and stacked["per_view"]["SSIM"]["00000"] == out["per_view"]["SSIM"]["small"]
