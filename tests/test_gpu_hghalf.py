"""The half-precision hourglass (ibgs_amd.hourglass with precision="float16"; csrc/hghalf.hip) on the device.

The ARBITER is tests/hourglass_ref.forward_ref: float64 numpy on the UNROUNDED float32 input and parameters.  The YARDSTICK of a tensor is
d_ref = max |tests/hghalf_ref.autocast_composition - float64| on the same inputs: torch's own half-precision run of the reference's network on the CPU
(tests/test_hghalf_host.py pins it to a recorded run of the reference), never the kernel.

  1. END TO END: for the six stored stages and the residual, max |hip - f64| <= F64_K x d_ref (F64_K = 2, the bar of DESIGN.md sections 12 - 15).  Where
     d_ref is exactly 0 (a stage of a few elements that are all ReLU-dead): 2^-11 max |f64|, half a binary16 ulp of the largest value.
  2. LAYER-LOCAL: each stored stage against ONE layer in float64 (hghalf_ref.layer_f64) fed the device's own earlier stages, so nothing compounds:
     |hip - f64| <= 1/2 ulp16(f64) + 2 d_chain per element, d_chain the distance from that float64 of a float32 k-ordered multiply-add chain of the same
     layer on the same operands.  This pins round-to-nearest-even, the taps and the padding, which 1. could hide inside its margin.  A second parameter set
     makes e1 binary16-SUBNORMAL: the same bound with no flush term holds only if the f16 matrix-core instruction takes subnormal operands as they are.
  3. EXACT (torch.equal): image_pred, repeatability, strides and dtypes of the input, purity, and a call through the C ABI on an arena of 0xFF bytes.
  4. fuse_color from the rasterizer's outputs, and that the call without the keyword keeps the float32 path's bits.
Every comparison prints its ratio before it asserts (DESIGN.md section 15 quotes the range)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _device, _lib, coloragg, hourglass
from tests import hghalf_ref as href
from tests import hourglass_ref as ref
from tests.test_gpu_hourglass import _net, _params          # the parameter sets "default" and "half_dead", as built there

pytestmark = pytest.mark.gpu

F64_K = 2.0
ZERO_FLOOR = 2.0 ** -11
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ibgs_amd", "csrc", "hghalf.hip")
T = int(re.search(r"constexpr int HGH_TILE = (\d+);", _build._code_only(open(SRC).read())).group(1))          # side of a workgroup's output tile
FRAMES = [(4, 4), (5, 7), (16, 24), (17, 67), (4, T + 1), (T + 1, 4), (2 * T + 3, 2 * T + 5)]
CHECKED = href.CHECKED


@functools.lru_cache(maxsize=None)
def _cpu(h, w, kind, signed=False):
    """-> (x (1, 38, h, w) float32 numpy, arbiter stages, {stage: d_ref}); computed once, shared, written by nobody"""
    x = ref.seeded_input(1000 * h + w, h, w, signed)
    return (x,) + href.d_ref(x, _params(kind))


def _check(name, got, want64, d):
    want = torch.as_tensor(np.asarray(want64), dtype=torch.float64, device=got.device)
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    err = float((got.double() - want).abs().max())
    print("%-44s err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= F64_K * d, (name, err, d)
    else:
        assert err <= ZERO_FLOOR * float(want.abs().max()), (name, err)


def _run(x, net, burned=1.0):
    xd = torch.as_tensor(x).cuda()
    with torch.no_grad():
        residual, image_pred, stages = hourglass.hourglass_forward(xd, net, render_scale=burned, return_stages=True, precision="float16")
    torch.cuda.synchronize()
    assert residual.dtype == torch.float32 and image_pred.dtype == torch.float32 and all(stages[k].dtype == torch.float16 for k in ref.STAGES)
    assert torch.equal(image_pred, burned * xd[0, 35:38] + residual)
    return residual, image_pred, stages


def _parity(name, x, net, want, d_ref):
    residual, image_pred, stages = _run(x, net)
    failed = []
    for k in CHECKED:          # every stage is printed before the first failure is raised: the first stage off its bar localises it
        try:
            _check("%s %s" % (name, k), residual if k == "residual" else stages[k], want[k], d_ref[k])
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]
    return residual, image_pred, stages


def _local(name, x, p, stages, flush_term=False):
    """Check 2 on the six stored stages of one run.  -> the largest |hip - f64| / bound."""
    s = {k: v.float().cpu().numpy().astype(np.float64) for k, v in stages.items()}
    worst, failed = 0.0, []
    for layer, stage in href.LAYER_STAGE:
        inputs = href.layer_inputs(s, x[0], layer)
        want = href.layer_f64(inputs, p[layer + "_w"], p[layer + "_b"])
        d_chain = float(np.abs(href.layer_chain(inputs, p[layer + "_w"], p[layer + "_b"]).astype(np.float64) - want).max())
        bound = 0.5 * href.ulp16(want) + 2.0 * d_chain
        if flush_term:
            bound = bound + 2.0 ** -14 * np.abs(href.h16(p[layer + "_w"])).reshape(want.shape[0], -1).sum(1).max()
        ratio = np.abs(s[stage] - want) / bound
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print("%-44s |hip - f64| / bound %.3f at %s (f64 %.6e, hip %.6e; d_chain %.2e)" % ("%s %s" % (name, stage), ratio.max(), at, want[at], s[stage][at], d_chain))
        worst = max(worst, float(ratio.max()))
        if not ratio.max() <= 1.0:
            failed.append((name, stage, float(ratio.max()), at))
    assert not failed, failed
    return worst


# ---- 1. and 2.: frames x parameter sets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "half_dead"])
@pytest.mark.parametrize("h,w", FRAMES)
def test_against_float64_end_to_end_and_layer_by_layer(h, w, kind):
    x, want, d_ref = _cpu(h, w, kind)
    name = "%dx%d %s" % (h, w, kind)
    failed = []
    try:
        residual, image_pred, stages = _parity(name, x, _net(kind), want, d_ref)
    except AssertionError as e:
        failed.append(e)
        residual, image_pred, stages = _run(x, _net(kind))
    assert tuple(stages["b"].shape) == (9, h // 4, w // 4) and tuple(stages["e2"].shape) == (19, h // 2, w // 2) and tuple(residual.shape) == (3, h, w)
    _local(name, x, _params(kind), stages)
    if failed:
        raise failed[0]


def test_arbitrary_sign_features():
    h, w = 17, 67
    x, want, d_ref = _cpu(h, w, "default", True)
    assert x[0, :32].min() < -1
    _, _, stages = _parity("%dx%d signed" % (h, w), x, _net("default"), want, d_ref)
    _local("%dx%d signed" % (h, w), x, _params("default"), stages)


def test_binary16_subnormal_operands_are_taken_as_they_are():
    """enc1 scaled by 2^-13 makes most of e1 binary16-subnormal (below 2^-14), enc2 scaled by 2^12 brings e2 back to ordinary magnitudes.  The layer-local
    bound WITHOUT a flush term then holds for e1 (the conversion writes subnormals) and for e2 (the f16 matrix-core instruction reads them): a kernel or an
    instruction that flushed them would leave e2 = relu(bias) and miss the bound by orders of magnitude."""
    h, w = 17, 67
    p = dict(_params("default"))
    p["enc1_w"], p["enc1_b"] = (p["enc1_w"] * np.float32(2.0 ** -13)).astype(np.float32), (p["enc1_b"] * np.float32(2.0 ** -13)).astype(np.float32)
    p["enc2_w"] = (p["enc2_w"] * np.float32(2.0 ** 12)).astype(np.float32)
    net = hourglass.HourglassCNN()
    net.load_state_dict({k: torch.tensor(v) for k, v in p.items()})
    net = net.cuda().requires_grad_(False)
    x = _cpu(h, w, "default")[0]
    _, _, stages = _run(x, net)
    e1 = stages["e1"].float()
    sub = float(((e1 > 0) & (e1 < 2.0 ** -14)).float().mean())
    print("%.2f of e1 is a non-zero binary16 subnormal; e2 has max %.3f" % (sub, float(stages["e2"].float().max())))
    assert sub > 0.25 and float(stages["e2"].float().max()) > 0.05
    flushed = href.layer_f64(np.zeros((38, h // 2, w // 2)), p["enc2_w"], p["enc2_b"])
    kept = href.layer_f64(ref.pool_ref(e1.cpu().numpy().astype(np.float64)), p["enc2_w"], p["enc2_b"])
    got = stages["e2"].float().cpu().numpy().astype(np.float64)
    print("e2: max |hip - f64 with the subnormals| %.3e, max |hip - f64 with e1 flushed to zero| %.3e" % (np.abs(got - kept).max(), np.abs(got - flushed).max()))
    worst = _local("subnormal e1", x, p, stages)
    assert worst <= 1.0


# ---- 3. exact properties -------------------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    h, w = 17, 67
    x = torch.as_tensor(_cpu(h, w, "default")[0]).cuda()
    net = _net("default")
    x0, p0 = x.clone(), [p.detach().clone() for p in net.parameters()]
    half = dict(precision="float16")
    with torch.no_grad():
        plain = hourglass.hourglass_forward(x, net, **half)
        assert torch.is_tensor(plain) and tuple(plain.shape) == (3, h, w) and plain.dtype == torch.float32
        assert not torch.equal(plain, hourglass.hourglass_forward(x, net))          # another precision than the float32 path
        for burned in (1.0, 0.75):
            residual, image_pred = hourglass.hourglass_forward(x, net, render_scale=burned, **half)
            assert torch.equal(residual, plain) and torch.equal(image_pred, burned * x[0, 35:38] + residual), burned
        again = net(x, **half)          # a second call, through the module
        assert torch.equal(again, plain)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            side, side_pred, side_stages = hourglass.hourglass_forward(x, net, render_scale=0.75, return_stages=True, **half)
        s.synchronize()
        assert torch.equal(side, plain) and torch.equal(side_pred, image_pred)
        # strides, layouts and dtypes of the input
        wide = torch.zeros(1, 38, h, 2 * w + 1, device="cuda")
        wide[..., ::2][..., :w] = x
        views = {"(38, H, W)": x[0], "every other column": wide[..., ::2][..., :w], "transposed storage": x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2),
                 "channels last": x.contiguous(memory_format=torch.channels_last), "float64": x.double()}
        assert not views["every other column"].is_contiguous() and not views["transposed storage"].is_contiguous()
        for what, v in views.items():
            assert torch.equal(v.float().reshape(x.shape), x)
            r, ip, st = hourglass.hourglass_forward(v, net, render_scale=0.75, return_stages=True, **half)
            assert torch.equal(r, plain) and torch.equal(ip, image_pred) and all(torch.equal(st[k], side_stages[k]) for k in ref.STAGES), what
        # through the C ABI on a test-owned arena of 0xFF bytes (NaN at both widths): the bits of the public call, and no NaN anywhere
        need = _lib.load().ibgs_hgh_required_scratch(h, w)
        arena = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        assert bool(torch.isnan(arena[:4096].view(torch.float16)).all()) and bool(torch.isnan(arena[:4096].view(torch.float32)).all())
        flat = [getattr(net, layer + s).detach().contiguous() for layer, _, _, _ in hourglass.LAYERS for s in ("_w", "_b")]
        r = torch.full((3, h, w), float("nan"), device="cuda")
        ip = torch.full((3, h, w), float("nan"), device="cuda")
        _device.call(x.device, "ibgs_hgh_forward", h, w, x.data_ptr(), *[t.data_ptr() for t in flat], 0.75, r.data_ptr(), ip.data_ptr(), arena.data_ptr(), arena.numel())
        torch.cuda.synchronize()
        st = hourglass._arena_views(arena, h, w, half=True)
        assert torch.equal(r, plain) and torch.equal(ip, image_pred) and all(torch.equal(st[k], side_stages[k]) for k in ref.STAGES)
        assert not bool(torch.isnan(r).any()) and not bool(torch.isnan(ip).any()) and not any(bool(torch.isnan(v).any()) for v in st.values())
        e1_all = arena[st["e1"].data_ptr() - arena.data_ptr():][:h * w * 40 * 2].view(torch.float16).view(h, w, 40)          # the padding channels: zeros
        assert torch.equal(e1_all[..., :38].permute(2, 0, 1), st["e1"]) and bool((e1_all[..., 38:] == 0).all())
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and all(torch.equal(p, q) for p, q in zip(net.parameters(), p0))
    with pytest.raises(ValueError, match=r'"float32" or "float16"'):
        with torch.no_grad():
            hourglass.hourglass_forward(x, net, precision="bfloat16")
    live = hourglass.HourglassCNN().cuda()
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):
        live(x, **half)


# ---- 4. end to end: the rasterizer's outputs in, image_pred out ------------------------------------------------------------------------------------------
def test_fuse_color_from_the_rasterizer():
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
    torch.manual_seed(7)
    net = hourglass.ColorAggregationNet().to(dev)
    p = {k: v.detach().cpu().numpy() for k, v in net.cnn.state_dict().items()}
    renderer.clear_caches()
    try:
        with torch.no_grad():
            for j in cam.nearest_id:
                scn.rendered_depth_list[j] = renderer.render_depth(cams[j], pc, scn, pipe, args, torch.zeros(3, device=dev), True, 3, 4)
            pkg = renderer.render(cam, pc, scn, pipe, args, torch.zeros(3, device=dev), learnt_normal=True, nb_src_frames=3, buffer_length=4, render_geo=True)
            out = hourglass.fuse_color(pkg, net, 3, burned_in_gauss=0.75, precision="float16")
            cnn_input, mask = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
            assert sorted(out) == ["burned_in_gauss", "image_pred", "nb_valid_warp_level", "residual", "valid_warp_mask", "warped_image_list"]
            assert 1 <= int(out["nb_valid_warp_level"]) <= 3 and torch.equal(out["valid_warp_mask"], mask)
            want, d_ref = href.d_ref(cnn_input.cpu().numpy(), p)
            _check("fuse_color residual", out["residual"], want["residual"], d_ref["residual"])
            assert out["residual"].dtype == torch.float32 and torch.equal(out["image_pred"], 0.75 * pkg["render"] + out["residual"])
            through_module = net(pkg, 3, 0.75, precision="float16")
            assert torch.equal(through_module["residual"], out["residual"]) and torch.equal(through_module["image_pred"], out["image_pred"])
            # without the keyword: the bits of the float32 path
            plain = hourglass.fuse_color(pkg, net, 3, burned_in_gauss=0.75)
            r32, ip32 = hourglass.hourglass_forward(cnn_input, net.cnn, render_scale=0.75, precision="float32")
            assert torch.equal(plain["residual"], r32) and torch.equal(plain["image_pred"], ip32) and not torch.equal(r32, out["residual"])
            explicit = hourglass.fuse_color(pkg, net, 3, burned_in_gauss=0.75, precision="float32")
            assert torch.equal(explicit["residual"], r32) and torch.equal(explicit["image_pred"], ip32)
            # no slot carries a colour: nothing raises and the level count is 0
            empty = dict(pkg, warped_image=torch.zeros_like(pkg["warped_image"]))
            none = hourglass.fuse_color(empty, net, 3, precision="float16")
            assert int(none["nb_valid_warp_level"]) == 0 and hourglass.fuse_color(empty, net, 3, none_if_no_level=True, precision="float16") is None
            assert not bool(torch.isnan(none["image_pred"]).any())
    finally:
        renderer.clear_caches()
