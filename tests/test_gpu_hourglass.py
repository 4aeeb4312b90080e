"""The hourglass CNN (ibgs_amd.hourglass; csrc/hourglass.hip) on the device.

The ARBITER is tests/hourglass_ref.forward_ref (float64 numpy).  The YARDSTICK of a tensor is d_ref = max(d_torch, d_chain): the max-abs distances from the
arbiter of tests/hourglass_ref.torch_composition at float32 ON THE CPU and of tests/hourglass_ref.chain_f32 (every convolution one k-ordered, singly rounded
multiply-add chain from the bias: what the f32 matrix-core instruction is), on the same inputs.  THE BAR, as in tests/test_gpu_coloragg.py:
max |hip - f64| <= F64_K x d_ref (F64_K = 2); where d_ref is exactly 0: 2^-22 max |f64|.  Two yardsticks because torch's blocked CPU convolution is
2 - 4 e-8 from float64 on outputs of about 0.2 and an honest sequential chain 1.2 - 2.2 times that: torch alone would refuse a correct kernel, the chain
alone would be a yardstick chosen here; neither is the code under test.  On the CPU because MIOpen compiles a kernel on the first use of every odd shape (the
device composition is timed by tools/bench_hourglass.py).  Every comparison prints its ratio before it asserts (DESIGN.md section 15 quotes the range), every
stage has its own d_ref, and bit-for-bit properties are asserted with torch.equal."""
import functools
import os
import time

import numpy as np
import pytest
import torch

from ibgs_amd import coloragg, hourglass
from tests import hourglass_ref as ref

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
T = 16          # side of a workgroup's output tile (csrc/shared/conv_tile.h: CT_TILE; tests/test_hourglass_host.py checks the constant).  The grid is not capped.
FRAMES = [(4, 4), (5, 7), (16, 24), (17, 67), (4, T + 1), (T + 1, 4), (2 * T + 3, 2 * T + 5)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hourglass.npz")
CHECKED = ref.STAGES + ("residual",)


# ---- parameters, inputs and the three CPU evaluations, computed once and shared: nobody writes them -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _params(kind):
    """"default": nn.Conv2d's initialisation, seeded.  "half_dead": the same with every ReLU layer's bias moved by the median of its pre-activation on a
    16 x 24 input, layer after layer, so that about half of every stage is dead."""
    p = ref.seeded_params(11)
    if kind == "half_dead":
        x = ref.seeded_input(12, 16, 24)
        for layer, stage in (("enc1", "e1"), ("enc2", "e2"), ("enc3", "b"), ("up2_conv", "u2"), ("dec2", "d2"), ("up1_conv", "u1"), ("dec1", "d1"), ("fuse_input", "f")):
            p[layer + "_b"] = (p[layer + "_b"] + 1.0).astype(np.float32)          # lift the layer: its output is its pre-activation while that is positive
            pre = ref.forward_ref(x, p)[stage]
            assert pre.min() > 0
            p[layer + "_b"] = (p[layer + "_b"] - np.float32(np.median(pre))).astype(np.float32)
        s = ref.forward_ref(x, p)
        for stage in ref.STAGES + ("d1", "f"):
            dead = float((s[stage] == 0).mean())
            assert 0.3 < dead < 0.7, (stage, dead)
    return p


@functools.lru_cache(maxsize=None)
def _net(kind):
    net = hourglass.HourglassCNN()
    net.load_state_dict({k: torch.tensor(v) for k, v in _params(kind).items()})
    return net.cuda().requires_grad_(False)


@functools.lru_cache(maxsize=None)
def _cpu(h, w, kind, signed=False):
    """-> (x (1, 38, h, w) float32 numpy, arbiter stages, {stage: d_ref}, {stage: (d_torch, d_chain)})"""
    x = ref.seeded_input(1000 * h + w, h, w, signed)
    return (x,) + _yardsticks(x, _params(kind))


def _yardsticks(x, p):
    want = ref.forward_ref(x, p)
    t32, chain = ref.torch_composition(x, p, torch.float32), ref.chain_f32(x, p)
    both = {k: (float(np.abs(t32[k].numpy().astype(np.float64) - want[k]).max()), float(np.abs(chain[k].astype(np.float64) - want[k]).max())) for k in CHECKED}
    return want, {k: max(v) for k, v in both.items()}, both


def _check(name, got, want64, d, both=None):
    want = torch.as_tensor(np.asarray(want64), dtype=torch.float64, device=got.device)
    assert got.dtype == torch.float32 and got.shape == want.shape, (name, got.dtype, tuple(got.shape), tuple(want.shape))
    err = float((got.double() - want).abs().max())
    print("%-56s err %.3e  d_ref %.3e%s  ratio %s" % (name, err, d, "" if both is None else " (torch %.3e, chain %.3e)" % both, "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= F64_K * d, (name, err, d)
    else:
        assert err <= FLOOR * float(want.abs().max()), (name, err)


def _parity(name, x, net, want, d_ref, both, burned=1.0):
    xd = torch.as_tensor(x).cuda()
    with torch.no_grad():
        residual, image_pred, stages = hourglass.hourglass_forward(xd, net, render_scale=burned, return_stages=True)
    torch.cuda.synchronize()
    failed = []
    for k in CHECKED:          # every stage is printed before the first failure is raised: the first stage off its bar localises it
        try:
            _check("%s %s" % (name, k), residual if k == "residual" else stages[k], want[k], d_ref[k], both[k])
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]
    assert torch.equal(image_pred, burned * xd[0, 35:38] + residual)
    return residual, image_pred, stages


# ---- 1. frames x parameter sets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "half_dead"])
@pytest.mark.parametrize("h,w", FRAMES)
def test_forward_and_stages_against_float64(h, w, kind):
    x, want, d_ref, both = _cpu(h, w, kind)
    residual, image_pred, stages = _parity("%dx%d %s" % (h, w, kind), x, _net(kind), want, d_ref, both)
    assert tuple(stages["b"].shape) == (9, h // 4, w // 4) and tuple(residual.shape) == (3, h, w)
    if kind == "half_dead" and h * w >= 16 * 24:
        for k in ref.STAGES:
            dead = float((stages[k] == 0).float().mean())
            print("%dx%d half_dead %s: %.2f of the stage is ReLU-dead" % (h, w, k, dead))
            assert 0.15 < dead < 0.85, (k, dead)


@pytest.mark.parametrize("h,w", [(17, 67), (2 * T + 3, 2 * T + 5)])
def test_arbitrary_sign_features(h, w):
    x, want, d_ref, both = _cpu(h, w, "default", True)
    assert x[0, :32].min() < -1
    _parity("%dx%d signed" % (h, w), x, _net("default"), want, d_ref, both)


# ---- 2. the recorded runs of the reference's own network -----------------------------------------------------------------------------------------------
def test_reference_fixtures():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.tensor(z[k]) for k in z.files if k.startswith("sd/")}
    net = hourglass.ColorAggregationNet()
    net.load_state_dict(sd)
    net = net.cuda().requires_grad_(False)
    p = {mine: sd["conv_decoder." + theirs].numpy() for theirs, mine in hourglass.REFERENCE_KEYS.items()}
    for tag, x, recorded in (("fixture 16x24", z["cnn_input"], z["residual"].T.reshape(3, 16, 24)), ("fixture 13x19", z["odd_cnn_input"], z["odd_residual"][0])):
        want, d_ref, both = _yardsticks(x, p)
        print("%s: the reference's recorded float32 run is %.3e from float64" % (tag, float(np.abs(recorded - want["residual"]).max())))
        residual, _, _ = _parity(tag, x, net.cnn, want, d_ref, both)
        # ... and the recorded residual itself, in the (B, 3) form the reference's network returns: within the bar's reach of it (its own distance added)
        got = residual.permute(1, 2, 0).reshape(-1, 3).cpu().numpy()
        theirs = recorded.transpose(1, 2, 0).reshape(-1, 3)
        assert np.abs(got - theirs).max() <= F64_K * d_ref["residual"] + np.abs(recorded - want["residual"]).max()


# ---- 3. exact properties -------------------------------------------------------------------------------------------------------------------------------
def test_image_pred_is_torchs_expression_and_the_call_is_pure():
    h, w = 17, 67
    x = torch.as_tensor(_cpu(h, w, "default")[0]).cuda()
    net = _net("default")
    x0, p0 = x.clone(), [p.detach().clone() for p in net.parameters()]
    with torch.no_grad():
        plain = hourglass.hourglass_forward(x, net)
        assert torch.is_tensor(plain) and tuple(plain.shape) == (3, h, w)
        for burned in (1.0, 0.75):
            residual, image_pred = hourglass.hourglass_forward(x, net, render_scale=burned)
            assert torch.equal(residual, plain) and torch.equal(image_pred, burned * x[0, 35:38] + residual), burned
        again = net(x)          # a second call, through the module
        assert torch.equal(again, plain)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            side, side_pred, side_stages = hourglass.hourglass_forward(x, net, render_scale=0.75, return_stages=True)
        s.synchronize()
        assert torch.equal(side, plain) and torch.equal(side_pred, image_pred)
        # strides and the (38, H, W) form
        wide = torch.zeros(1, 38, h, 2 * w + 1, device="cuda")
        wide[..., ::2][..., :w] = x
        views = {"(38, H, W)": x[0], "every other column": wide[..., ::2][..., :w], "transposed storage": x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2),
                 "channels last": x.contiguous(memory_format=torch.channels_last), "float64": x.double()}
        assert not views["every other column"].is_contiguous() and not views["transposed storage"].is_contiguous()
        for what, v in views.items():
            assert torch.equal(v.float().reshape(x.shape), x)
            r, ip, st = hourglass.hourglass_forward(v, net, render_scale=0.75, return_stages=True)
            assert torch.equal(r, plain) and torch.equal(ip, image_pred) and all(torch.equal(st[k], side_stages[k]) for k in ref.STAGES), what
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and all(torch.equal(p, q) for p, q in zip(net.parameters(), p0))
    # parameters that require grad are fine under no_grad, refused with grad mode on; tensors on two devices are refused by name
    live = hourglass.HourglassCNN().cuda()
    with torch.no_grad():
        assert tuple(live(x).shape) == (3, h, w)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):
        live(x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        with torch.no_grad():
            hourglass.hourglass_forward(x, hourglass.HourglassCNN())
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="cnn_input is on"):
            with torch.no_grad():
                hourglass.hourglass_forward(x.to("cuda:1"), net)


def test_the_call_never_waits():
    """The forward behind a queue of other work: it returns while that work is still running (the events-around-a-queue check of tests/test_gpu_coloragg.py)."""
    x = torch.as_tensor(_cpu(17, 67, "default")[0]).cuda()
    net = _net("default")
    with torch.no_grad():
        want = hourglass.hourglass_forward(x, net, render_scale=1.0)
    a = torch.rand(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    start, queued, done = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    start.record()
    for _ in range(40):
        a = (a @ a).clamp_(0, 1)
    queued.record()
    t0 = time.perf_counter()
    with torch.no_grad():
        got = hourglass.hourglass_forward(x, net, render_scale=1.0)
    host_ms = (time.perf_counter() - t0) * 1e3
    still_running = not queued.query()
    done.record()
    torch.cuda.synchronize()
    print("forward: host %.3f ms; the queue in front of it %.3f ms on the device, its own kernels %.3f ms" % (host_ms, start.elapsed_time(queued), queued.elapsed_time(done)))
    assert still_running, "hourglass_forward returned only after the work queued in front of it had finished: something in it waits for the device"
    assert host_ms < start.elapsed_time(queued)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 4. end to end: the rasterizer's outputs in, image_pred out ------------------------------------------------------------------------------------------
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
    torch.manual_seed(7)
    net = hourglass.ColorAggregationNet().to(dev)
    p = {k: v.detach().cpu().numpy() for k, v in net.cnn.state_dict().items()}
    renderer.clear_caches()
    try:
        with torch.no_grad():
            for j in cam.nearest_id:
                scn.rendered_depth_list[j] = renderer.render_depth(cams[j], pc, scn, pipe, args, torch.zeros(3, device=dev), True, 3, 4)
            pkg = renderer.render(cam, pc, scn, pipe, args, torch.zeros(3, device=dev), learnt_normal=True, nb_src_frames=3, buffer_length=4, render_geo=True)
            out = hourglass.fuse_color(pkg, net, 3, burned_in_gauss=0.75)
            cnn_input, mask = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
            assert sorted(out) == ["burned_in_gauss", "image_pred", "nb_valid_warp_level", "residual", "valid_warp_mask", "warped_image_list"]
            lv = out["nb_valid_warp_level"]
            assert lv.is_cuda and lv.dtype == torch.int32 and lv.dim() == 0 and 1 <= int(lv) <= 3 and out["burned_in_gauss"] == 0.75
            assert torch.equal(out["valid_warp_mask"], mask) and tuple(out["warped_image_list"].shape) == (H, W, 3, 3)
            assert torch.equal(out["warped_image_list"], pkg["warped_image"].view(-1, 3, H, W)[:3].permute(2, 3, 0, 1))
            want, d_ref, both = _yardsticks(cnn_input.cpu().numpy(), p)
            _check("end to end residual", out["residual"], want["residual"], d_ref["residual"], both["residual"])
            assert torch.equal(out["image_pred"], 0.75 * pkg["render"] + out["residual"])
            assert hourglass.fuse_color(pkg, net, 3, none_if_no_level=True) is not None
            # no slot carries a colour: nothing raises, the level count is 0 and image_pred is the network's output on zero features
            empty = dict(pkg, warped_image=torch.zeros_like(pkg["warped_image"]))
            none = hourglass.fuse_color(empty, net, 3)
            assert int(none["nb_valid_warp_level"]) == 0 and hourglass.fuse_color(empty, net, 3, none_if_no_level=True) is None
            zero_feat = cnn_input.clone()
            zero_feat[:, :32] = 0
            r0, ip0 = hourglass.hourglass_forward(zero_feat, net.cnn, render_scale=1.0)
            assert torch.equal(none["residual"], r0) and torch.equal(none["image_pred"], ip0) and not torch.equal(r0, out["residual"])
        with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\).*training keeps torch's CNN"):
            hourglass.fuse_color(pkg, net, 3)
    finally:
        renderer.clear_caches()
