"""Training at a reduced residual resolution (ibgs_amd.resample_train; csrc/rsztrain.hip) on the device.

The ARBITER is tests/resample_train_ref (float64 autograd of the explicit-tap composition; for the whole tail chained through tests/hourglass_bwd_ref).  The
YARDSTICK of a gradient tensor is d_ref = the larger of the max-abs distances from the arbiter of two float32 evaluations ON THE CPU on the same inputs: torch's
own composition (F.interpolate, Linear, autograd) and the arbiter's float32 twin.  THE BAR is the project's: max |hip - f64| <= F64_K x d_ref (F64_K = 2);
where d_ref is exactly 0: 2^-22 max |f64|.  Every comparison prints its ratio before it asserts (DESIGN.md section 19 quotes the range); bit-for-bit
properties are asserted with torch.equal.

A gradient is discontinuous where a pre-activation or a max-mode gap is 0: every frame uses its decided seed (tests/resample_train_ref.SEEDS; the host test
asserts the margin).  The reduced-resolution kernel's grid is capped at 512 workgroups of 128 reduced pixels: one frame (516 x 512 at 0.5: 516 chunks) lies
beyond one pass of it, decided by raised biases."""
import functools
import os

import numpy as np
import pytest
import torch

from ibgs_amd import coloragg, exposure, hourglass, resample, resample_train
from tests import dirty_alloc as da
from tests import hourglass_ref
from tests import resample_ref as ref
from tests import resample_train_ref as tr
from tests.test_gpu_resample import UPSAMPLE
from tests.test_resample_train_host import fixture

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
DEV = "cuda"
OWN_SIZE_SEEDS = {(13, 20, 1.0): 1}          # decided like tr.SEEDS (the test that uses it asserts so): a frame resampled to its own size
CNN_NAMES = [name + suffix for name, _, _, _ in hourglass_ref.LAYERS for suffix in ("_w", "_b")]


def _dev(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def _compare(tag, got, want, t32, twin, failed):
    """Prints the ratio; appends to `failed` what misses the bar."""
    assert got is not None, tag
    w64 = torch.as_tensor(np.asarray(want), dtype=torch.float64, device=got.device).reshape(got.shape)
    assert got.dtype == torch.float32
    err = float((got.double() - w64).abs().max())
    d = max(float(np.abs(np.asarray(t32, np.float64) - want).max()), float(np.abs(np.asarray(twin, np.float64) - want).max()))
    top = float(w64.abs().max())
    print("%-72s err %.3e  d_ref %.3e  max|f64| %.3e  ratio %s" % (tag, err, d, top, "%.2f" % (err / d) if d > 0 else "-"))
    if not (err <= F64_K * d if d > 0 else err <= FLOOR * top):
        failed.append((tag, err, d, top))


# ---- the CPU evaluations, computed once and shared: nobody writes them -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(h, w, s, raised=False):
    case, params = ref.seeded_case(h, w, seed=0 if raised else {**tr.SEEDS, **OWN_SIZE_SEEDS}[(h, w, s)])
    size = ref.scaled_size(h, w, s)
    if raised:
        params = tr.raised_biases(case, params, size)
        with torch.no_grad():
            _, (z1, z2) = tr.features(*case, *params, size, 3, "mean", torch.float64, return_preacts=True)
        assert float(z1.min()) >= 0.5 and float(z2.min()) >= 0.5
    go = torch.randn((1, 38) + size, generator=torch.Generator().manual_seed(1000 * h + w))
    return case, params, size, go


@functools.lru_cache(maxsize=None)
def _feature_cpu(h, w, s, mode, levels, raised=False):
    case, params, size, go = _case(h, w, s, raised)
    want, _ = tr.feature_grads(case, params, size, levels, mode, go)
    t32, _ = tr.feature_grads(case, params, size, levels, mode, go, torch.float32, interpolate=True)
    twin, _ = tr.feature_grads(case, params, size, levels, mode, go, torch.float32)
    return want, t32, twin


def _leaves(tensors):
    return [t.detach().clone().to(DEV).requires_grad_(True) for t in tensors]


def _feature_run(case, params, size, levels, mode, go):
    """-> (cnn_input, {name: gradient}) of resized_features_train on fresh leaves"""
    render, warped = _leaves(case[:2])
    p = _leaves(params)
    out = resample_train.resized_features_train(render, warped, _dev(case[2]), _dev(case[3]), *p, size, levels, mode)
    (out * go).sum().backward()
    return out.detach(), dict(zip(tr.NAMES, [t.grad for t in [render, warped] + p]))


def _feature_parity(h, w, s, mode, levels, raised=False):
    case, params, size, go = _case(h, w, s, raised)
    want, t32, twin = _feature_cpu(h, w, s, mode, levels, raised)
    out, grads = _feature_run(case, params, size, levels, mode, go.to(DEV))
    word = torch.full((), levels, dtype=torch.int32, device=DEV)
    out_w, grads_w = _feature_run(case, params, size, word, mode, go.to(DEV))          # the level count as a device word: the same bits
    with torch.no_grad():
        plain = resample.resized_features(*[_dev(t) for t in case], *[_dev(t) for t in params], size, levels, mode)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(out_w, plain) and int(word) == levels          # the forward is resample's, bit for bit
    assert all(torch.equal(grads[k], grads_w[k]) for k in tr.NAMES)
    failed = []
    for k in tr.NAMES:
        _compare("%dx%d s %.2f -> %dx%d %s levels %d %s" % (h, w, s, size[0], size[1], mode, levels, k), grads[k], want[k], t32[k], twin[k], failed)
    assert not failed, failed
    return grads, want


# ---- 1. resized_features_train --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("frame", tr.FRAMES, ids=lambda f: "%dx%d_s%g" % f)
def test_feature_gradients_against_float64(frame, mode):
    h, w, s = frame
    for levels in (3, 1, 0):
        grads, want = _feature_parity(h, w, s, mode, levels)
        assert grads["warped"].shape == (3, 3, h, w) and float(grads["warped"][levels:].abs().max() if levels < 3 else 0.0) == 0.0          # zero from `levels` on
        if levels == 0:          # no slot: only the colour channels' gradient reaches render, gathered
            assert all(float(grads[k].abs().max()) == 0.0 for k in tr.NAMES[1:]) and float(grads["render"].abs().max()) > 0
        else:
            assert all(float(grads[k].abs().max()) > 0 for k in tr.NAMES)
            assert float(grads["warped"][1].abs().max()) == 0.0          # slot 1 is invalid everywhere: its mask is the full-resolution pixel's own


def test_a_frame_beyond_one_pass_of_the_capped_grid():
    h, w, s = tr.BIG
    _feature_parity(h, w, s, "mean", 3, raised=True)


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("h,w,levels,raised,chunks", [(13, 20, 2, False, 3), (257, 256, 3, True, 514)], ids=["13x20_levels2", "257x256_levels3"])
def test_at_the_frames_own_size_the_backward_is_the_front_ends(h, w, levels, raised, chunks, mode):
    """rzt_features_bwd_kernel and cagg_bwd_kernel run ONE per-slot backward and ONE set of parameter sums (csrc/shared/pv_mlp_bwd.h) and one final pass
    (cagg_final_kernel).  At size == (H, W) every tap has t = 0 and u = 1, and fma(0, b, 1 a) = a for finite inputs (a masked -0 becomes +0, which changes no
    product's bits that torch.equal sees), so a slot's blended row is the pixel's own row; the two grids agree (pv_bwd_groups of the same H W), so every workgroup
    adds the same chunks in the same order.  The gather's weight is 1 at the pixel itself and its G = fma(1, gx, 0) = gx, so grad_warped = gx v in both.  Hence
    the same bits for grad_warped and the four parameter gradients.  grad_render is NOT compared bit for bit: the gather forms (go - gv0) - gv1 .. where the front
    end forms go + ((0 - gv0) - gv1 ..), and the two associations round differently; both are held to this file's bar against the float64 arbiter.  The forwards
    are not compared: channels 32 .. 34 differ by design (the reduced tail normalises the ray).
    13 x 20, levels 2 of 3: three chunks of 128, the last with lanes past the frame, one slot zeroed.  257 x 256: 514 chunks against the cap of 512, so two
    workgroups walk a second chunk; raised biases keep every ReLU away from zero."""
    case, params, size, go = _case(h, w, 1.0, raised)
    assert size == (h, w) and (h * w + 127) // 128 == chunks
    if not raised:
        assert tr.decided_seed(h, w, 1.0) == OWN_SIZE_SEEDS[(h, w, 1.0)]
    go = go.to(DEV)
    _, mine = _feature_run(case, params, size, levels, mode, go)
    render, warped = _leaves(case[:2])
    p = _leaves(params)
    out, _ = coloragg.per_view_features(render, warped, _dev(case[2]), _dev(case[3]), *p, levels=levels, mode=mode)
    (out * go).sum().backward()
    theirs = dict(zip(tr.NAMES, [t.grad for t in [render, warped] + p]))
    torch.cuda.synchronize()
    for k in tr.NAMES[1:]:
        assert mine[k].shape == theirs[k].shape and float(mine[k].abs().max()) > 0, k
        assert torch.equal(mine[k], theirs[k]), (k, float((mine[k] - theirs[k]).abs().max()))
    assert float(mine["warped"][levels:].abs().max() if levels < 3 else 0.0) == 0.0
    want, t32, twin = _feature_cpu(h, w, 1.0, mode, levels, raised)
    failed = []
    for who, grads in (("reduced", mine), ("front end", theirs)):
        _compare("%dx%d at its own size %s levels %d render (%s)" % (h, w, mode, levels, who), grads["render"], want["render"], t32["render"], twin["render"], failed)
    assert not failed, failed


def test_only_what_autograd_needs():
    """Detached images: the parameter gradients are the bits of the full backward (the gather kernel and the scratch planes are not used); frozen parameters: the
    image gradients are."""
    h, w, s = 35, 37, 0.5
    case, params, size, go = _case(h, w, s)
    go = go.to(DEV)
    for mode in ("mean", "max"):
        _, full = _feature_run(case, params, size, 3, mode, go)
        p = _leaves(params)
        out = resample_train.resized_features_train(_dev(case[0]), _dev(case[1]), _dev(case[2]), _dev(case[3]), *p, size, 3, mode)
        (out * go).sum().backward()
        assert all(torch.equal(t.grad, full[k]) for t, k in zip(p, tr.NAMES[2:]))
        render, warped = _leaves(case[:2])
        out = resample_train.resized_features_train(render, warped, _dev(case[2]), _dev(case[3]), *[_dev(t) for t in params], size, 3, mode)
        (out * go).sum().backward()
        assert torch.equal(render.grad, full["render"]) and torch.equal(warped.grad, full["warped"])
        render, = _leaves(case[:1])          # one image alone
        out = resample_train.resized_features_train(render, _dev(case[1]), _dev(case[2]), _dev(case[3]), *[_dev(t) for t in params], size, 3, mode)
        (out * go).sum().backward()
        assert torch.equal(render.grad, full["render"])
    x = _leaves(case[:1])[0]
    out = resample_train.resized_features_train(x, _dev(case[1]), _dev(case[2]), _dev(case[3]), *[_dev(t) for t in params], size, 3)
    upstream = go.clone().requires_grad_(True)          # (a gradient that depends on a leaf: there is something to differentiate twice)
    g, = torch.autograd.grad((out * upstream).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- 2. upsample_residual_train -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full,reduced", UPSAMPLE, ids=lambda p: "x".join(map(str, p)))
def test_upsample_gradients_against_float64(full, reduced):
    h, w = full
    rng = np.random.default_rng(1000 * h + w)
    res = (0.2 * rng.standard_normal((3,) + reduced)).astype(np.float32)
    render = rng.random((3, h, w)).astype(np.float32)
    g_up, g_pred = (rng.standard_normal((3, h, w)).astype(np.float32) for _ in range(2))
    failed = []
    for scale in (1.0, 0.5, 0.0):
        for a, b, which in ((g_up, None, "residual_up"), (None, g_pred, "image_pred"), (g_up, g_pred, "both")):
            want = tr.upsample_grads(res, render, scale, a, b)
            t32 = tr.upsample_grads(res, render, scale, a, b, torch.float32, interpolate=True)
            twin = tr.upsample_grads(res, render, scale, a, b, torch.float32)
            r_d, x_d = _leaves([torch.as_tensor(res), torch.as_tensor(render)])
            up, pred = resample_train.upsample_residual_train(r_d, x_d, scale)
            with torch.no_grad():
                plain = resample.upsample_residual(r_d.detach(), x_d.detach(), scale)
            assert torch.equal(up, plain[0]) and torch.equal(pred, plain[1])
            loss = (0 if a is None else (up * _dev(a)).sum()) + (0 if b is None else (pred * _dev(b)).sum())
            loss.backward()
            torch.cuda.synchronize()
            tag = "%dx%d -> %dx%d scale %.1f upstream %s " % (reduced + full + (scale, which))
            _compare(tag + "residual", r_d.grad, want["residual"], t32["residual"], twin["residual"], failed)
            if b is None:
                assert x_d.grad is None
            else:
                assert torch.equal(x_d.grad, scale * _dev(b))          # render's share: torch's product
    assert not failed, failed


# ---- 3. end to end on the fixture scene ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    z, planes, mlp, cnn = fixture()
    made = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consumer_resized.npz"))
    pkg = {"render": _dev(planes["color"]), "warped_image": _dev(planes["warped_image"]), "cam_feat": _dev(planes["cam_feat"]), "camera_ray": _dev(planes["camera_ray"]),
           "min_depth_diff": _dev(planes["min_depth_diff"]), "use_first_src_frame_mask": _dev(planes["use_first_src_frame_mask"])}
    net = hourglass.ColorAggregationNet()
    net.load_state_dict({k[3:]: torch.tensor(made[k]) for k in made.files if k.startswith("sd/")})
    return z, planes, mlp, cnn, pkg, net.cuda()


@functools.lru_cache(maxsize=None)
def _tail_cpu(expo, burned, images):
    z, planes, mlp, cnn = _scene()[:4]
    kw = dict(burned=burned, expo=expo, images=images)
    want, pred = tr.tail_grads(planes, mlp, cnn, (16, 24), z["g"], **kw)
    t32, _ = tr.tail_grads(planes, mlp, cnn, (16, 24), z["g"], dtype=torch.float32, interpolate=True, **kw)
    twin, _ = tr.tail_grads(planes, mlp, cnn, (16, 24), z["g"], dtype=torch.float32, **kw)
    return want, t32, twin, pred


def _params_of(net):
    named = {k: getattr(net.front_end, k) for k in ("w1", "b1", "w2", "b2")}
    named.update({k: getattr(net.cnn, k) for k in CNN_NAMES})
    return named


def _tail_run(pkg, net, g, **kw):
    """-> (the dictionary, {name: gradient}) of fuse_color_train_scaled at 0.5 with fresh image leaves and cleared parameter gradients"""
    live = dict(pkg, render=pkg["render"].detach().clone().requires_grad_(True), warped_image=pkg["warped_image"].detach().clone().requires_grad_(True))
    for p in net.parameters():
        p.grad = None
    out = resample_train.fuse_color_train_scaled(live, net, 0.5, 3, **kw)
    (out["image_pred"] * g).sum().backward()
    grads = {"render": live["render"].grad, "warped": live["warped_image"].grad}
    grads.update({k: p.grad for k, p in _params_of(net).items()})
    return out, grads


@pytest.mark.parametrize("expo", [False, True], ids=["plain", "exposure"])
def test_fuse_color_train_scaled_on_the_fixture_scene(expo):
    z, planes, _, _, pkg, net = _scene()
    g = _dev(z["g"])
    want, t32, twin, pred = _tail_cpu(expo, 1.0, True)
    out, grads = _tail_run(pkg, net, g, enable_exposure_correction=expo)
    with torch.no_grad():
        test_time = hourglass.fuse_color(pkg, net, 3, residual_resolution_scale=0.5, enable_exposure_correction=expo)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(test_time) and out["burned_in_gauss"] == 1.0 and int(out["nb_valid_warp_level"]) == 3
    for k in test_time:          # the forward is fuse_color's at the same scale: every key, every bit
        assert torch.equal(out[k], test_time[k]) if torch.is_tensor(out[k]) else out[k] == test_time[k], k
    assert float((out["image_pred"].detach().double().cpu() - torch.as_tensor(pred)).abs().max()) < 1e-4
    failed = []
    for k in ["render", "warped", "w1", "b1", "w2", "b2"] + CNN_NAMES:
        _compare("fuse_color_train_scaled 32x48 s 0.5 %s %s" % ("exposure" if expo else "plain", k), grads[k], want[k], t32[k], twin[k], failed)
    assert not failed, failed


def test_burn_in_blocks_the_image_gradients_and_trains_the_parameters():
    z, _, _, _, pkg, net = _scene()
    g = _dev(z["g"])
    want, t32, twin, _ = _tail_cpu(False, 0.75, False)
    out, grads = _tail_run(pkg, net, g, iter_count=5, burn_start=0, burn_end=10)
    torch.cuda.synchronize()
    assert out["burned_in_gauss"] == 0.75 and grads["render"] is None and grads["warped"] is None
    failed = []
    for k in ["w1", "b1", "w2", "b2"] + CNN_NAMES:
        _compare("burn-in 0.75 %s" % k, grads[k], want[k], t32[k], twin[k], failed)
    assert not failed, failed


# ---- 4. bit for bit ------------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]), k


def test_exact_properties():
    z, _, _, _, pkg, net = _scene()
    g = _dev(z["g"])
    before = {k: v.clone() for k, v in pkg.items()}
    p0 = [p.detach().clone() for p in net.parameters()]
    for expo in (False, True):
        kw = dict(enable_exposure_correction=expo)
        out, grads = _tail_run(pkg, net, g, **kw)
        again, grads_again = _tail_run(pkg, net, g, **kw)          # a second call
        _same(out, again)
        _same(grads, grads_again)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            on_side, grads_side = _tail_run(pkg, net, g, **kw)
        side.synchronize()
        _same(out, on_side)
        _same(grads, grads_side)
        # a scale == 1, in any spelling, is fuse_color_train itself
        for p in net.parameters():
            p.grad = None
        for one in (1, 1.0):
            _same(resample_train.fuse_color_train_scaled(pkg, net, one, 3, **kw), hourglass.fuse_color_train(pkg, net, 3, **kw))
        # the composition by hand
        render = exposure.exposure_correct(pkg["render"], pkg["warped_image"], pkg["use_first_src_frame_mask"])[0] if expo else pkg["render"]
        front = net.front_end
        x = resample_train.resized_features_train(render, pkg["warped_image"], pkg["cam_feat"], pkg["camera_ray"], front.w1, front.b1, front.w2, front.b2, (16, 24),
                                                  resample.count_levels(pkg["warped_image"], 3), front.mode)
        up, pred = resample_train.upsample_residual_train(hourglass.hourglass_train(x, net.cnn), render, 1.0)
        assert torch.equal(out["residual"], up) and torch.equal(out["image_pred"], pred)
    assert int(resample_train.fuse_color_train_scaled(pkg, net, 0.5, 2)["nb_valid_warp_level"]) == 2
    empty = dict(pkg, warped_image=torch.zeros_like(pkg["warped_image"]))
    none = resample_train.fuse_color_train_scaled(empty, net, 0.5, 3)
    assert int(none["nb_valid_warp_level"]) == 0 and resample_train.fuse_color_train_scaled(empty, net, 0.5, 3, none_if_no_level=True) is None
    (none["image_pred"] * g).sum().backward()          # every source slot zeroed: nothing raises
    torch.cuda.synchronize()
    assert all(torch.equal(pkg[k], before[k]) for k in pkg) and all(torch.equal(p, q) for p, q in zip(net.parameters(), p0))


def test_dirty_guard_banded_buffers():
    """tests/dirty_alloc.py: every torch.empty of the wrappers served from 0x00, 0xFF and 0x40 bytes between guards: the same bits (gradients included), no NaN,
    guards intact."""
    z, _, _, _, pkg, net = _scene()
    g = _dev(z["g"])

    def tail():
        out, grads = _tail_run(pkg, net, g, enable_exposure_correction=True)
        assert out.pop("burned_in_gauss") == 1.0          # (a float: the rest are tensors)
        return out, grads
    # forward: the correction (corrected, affine, fit_ok, its arena), the levels and their arena, cnn_input, the hourglass (residual, its arena), the two outputs;
    # backward: the residual's gradient; the hourglass (grad_x, 18 gradients, its arena); this unit (6 gradients, its arena); the correction's (1)
    da.check("fuse_color_train_scaled 32x48 s 0.5, forward and backward", tail, DEV, (4 + 2 + 1 + 2 + 2) + 1 + 20 + 7 + 1)
    for h, w, s in ((9, 11, 0.5), (35, 37, 0.5)):
        case, params, size, go = _case(h, w, s)
        go = go.to(DEV)
        res = torch.rand((3,) + size, generator=torch.Generator().manual_seed(h))
        g_full = torch.rand(3, h, w, generator=torch.Generator().manual_seed(w)).to(DEV)

        def units():
            outs = [_feature_run(case, params, size, 3, mode, go) for mode in ("mean", "max")]
            r_d, x_d = _leaves([res, case[0]])
            up, pred = resample_train.upsample_residual_train(r_d, x_d, 0.5)
            ((up + pred) * g_full).sum().backward()
            return outs, up.detach(), pred.detach(), r_d.grad, x_d.grad
        # per mode: cnn_input, 6 gradients and the arena; the two outputs and the residual's gradient
        da.check("resized_features_train + upsample_residual_train %dx%d s %.2f, forward and backward" % (h, w, s), units, DEV, 2 * (1 + 7) + 2 + 1)
