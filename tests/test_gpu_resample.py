"""The reduced-resolution colour tail (ibgs_amd.resample; csrc/resample.hip; `hourglass.fuse_color(..., residual_resolution_scale=s)`) on the device.

The ARBITER is tests/resample_ref (float64 numpy, explicit taps and weights), with tests/hourglass_ref.forward_ref in the middle for the whole tail.  The
YARDSTICK of a tensor is d_ref = max of the max-abs distances from the arbiter of two float32 evaluations ON THE CPU on the same inputs: torch's own
composition (F.interpolate, Linear; for the fixture scene the reference's recorded run) and a sequential float32 chain (tests/resample_ref.chain_f32,
tests/hourglass_ref.chain_f32).  `upsample_residual` has torch's float32 F.interpolate alone, as its whole work is that one call.  THE BAR, as in
tests/test_gpu_hourglass.py: max |hip - f64| <= F64_K x d_ref (F64_K = 2); where d_ref is exactly 0: 2^-22 max |f64|.  Every comparison prints its ratio before it
asserts (DESIGN.md section 19 quotes the range); bit-for-bit properties are asserted with torch.equal.

The grid of neither kernel is capped (a wave per 32 reduced pixels; a thread per 4 output columns), so no frame lies beyond one pass of it."""
import functools
import os

import numpy as np
import pytest
import torch

from ibgs_amd import coloragg, hourglass, resample
from tests import dirty_alloc as da
from tests import exposure_ref
from tests import hourglass_ref
from tests import resample_ref as ref

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
# (H, W, s): the smallest; odd sizes; steps of exactly 2 (every weight 0 or 1, the last row and column on the clamp); a full wave block with a non-integer
# step; a non-integer ratio; upscaling; pixel counts that do not fill a wave's block
FRAMES = [(8, 8, 0.5), (9, 11, 0.5), (9, 13, 0.56), (33, 65, 0.5), (32, 48, 0.75), (32, 48, 1.5), (35, 37, 0.5)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = (("features", slice(0, 32)), ("ray", slice(32, 35)), ("colour", slice(35, 38)))
DEV = "cuda"


def _dev(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def _check(name, got, want64, d):
    want = torch.as_tensor(np.asarray(want64), dtype=torch.float64, device=got.device)
    assert got.dtype == torch.float32 and got.shape == want.shape, (name, got.dtype, tuple(got.shape), tuple(want.shape))
    err = float((got.double() - want).abs().max())
    print("%-64s err %.3e  d_ref %.3e  ratio %s" % (name, err, d, "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= F64_K * d, (name, err, d)
    else:
        assert err <= FLOOR * float(want.abs().max()), (name, err)


# ---- the CPU evaluations, computed once and shared: nobody writes them -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(h, w):
    case, params = ref.seeded_case(h, w)
    v = ref.coloragg_ref.valid_ref(case[2])
    assert not v[1].any() and all((v[k][:, 1:] != v[k][:, :-1]).mean() > 0.2 for k in (0, 2))          # validity varies between neighbours; one slot all-invalid
    return case, params, tuple(t.to(DEV) for t in case), tuple(t.to(DEV) for t in params)


@functools.lru_cache(maxsize=None)
def _features_cpu(h, w, s, mode, levels):
    """-> (arbiter (1, 38, Hr, Wr), {group: d_ref}, the level count used)"""
    case, params = _case(h, w)[:2]
    size = ref.scaled_size(h, w, s)
    want, lv = ref.features_ref(*case, *params, size, mode=mode, levels=levels)
    t32 = ref.torch_composition(*case, *params, size, mode=mode, dtype=torch.float32, levels=levels).numpy().astype(np.float64)
    chain = ref.chain_f32(*case, *params, size, mode=mode, levels=levels).astype(np.float64)
    d = {g: max(float(np.abs(t32[0, sl] - want[0, sl]).max()), float(np.abs(chain[0, sl] - want[0, sl]).max())) for g, sl in GROUPS}
    return want, d, lv


def _features_parity(h, w, s, mode, levels_arg, levels_ref):
    _, _, case, params = _case(h, w)
    size = ref.scaled_size(h, w, s)
    want, d, lv = _features_cpu(h, w, s, mode, levels_ref)
    with torch.no_grad():
        got = resample.resized_features(*case, *params, size, levels_arg, mode)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 38) + size
    failed = []
    for g, sl in GROUPS:          # every group is printed before the first failure is raised
        try:
            _check("%dx%d s %.2f -> %dx%d %s levels %s %s" % (h, w, s, size[0], size[1], mode, lv, g), got[0, sl], want[0, sl], d[g])
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]
    return got, lv


# ---- 1. resized_features ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d_s%g" % f)
def test_resized_features_against_float64(frame, mode):
    h, w, s = frame
    _, _, case, _ = _case(h, w)
    counted = resample.count_levels(case[1], 3)          # the device word of ibgs_cagg_levels, at full resolution
    got, lv = _features_parity(h, w, s, mode, counted, None)
    assert int(counted) == lv == 3
    if frame == (9, 13, 0.56):          # steps of exactly 2: the colour is the tap itself
        assert torch.equal(got[0, 35:], case[0][:, ::2, ::2])


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("frame", [(5, 7), (9, 29)], ids=lambda f: "%dx%d" % f)
def test_at_the_frames_own_size_it_is_the_front_end_bit_for_bit(frame, mode):
    """resample.hip and coloragg.hip run ONE per-view chain (csrc/shared/pv_mlp.h).  At size == (H, W) every tap has t = 0 and u = 1, and fma(0, b, 1 a) = a for
    finite inputs: the blended slot is the slot, so the aggregate (channels 0 .. 31) and the colour (35 .. 37) must be `per_view_features`'s to the bit.  The ray
    channels are not compared: the resampled ray is normalised.  5 x 7: one partial wave; 9 x 29 = 261 pixels: three workgroups, the last wave partial."""
    h, w = frame
    g = torch.Generator().manual_seed(100 * h + w)
    r = lambda *shape: torch.randn(*shape, generator=g)
    render, warped, feat, ray = r(3, h, w), r(9, h, w), r(12, h, w), r(3, h, w)          # cam_feat signed: about half of every slot's pixels are masked
    params = (r(32, 7) / 7 ** 0.5, r(32) / 4, r(32, 32) / 32 ** 0.5, r(32) / 4)
    valid = feat.view(3, 4, h, w).sum(1) > 0
    assert all(0.25 < float(v.float().mean()) < 0.75 for v in valid)
    args = tuple(t.to(DEV) for t in (render, warped, feat, ray) + params)
    for levels in (0, 2, 3):
        with torch.no_grad():
            mine = resample.resized_features(*args, (h, w), levels, mode)
            theirs, _ = coloragg.per_view_features(*args, mode=mode, levels=levels)
        torch.cuda.synchronize()
        assert mine.shape == theirs.shape == (1, 38, h, w) and bool(torch.isfinite(mine).all())
        assert torch.equal(mine[0, :32], theirs[0, :32]) and torch.equal(mine[0, 35:], theirs[0, 35:]), (frame, mode, levels)
        assert bool(mine[0, :32].any()) == (levels > 0) and torch.equal(theirs[0, 35:], args[0])


@pytest.mark.parametrize("frame", [(9, 11, 0.5), (35, 37, 0.5)], ids=lambda f: "%dx%d_s%g" % f)
def test_levels(frame):
    """0 (the aggregated channels exactly zero, ray and colour still written), 1, S, as ints and as a device word the caller filled; words outside 0 .. S are
    clamped."""
    h, w, s = frame
    for mode in ("mean", "max"):
        full = None
        for levels in (0, 1, 3):
            got, lv = _features_parity(h, w, s, mode, levels, levels)
            assert lv == levels
            word = torch.full((), levels, dtype=torch.int32, device=DEV)
            with torch.no_grad():
                again = resample.resized_features(*_case(h, w)[2], *_case(h, w)[3], ref.scaled_size(h, w, s), word, mode)
            assert torch.equal(again, got) and int(word) == levels
            if levels == 0:
                assert float(got[0, :32].abs().max()) == 0.0 and float(got[0, 35:].abs().max()) > 0
                assert torch.allclose(got[0, 32:35].square().sum(0), torch.ones((), device=DEV), atol=1e-5)
            full = got if levels == 3 else full
        with torch.no_grad():
            for word, same_as in ((7, full), (-2, None)):
                out = resample.resized_features(*_case(h, w)[2], *_case(h, w)[3], ref.scaled_size(h, w, s), torch.full((), word, dtype=torch.int32, device=DEV), mode)
                assert torch.equal(out, full) if same_as is not None else float(out[0, :32].abs().max()) == 0.0


# ---- 2. upsample_residual ------------------------------------------------------------------------------------------------------------------------------------
UPSAMPLE = [((h, w), ref.scaled_size(h, w, s)) for h, w, s in FRAMES] + [((9, 11), (1, 5)), ((9, 12), (4, 1)), ((6, 7), (1, 1)), ((1, 1), (4, 5)), ((1, 9), (4, 5))]


@pytest.mark.parametrize("full,reduced", UPSAMPLE, ids=lambda p: "x".join(map(str, p)))
def test_upsample_residual_against_float64(full, reduced):
    h, w = full
    g = np.random.default_rng(1000 * h + w)
    res = (0.2 * g.standard_normal((3,) + reduced)).astype(np.float32)
    render = g.random((3, h, w)).astype(np.float32)
    res_d, render_d = _dev(res), _dev(render)
    for scale in (1.0, 0.5, 0.0):
        want_up, want_pred = ref.upsample_ref(res, render, scale)
        t_up, t_pred = ref.torch_upsample(res, render, scale)
        d_up, d_pred = (float(np.abs(t.numpy().astype(np.float64) - want).max()) for t, want in ((t_up, want_up), (t_pred, want_pred)))
        with torch.no_grad():
            up, pred = resample.upsample_residual(res_d, render_d, scale)
        torch.cuda.synchronize()
        tag = "%dx%d -> %dx%d scale %.1f" % (reduced + full + (scale,))
        _check(tag + " residual", up, want_up, d_up)
        _check(tag + " image_pred", pred, want_pred, d_pred)
        assert torch.equal(pred, scale * render_d + up)          # torch's expression on the returned residual, bit for bit
    if reduced == (1, 1):
        assert torch.equal(up, res_d.expand(3, h, w))
    # (the 16-byte path serves the widths above that are a multiple of 4 -- 8, 48, 12 --, the 4-byte path the others)


# ---- 3. end to end on the fixture scene ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    z, c = np.load(os.path.join(GOLDEN, "consumer_resized.npz")), np.load(os.path.join(GOLDEN, "consumer.npz"))
    planes = {k: c["oracle_" + k] for k in ("color", "warped_image", "cam_feat", "camera_ray", "min_depth_diff", "use_first_src_frame_mask")}
    pkg = {"render": _dev(planes["color"]), "warped_image": _dev(planes["warped_image"]), "cam_feat": _dev(planes["cam_feat"]), "camera_ray": _dev(planes["camera_ray"]),
           "min_depth_diff": _dev(planes["min_depth_diff"]), "use_first_src_frame_mask": _dev(planes["use_first_src_frame_mask"])}
    sd = {k[3:]: torch.tensor(z[k]) for k in z.files if k.startswith("sd/")}
    net = hourglass.ColorAggregationNet()
    net.load_state_dict(sd)
    mlp = tuple(sd["per_view_mlp." + k].numpy() for k in ("0.weight", "0.bias", "2.weight", "2.bias"))
    cnn = {mine: sd["conv_decoder." + theirs].numpy() for theirs, mine in hourglass.REFERENCE_KEYS.items()}
    return z, planes, pkg, net.cuda().requires_grad_(False), mlp, cnn


@functools.lru_cache(maxsize=None)
def _tail_cpu(tag, s, expo):
    """-> ({"residual", "image_pred"} arbiter, {..} d_ref, {..} (d_recorded, d_chain))"""
    z, planes, _, _, mlp, cnn = _fixture()
    h, w = planes["color"].shape[-2:]
    size = ref.scaled_size(h, w, s)
    render = exposure_ref.correct_ref(planes["color"], planes["warped_image"], planes["use_first_src_frame_mask"])[0] if expo else planes["color"].astype(np.float64)
    x, lv = ref.features_ref(render, planes["warped_image"], planes["cam_feat"], planes["camera_ray"], *mlp, size)
    assert lv == 3
    want = dict(zip(("residual", "image_pred"), ref.upsample_ref(hourglass_ref.forward_ref(x, cnn)["residual"], render, 1.0)))
    r32 = render.astype(np.float32)
    x32 = ref.chain_f32(r32, planes["warped_image"], planes["cam_feat"], planes["camera_ray"], *mlp, size)
    chain = dict(zip(("residual", "image_pred"), ref.upsample_ref(hourglass_ref.chain_f32(x32, cnn)["residual"], r32, 1.0, np.float32)))
    both = {k: (float(np.abs(z[tag + "_" + k].astype(np.float64) - want[k]).max()), float(np.abs(chain[k].astype(np.float64) - want[k]).max())) for k in want}
    return want, {k: max(v) for k, v in both.items()}, both


@pytest.mark.parametrize("tag,s,expo", [("half", 0.5, False), ("half_exposure", 0.5, True), ("three_quarters", 0.75, False), ("three_halves", 1.5, False)])
def test_fuse_color_on_the_fixture_scene(tag, s, expo):
    z, planes, pkg, net, _, _ = _fixture()
    want, d_ref, both = _tail_cpu(tag, s, expo)
    with torch.no_grad():
        out = hourglass.fuse_color(pkg, net, 3, residual_resolution_scale=s, enable_exposure_correction=expo)
        via_module = net(pkg, 3, residual_resolution_scale=s, enable_exposure_correction=expo)
    torch.cuda.synchronize()
    keys = ["burned_in_gauss", "image_pred", "nb_valid_warp_level", "residual", "valid_warp_mask", "warped_image_list"] + (["exposure_affine", "exposure_fit_ok"] if expo else [])
    assert sorted(out) == sorted(keys) == sorted(via_module)
    h, w = 32, 48
    assert tuple(out["residual"].shape) == tuple(out["image_pred"].shape) == (3, h, w) and out["burned_in_gauss"] == 1.0
    lv = out["nb_valid_warp_level"]
    assert lv.is_cuda and lv.dtype == torch.int32 and lv.dim() == 0 and int(lv) == 3
    assert torch.equal(out["valid_warp_mask"], (pkg["min_depth_diff"] < 0.999).float()) and tuple(out["valid_warp_mask"].shape) == (1, h, w)
    assert torch.equal(out["warped_image_list"], pkg["warped_image"].view(-1, 3, h, w)[:3].permute(2, 3, 0, 1))
    for k in keys:
        assert torch.equal(out[k], via_module[k]) if torch.is_tensor(out[k]) else out[k] == via_module[k], k
    failed = []
    for k in ("residual", "image_pred"):
        print("%s: the reference's recorded float32 run is %.3e from float64, the float32 chain %.3e" % ((tag + " " + k,) + both[k]))
        try:
            _check("fuse_color %s s %.2f %s" % (tag, s, k), out[k], want[k], d_ref[k])
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]


# ---- 4. bit for bit --------------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


def test_exact_properties():
    _, _, pkg, net, _, _ = _fixture()
    before = {k: v.clone() for k, v in pkg.items()}
    p0 = [p.detach().clone() for p in net.parameters()]
    with torch.no_grad():
        for expo in (False, True):
            kw = dict(burned_in_gauss=0.75, enable_exposure_correction=expo)
            plain = hourglass.fuse_color(pkg, net, 3, **kw)
            for one in (1, 1.0):          # s = 1 is the present path: every bit and key
                _same(hourglass.fuse_color(pkg, net, 3, residual_resolution_scale=one, **kw), plain)
            half = hourglass.fuse_color(pkg, net, 3, residual_resolution_scale=0.5, **kw)
            assert not torch.equal(half["residual"], plain["residual"])
            _same(hourglass.fuse_color(pkg, net, 3, residual_resolution_scale=0.5, **kw), half)          # a second call
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                on_side = hourglass.fuse_color(pkg, net, 3, residual_resolution_scale=0.5, **kw)
            side.synchronize()
            _same(on_side, half)
            # the composition by hand, in both precisions
            render = half_render = pkg["render"]
            if expo:
                from ibgs_amd import exposure
                half_render = exposure.exposure_correct(render, pkg["warped_image"], pkg["use_first_src_frame_mask"])[0]
            for precision in ("float32", "float16"):
                got = hourglass.fuse_color(pkg, net, 3, precision=precision, residual_resolution_scale=0.5, **kw)
                front = net.front_end
                x = resample.resized_features(half_render, pkg["warped_image"], pkg["cam_feat"], pkg["camera_ray"], front.w1, front.b1, front.w2, front.b2, (16, 24),
                                              resample.count_levels(pkg["warped_image"], 3), front.mode)
                up, pred = resample.upsample_residual(hourglass.hourglass_forward(x, net.cnn, precision=precision), half_render, 0.75)
                assert torch.equal(got["residual"], up) and torch.equal(got["image_pred"], pred), (expo, precision)
                assert torch.equal(pred, 0.75 * half_render + up)
            assert not torch.equal(got["residual"], half["residual"])          # float16 is another result
        # nb_visible_src_frames caps the count at full resolution, as in the present path
        assert int(hourglass.fuse_color(pkg, net, 2, residual_resolution_scale=0.5)["nb_valid_warp_level"]) == 2
        empty = dict(pkg, warped_image=torch.zeros_like(pkg["warped_image"]))
        none = hourglass.fuse_color(empty, net, 3, residual_resolution_scale=0.5)
        assert int(none["nb_valid_warp_level"]) == 0 and hourglass.fuse_color(empty, net, 3, none_if_no_level=True, residual_resolution_scale=0.5) is None
    torch.cuda.synchronize()
    assert all(torch.equal(pkg[k], before[k]) for k in pkg) and all(torch.equal(p, q) for p, q in zip(net.parameters(), p0))


@pytest.mark.parametrize("precision", ["float32", "float16"])
def test_dirty_guard_banded_buffers(precision):
    """tests/dirty_alloc.py: every torch.empty of the wrappers served from 0x00, 0xFF and 0x40 bytes between guards: the same bits, no NaN, guards intact."""
    _, _, pkg, net, _, _ = _fixture()

    def call():
        with torch.no_grad():
            out = hourglass.fuse_color(pkg, net, precision=precision, residual_resolution_scale=0.5, enable_exposure_correction=True)
        assert out.pop("burned_in_gauss") == 1.0          # (a float: the rest are tensors)
        return out
    # the correction: corrected, affine, fit_ok, its arena; the levels and their arena; cnn_input; the hourglass: residual, its arena; the two outputs
    da.check("fuse_color 32x48 s 0.5 %s" % precision, call, DEV, 4 + 2 + 1 + 2 + 2)
    for h, w, s in ((9, 11, 0.5), (35, 37, 0.5), (32, 48, 1.5)):
        _, _, case, params = _case(h, w)
        size = ref.scaled_size(h, w, s)
        res = torch.rand((3,) + size, generator=torch.Generator().manual_seed(h)).to(DEV)

        def units():
            with torch.no_grad():
                return resample.resized_features(*case, *params, size, 3), resample.upsample_residual(res, case[0], 0.5)
        da.check("resized_features + upsample_residual %dx%d s %.2f" % (h, w, s), units, DEV, 1 + 2)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    _, _, pkg, net, _, _ = _fixture()
    live = hourglass.ColorAggregationNet().cuda()
    with pytest.raises(RuntimeError, match=r"fuse_color is forward only.*torch\.no_grad\(\)"):
        hourglass.fuse_color(pkg, live, residual_resolution_scale=0.5)          # a parameter requires grad and grad mode is on
    with torch.no_grad():
        assert tuple(hourglass.fuse_color(pkg, live, residual_resolution_scale=0.5)["residual"].shape) == (3, 32, 48)
        with pytest.raises(ValueError, match=r"residual_resolution_scale 0\.1 turns the frame of 32 x 48 into 3 x 4"):
            hourglass.fuse_color(pkg, net, residual_resolution_scale=0.1)
        with pytest.raises(ValueError, match=r"into 9600 x 14400"):
            hourglass.fuse_color(pkg, net, residual_resolution_scale=300)
        with pytest.raises(RuntimeError, match="MI355X only"):
            resample.upsample_residual(torch.rand(3, 4, 4), pkg["render"])
    _, _, case, params = _case(9, 11)
    with pytest.raises(RuntimeError, match="resized_features is forward only"):
        resample.resized_features(*case, params[0].clone().requires_grad_(True), *params[1:], (4, 5), 3)
