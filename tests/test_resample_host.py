"""The reduced-resolution colour tail on a CPU-only box: the C ABI (include/ibgs_resample.h <-> _lib.RSZ_EXPORTS <-> the built library), the build
registration, the entry points' validation with null pointers and bad sizes, the argument checks of ibgs_amd.resample and of the fuse_color keyword (which
run before any GPU work), and the float64 restatement (tests/resample_ref.py) against torch's own float64 F.interpolate composition, against the recorded
run of the reference's fuse_color at residual_resolution_scale 0.5 (tests/golden/consumer_resized.npz), and against the wrong order of masking and
interpolation."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, coloragg, hourglass, resample
from tests import exposure_ref
from tests import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "resample.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["ibgs_rsz_features_forward", "ibgs_rsz_residual_upsample"]
# (H, W, s): the frames of tests/test_gpu_resample.py
FRAMES = [(8, 8, 0.5), (9, 11, 0.5), (9, 13, 0.56), (33, 65, 0.5), (32, 48, 0.75), (32, 48, 1.5), (35, 37, 0.5)]


# ---- 1. the ABI and the build ----------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_resample.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.RSZ_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
        assert re.search(r"%s\(void\* stream," % n, text), n          # the stream first, like the other unit headers
    defines = dict(re.findall(r"#define\s+IBGS_(RSZ_[A-Z_]+)\s+(\d+)", text))
    assert sorted(defines) == ["RSZ_FEATURES", "RSZ_MAX", "RSZ_MAX_SIDE", "RSZ_MAX_SRC", "RSZ_MEAN"]
    for name, val in defines.items():
        assert getattr(_lib, name) == int(val), name
    # the front end's constants, restated: the two units serve the same network
    assert (_lib.RSZ_MAX_SRC, _lib.RSZ_FEATURES, _lib.RSZ_MEAN, _lib.RSZ_MAX) == (_lib.CAGG_MAX_SRC, _lib.CAGG_FEATURES, _lib.CAGG_MEAN, _lib.CAGG_MAX)
    others = (_lib.EXPORTS + _lib.SSIM_EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS + _lib.GEOLOSS_EXPORTS
              + _lib.CAGG_EXPORTS + _lib.HG_EXPORTS + _lib.HGB_EXPORTS + _lib.HGH_EXPORTS + _lib.LPIPS_EXPORTS + _lib.EXPO_EXPORTS)
    assert not any("rsz" in n for n in others)


def test_unit_is_registered_and_its_kernels_attributed():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["rsz_features_kernel", "rsz_upsample_kernel"]
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "resample"]
    for k in kernels:
        assert _build.tu_of(k) == "resample", k
        assert not any(sub in k for sub in others), k          # whatever the order of the table
    assert [e for e in _build.KERNEL_TU if e[1] == "resample"] == [("rsz_", "resample")]
    assert "resample" in _build.SOURCES and "resample" in _build.UNIT_HEADERS and "resample" in _build.tu_shas()
    assert _build.SOURCES[-1] == "hourglass" and _build.KERNEL_TU[0] == ("meval_", "mesh_eval")
    assert "resample" not in _build.EXTRA and _build.compile_flags("resample") == _build.compile_flags("ssim") == _build.compile_flags("coloragg")
    # no kernel of another unit is claimed by the new entry
    for name in _build.SOURCES:
        if name != "resample":
            text = open(os.path.join(ROOT, "ibgs_amd", "csrc", name + ".hip")).read()
            for k in re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", text):
                assert "rsz_" not in k, (name, k)
    code = _build._code_only(src)
    assert "atomic" not in code.lower()          # every output element is one thread's own chain
    # the MLP chain is the one coloragg.hip runs, the tap and value rule the one rsztrain.hip runs; forward only: the backward's header is not compiled here
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "shared/pv_mlp.h", "shared/rsz_taps.h", "../../include/ibgs_resample.h"]
    assert [os.path.basename(h) for h in _build.UNIT_HEADERS["resample"]] == ["ibgs_resample.h", "pv_mlp.h", "rsz_taps.h"] and all(os.path.exists(h) for h in _build.UNIT_HEADERS["resample"])
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc")) if f.endswith(".h")) == ["adam_math.h", "blend.h", "block_ops.h", "common.h", "sh_color.h", "wave_bits.h", "wave_reduce.h"]
    assert sorted(os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc", "shared"))) == ["conv_tile.h", "conv_tile_f16.h", "hg_net.h", "pv_mlp.h", "pv_mlp_bwd.h", "rsz_taps.h", "ssim_window.h"]
    chain = _build._code_only(open(os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "pv_mlp.h")).read())
    assert re.search(r"__builtin_amdgcn_mfma_f32_32x32x2f32", chain) and not re.search(r"mfma", code.replace("pv_mfma", ""))
    assert re.search(r"pv_mlp\(", code) and re.search(r"pv_slot\(", code)
    assert re.search(r"constexpr int RT = 256;", code) and re.search(r"constexpr int RB = 32;", code) and re.search(r"constexpr int RQ = 4;", code)


def test_validation_before_any_gpu_work(built_lib):
    err = lambda: built_lib.ibgs_last_error()
    fwd, up = built_lib.ibgs_rsz_features_forward, built_lib.ibgs_rsz_residual_upsample
    # forward: (stream, S, H, W, Hr, Wr, mode, render, warped, feat, ray, w1, b1, w2, b2, levels, out)
    good = [None, 3, 8, 8, 4, 4, 0] + [128] * 10
    for k, v, msg in ((1, 0, b"sources"), (1, 6, b"sources"), (2, 0, b"a frame of"), (3, 65537, b"a frame of"), (4, 0, b"a reduced frame of"), (5, 65537, b"a reduced frame of"),
                      (4, -1, b"a reduced frame of")):
        args = list(good)
        args[k] = v
        assert fwd(*args) < 0 and b"rsz_features_forward" in err() and b"out of range" in err() and msg in err(), (k, v)
    for v in (2, -1):
        args = list(good)
        args[6] = v
        assert fwd(*args) < 0 and b"mode" in err()
    for ks, msg in (((7, 8, 9, 10), b"null image"), ((11, 12, 13, 14), b"null parameters"), ((15,), b"null levels"), ((16,), b"null outputs")):
        for k in ks:
            args = list(good)
            args[k] = None
            assert fwd(*args) < 0 and msg in err(), k
    # upsample: (stream, H, W, Hr, Wr, residual_r, render, render_scale, residual_out, image_pred_out)
    good = [None, 8, 8, 4, 4, 128, 128, 1.0, 128, 128]
    for k, v, msg in ((1, 0, b"a frame of"), (2, 65537, b"a frame of"), (3, 0, b"a reduced frame of"), (4, 65537, b"a reduced frame of")):
        args = list(good)
        args[k] = v
        assert up(*args) < 0 and b"rsz_residual_upsample" in err() and b"out of range" in err() and msg in err(), (k, v)
    for ks, msg in (((5, 6), b"null image"), ((8, 9), b"null outputs")):
        for k in ks:
            args = list(good)
            args[k] = None
            assert up(*args) < 0 and msg in err(), k


# ---- 2. the size and coordinate rules ------------------------------------------------------------------------------------------------------------------------
def test_size_rule_and_taps():
    assert [ref.scaled_size(h, w, s) for h, w, s in FRAMES] == [(4, 4), (4, 5), (5, 7), (16, 32), (24, 36), (48, 72), (17, 18)]
    for h, w, s in FRAMES + [(1080, 1920, 0.5), (720, 1280, 0.3), (7, 9, 0.99)]:
        assert resample.scaled_size(h, w, s) == ref.scaled_size(h, w, s) == (int(h * s), int(w * s))
        out = torch.nn.functional.interpolate(torch.zeros(1, 1, h, w), scale_factor=s, mode="bilinear", align_corners=True)
        assert tuple(out.shape[-2:]) == resample.scaled_size(h, w, s), (h, w, s)
    # 9 -> 5 and 13 -> 7: steps of exactly 2, every weight 0, the last index on the last tap's clamp
    for n_in, n_out in ((9, 5), (13, 7)):
        i0, i1, t = ref.taps(n_in, n_out)
        assert np.array_equal(i0, 2 * np.arange(n_out)) and not t.any() and i0[-1] == n_in - 1 == i1[-1]
    i0, i1, t = ref.taps(33, 16)          # a non-integer step: 32 / 15
    assert np.array_equal(i0, np.arange(16) * 32 // 15) and np.allclose(i0 + t, np.arange(16) * 32 / 15, rtol=0, atol=1e-14) and (t[1:-1] > 0).all()
    for n_in in (1, 5):          # one output: coordinate 0
        i0, i1, t = ref.taps(n_in, 1)
        assert i0.tolist() == [0] and t.tolist() == [0.0] and i1.tolist() == [min(1, n_in - 1)]
    i0, i1, t = ref.taps(1, 6)          # one input: every output reads it
    assert not i0.any() and not i1.any() and not t.any()


# ---- 3. the restatement against torch's float64 composition ----------------------------------------------------------------------------------------------
_case = ref.seeded_case


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_restatement_agrees_with_torch_in_float64(mode):
    """Values are O(1) and pass through about ten float64 operations: 1e-12 max."""
    for h, w, s in FRAMES:
        case, params = _case(h, w)
        size = ref.scaled_size(h, w, s)
        v = ref.coloragg_ref.valid_ref(case[2])
        assert not v[1].any() and all((v[k][:, 1:] != v[k][:, :-1]).mean() > 0.2 for k in (0, 2))
        for levels in (None, 0, 1):
            want, lv = ref.features_ref(*case, *params, size, mode=mode, levels=levels)
            theirs = ref.torch_composition(*case, *params, size, mode=mode, dtype=torch.float64, levels=levels).numpy()
            d = np.abs(want - theirs).max()
            print("%dx%d s %.2f %s levels %s: restatement against torch float64 %.3e (max %.3f)" % (h, w, s, mode, lv, d, np.abs(want).max()))
            assert want.shape == (1, 38) + size and d <= 1e-12 * np.abs(want).max()
            if lv == 0:
                assert not want[0, :32].any() and want[0, 32:].any()
        res = np.random.default_rng(h).standard_normal((3,) + size)
        for scale in (1.0, 0.5, 0.0):
            up, pred = ref.upsample_ref(res, case[0], scale)
            t_up, t_pred = ref.torch_upsample(res, case[0], scale, torch.float64)
            assert np.abs(up - t_up.numpy()).max() <= 1e-12 * np.abs(up).max() and np.abs(pred - t_pred.numpy()).max() <= 1e-12 * np.abs(pred).max()
    # one row or one column of residual: every output reads it
    for size in ((1, 5), (5, 1), (1, 1)):
        res = np.random.default_rng(3).standard_normal((3,) + size)
        up, _ = ref.upsample_ref(res, np.zeros((3, 6, 7)))
        t_up, _ = ref.torch_upsample(res, np.zeros((3, 6, 7)), 1.0, torch.float64)
        assert np.abs(up - t_up.numpy()).max() <= 1e-12 * np.abs(up).max()


# ---- 4. the restatement against the reference's recorded run --------------------------------------------------------------------------------------------
def _fixture():
    z, c = np.load(os.path.join(GOLDEN, "consumer_resized.npz")), np.load(os.path.join(GOLDEN, "consumer.npz"))
    planes = {k: c["oracle_" + k] for k in ("color", "warped_image", "cam_feat", "camera_ray", "use_first_src_frame_mask")}
    return z, planes


def test_restatement_reproduces_the_reference_run_and_tells_the_order():
    """Torch's float32 source coordinate, up to 72, has an ulp of 7.6e-6 and multiplies differences of at most 2 max: the bar is 1e-4 max; a layout or order
    mistake is of order max.  Interpolating the images first must lie more than 100 times the recording's own distance away."""
    z, planes = _fixture()
    h, w = int(z["H"]), int(z["W"])
    assert (h, w) == (32, 48) and int(z["half_levels"]) == int(z["half_exposure_levels"]) == 3 == ref.coloragg_ref.levels_ref(planes["warped_image"], 3)
    assert int(z["seed"]) == 4 and z["scales"].tolist() == [0.5, 0.75, 1.5]
    size = ref.scaled_size(h, w, 0.5)
    assert size == (16, 24) == tuple(z["half_size"]) and tuple(z["three_quarters_size"]) == (24, 36) and tuple(z["three_halves_size"]) == (48, 72)
    # a quarter of the horizontally adjacent pixel pairs differ in some slot's validity: the scene tells the two orders apart
    v = ref.coloragg_ref.valid_ref(planes["cam_feat"])[:3]
    assert (v[:, :, 1:] != v[:, :, :-1]).any(0).mean() > 0.2
    corrected = exposure_ref.correct_ref(planes["color"], planes["warped_image"], planes["use_first_src_frame_mask"])[0]
    for tag, render in (("half", planes["color"]), ("half_exposure", corrected)):
        got = ref.x_views_ref(render, planes["warped_image"], planes["cam_feat"], planes["camera_ray"], size, 3)
        wrong = ref.images_first_ref(render, planes["warped_image"], planes["cam_feat"], size, 3)
        for name, mine in zip(("x_views", "ray_dir", "c_3dgs"), got):
            theirs = z[tag + "_" + name].astype(np.float64)
            d, top = np.abs(mine - theirs).max(), np.abs(theirs).max()
            print("%s %s: the recording is %.3e from the restatement (max %.3f)" % (tag, name, d, top))
            assert mine.shape == theirs.shape and d <= 1e-4 * top
        d_right = np.abs(got[0] - z[tag + "_x_views"]).max()
        d_wrong = np.abs(wrong - z[tag + "_x_views"]).max()
        print("%s: interpolate-then-mask is %.3e from the recording, %.0f times the restatement's distance" % (tag, d_wrong, d_wrong / d_right))
        assert d_wrong > 100 * d_right
    assert np.abs(z["half_c_3dgs"] - z["half_exposure_c_3dgs"]).max() > 1e-3          # the correction did something in the recording


def test_fixture_holds_what_the_device_tests_need():
    z, _ = _fixture()
    for tag in ("half", "half_exposure", "three_quarters", "three_halves"):
        assert z[tag + "_residual"].shape == z[tag + "_image_pred"].shape == (3, 32, 48) and z[tag + "_residual"].dtype == np.float32
        assert 0.01 < np.abs(z[tag + "_residual"]).max() < 1
    sd = {k[3:]: torch.tensor(z[k]) for k in z.files if k.startswith("sd/")}
    net = hourglass.ColorAggregationNet()
    net.load_state_dict(sd)          # a whole checkpoint of the reference, unchanged
    assert len(sd) == 22 and os.path.getsize(os.path.join(GOLDEN, "consumer_resized.npz")) < 1 << 20


# ---- 5. the Python surface -----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_the_function():
    (render, warped, feat, ray), params = _case(8, 10)
    ok = (render, warped, feat, ray) + params

    def bad(fn, args, kind=ValueError, match="", **kw):
        with pytest.raises(kind, match="(?=.*%s).*%s" % (fn.__name__, match)):          # the function's name, wherever the message puts it
            with torch.no_grad():
                fn(*args, **kw)
    f = resample.resized_features
    bad(f, ok + ((4, 5), 3), RuntimeError, r"ibgs_amd\.resample runs on the MI355X only \(resized_features's render")
    bad(f, (torch.rand(2, 8, 10),) + ok[1:] + ((4, 5), 3), match="render")
    bad(f, ok[:1] + (torch.rand(10, 8, 10),) + ok[2:] + ((4, 5), 3), match="warped_image")
    bad(f, ok[:2] + (torch.rand(8, 8, 10),) + ok[3:] + ((4, 5), 3), match="warped_image holds 3 sources, cam_feat 2")
    bad(f, ok[:3] + (torch.rand(3, 8, 11),) + ok[4:] + ((4, 5), 3), match="camera_ray")
    bad(f, ok[:4] + (torch.rand(32, 8),) + ok[5:] + ((4, 5), 3), match="w1")
    bad(f, ok[:7] + (torch.rand(31),) + ((4, 5), 3), match="b2")
    for size in ((0, 5), (4,), 4, (4.5, 5), (4, 65537), (True, 5)):
        bad(f, ok + (size, 3), match="size|reduced")
    bad(f, ok + ((4, 5), -1), match="levels")
    bad(f, ok + ((4, 5), torch.zeros((), dtype=torch.int64)), match="levels must be an int or a 0-d int32 tensor")
    bad(f, ok + ((4, 5), torch.zeros(1, dtype=torch.int32)), match="levels")
    bad(f, ok + ((4, 5), 3, "sum"), match="mode")
    bad(f, (render.numpy(),) + ok[1:] + ((4, 5), 3), TypeError, "render")
    with pytest.raises(RuntimeError, match=r"resized_features is forward only.*torch\.no_grad\(\)"):
        f(*(ok[:4] + (params[0].clone().requires_grad_(True),) + ok[5:]), (4, 5), 3)
    u = resample.upsample_residual
    bad(u, (torch.rand(3, 4, 5), render), RuntimeError, r"ibgs_amd\.resample runs on the MI355X only \(upsample_residual's residual")
    bad(u, (torch.rand(4, 5), render), match="residual")
    bad(u, (torch.rand(3, 4, 5), torch.rand(1, 8, 10)), match="render")
    bad(u, (torch.rand(3, 0, 5), render), match="empty")
    bad(u, (torch.rand(3, 4, 5), render, "x"), TypeError, "render_scale")
    with pytest.raises(RuntimeError, match="upsample_residual is forward only"):
        u(torch.rand(3, 4, 5, requires_grad=True), render)
    bad(resample.count_levels, (warped,), RuntimeError, "MI355X only")
    bad(resample.count_levels, (torch.rand(10, 8, 10),), match="warped_image")
    bad(resample.count_levels, (warped, 0), match="nb_visible_src_frames")
    for args, kind in (((8, 10, 0), ValueError), ((8, 10, -0.5), ValueError), ((8, 10, float("nan")), ValueError), ((8, 10, float("inf")), ValueError), ((0, 10, 0.5), ValueError),
                       ((8.5, 10, 0.5), ValueError), ((8, 10, "half"), TypeError), ((8, 10, None), TypeError)):
        bad(resample.scaled_size, args, kind)
    if torch.cuda.is_available() and torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="render is on"):
            with torch.no_grad():
                f(*[t.to("cuda:0") for t in ok[:1]], *[t.to("cuda:1") for t in ok[1:]], (4, 5), 3)
    src = open(os.path.join(ROOT, "ibgs_amd", "resample.py")).read()
    assert not re.search(r"^(import|from)\s+(oracle|tests)\b", src, re.M)
    assert ".item()" not in src and ".cpu()" not in src and "synchronize" not in src and "interpolate(" not in src.split('"""')[2]          # nothing reads back; no torch resampling


def test_keyword_is_checked_before_any_gpu_work():
    h, w = 16, 24
    g = torch.Generator().manual_seed(3)
    pkg = dict(render=torch.rand(3, h, w, generator=g), warped_image=torch.rand(9, h, w, generator=g), cam_feat=torch.rand(12, h, w, generator=g),
               camera_ray=torch.rand(3, h, w, generator=g), min_depth_diff=torch.rand(1, h, w, generator=g))
    net = hourglass.ColorAggregationNet()
    with torch.no_grad():
        for call in (lambda p, **kw: hourglass.fuse_color(p, net, **kw), lambda p, **kw: net(p, **kw)):
            # a scale whose Hr falls below HG_MIN_SIDE, one whose Wr exceeds HG_MAX_SIDE: the sizes are named
            with pytest.raises(ValueError, match=r"fuse_color: residual_resolution_scale 0\.2 turns the frame of 16 x 24 into 3 x 4, which is out of the hourglass's range \(sides 4 \.\. 8192\)"):
                call(pkg, residual_resolution_scale=0.2)
            with pytest.raises(ValueError, match=r"into 6400 x 9600"):
                call(pkg, residual_resolution_scale=400)
            for s, kind in ((0, ValueError), (-1.0, ValueError), (float("nan"), ValueError), ("half", TypeError), (None, TypeError)):
                with pytest.raises(kind, match="scaled_size"):
                    call(pkg, residual_resolution_scale=s)
            # in range: the first thing that needs the device refuses the CPU tensors, at the new path's own entry
            with pytest.raises(RuntimeError, match=r"resample runs on the MI355X only \(count_levels's warped_image"):
                call(pkg, residual_resolution_scale=0.5)
            with pytest.raises(KeyError, match="fuse_color: render_pkg lacks 'use_first_src_frame_mask'"):
                call(pkg, residual_resolution_scale=0.5, enable_exposure_correction=True)
            # == 1 in any spelling: the present path (which refuses the CPU tensors at the front end)
            for s in (1, 1.0, np.float32(1)):
                with pytest.raises(RuntimeError, match=r"coloragg runs on the MI355X only"):
                    call(pkg, residual_resolution_scale=s)
    with pytest.raises(RuntimeError, match=r"fuse_color is forward only.*torch\.no_grad\(\)"):
        hourglass.fuse_color(pkg, net, residual_resolution_scale=0.5)          # the parameters require grad and grad mode is on
    # the keyword defaults to 1.0, sits behind every positional parameter, and training has none
    for f in (hourglass.fuse_color, hourglass.ColorAggregationNet.forward):
        p = inspect.signature(f).parameters
        assert p["residual_resolution_scale"].default == 1.0 and p["residual_resolution_scale"].kind is inspect.Parameter.KEYWORD_ONLY
        assert list(p)[-2:] == ["residual_resolution_scale", "enable_exposure_correction"] and list(p)[-3] == "precision"
    for f in (hourglass.fuse_color_train, coloragg.fuse_color_inputs, hourglass.hourglass_forward):
        assert "residual_resolution_scale" not in inspect.signature(f).parameters
