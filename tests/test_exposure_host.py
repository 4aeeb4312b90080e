"""The exposure correction on a CPU-only box: the C ABI (include/ibgs_exposure.h <-> _lib.EXPO_EXPORTS <-> the built library), the build registration, the
entry points' validation with null pointers and bad sizes, the argument checks of ibgs_amd.exposure and of the fuse_color keyword (which run before any
GPU work), and the float64 restatement (tests/exposure_ref.py) against the recorded run of the reference's own fuse_color with the correction on
(tests/golden/consumer.npz, keys exposure_*) and against its float32 yardstick where float32 QR loses digits."""
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, coloragg, exposure, hourglass
from tests import exposure_ref as ref
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "exposure.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "consumer.npz")
NAMES = ["ibgs_expo_required_scratch", "ibgs_expo_fit", "ibgs_expo_apply", "ibgs_expo_apply_backward"]


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_exposure.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.EXPO_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    for n in ("fit", "apply", "apply_backward"):          # the stream first, like the other unit headers
        assert re.search(r"ibgs_expo_%s\(void\* stream," % n, text), n
    defines = dict(re.findall(r"#define\s+IBGS_(EXPO_[A-Z_]+)\s+([0-9.e+-]+)", text))
    assert sorted(defines) == ["EXPO_FIT", "EXPO_MAX_GROUPS", "EXPO_MAX_SIDE", "EXPO_MOMENTS", "EXPO_PIVOT_MIN", "EXPO_PIXELS_PER_THREAD", "EXPO_SOLVE", "EXPO_SUMS", "EXPO_THREADS"]
    for name, val in defines.items():
        assert getattr(_lib, name) == float(val), name
    # the rank rule's threshold lies between the two limits of DESIGN.md section 18: below 1 / (4 cond^2) at cond 1e4, far above a residue of f64 sums
    assert 1e3 * 2.0 ** -52 < _lib.EXPO_PIVOT_MIN < 1.0 / (4 * 1e4 ** 2) / 10
    others = (_lib.EXPORTS + _lib.SSIM_EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS + _lib.GEOLOSS_EXPORTS
              + _lib.CAGG_EXPORTS + _lib.HG_EXPORTS + _lib.HGB_EXPORTS + _lib.HGH_EXPORTS + _lib.LPIPS_EXPORTS)
    assert not any("expo" in n for n in others)


# ---- 2. the build ----------------------------------------------------------------------------------------------------------------------------------------
def test_unit_is_registered_and_its_kernels_attributed():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["expo_apply_kernel", "expo_moments_kernel", "expo_solve_kernel"]
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "exposure"]
    for k in kernels:
        assert _build.tu_of(k) == "exposure", k
        assert not any(sub in k for sub in others), k          # whatever the order of the table
    assert [e for e in _build.KERNEL_TU if e[1] == "exposure"] == [("expo_", "exposure")]
    assert "exposure" in _build.SOURCES and "exposure" in _build.UNIT_HEADERS and "exposure" in _build.tu_shas()
    assert "exposure" not in _build.EXTRA and _build.compile_flags("exposure") == _build.compile_flags("ssim")          # a tolerance contract: no contraction flag
    # no kernel of another unit is claimed by the new entry
    for name in _build.SOURCES:
        if name != "exposure":
            text = open(os.path.join(ROOT, "ibgs_amd", "csrc", name + ".hip")).read()
            for k in re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", text):
                assert "expo_" not in k, (name, k)
    code = _build._code_only(src)
    assert "atomic" not in code.lower()          # per-workgroup partials and a fixed-order pass: no atomics at all
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "block_ops.h", "../../include/ibgs_exposure.h"]
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc")) if "exposure" in f and not f.startswith("_")) == ["exposure.hip"]
    assert re.search(r"block_reduce<ET, ES>\(", code)


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_expo_required_scratch
    partial = _lib.EXPO_SUMS * 8
    sweep = _lib.EXPO_THREADS * _lib.EXPO_PIXELS_PER_THREAD
    assert need(1, 1) == 128 + partial and need(1, sweep) == 128 + partial and need(1, sweep + 1) == 128 + 2 * partial
    cap = 128 + _lib.EXPO_MAX_GROUPS * partial
    assert need(1080, 1920) == need(720, 1280) == need(65536, 65536) == need(_lib.EXPO_MAX_GROUPS, sweep) == cap > need(_lib.EXPO_MAX_GROUPS - 1, sweep)
    assert need(0, 8) == 0 and need(8, 0) == 0 and need(-1, 8) == 0 and need(65537, 8) == 0
    err = lambda: built_lib.ibgs_last_error()
    fit, app, bwd = built_lib.ibgs_expo_fit, built_lib.ibgs_expo_apply, built_lib.ibgs_expo_apply_backward
    big = 1 << 20
    # fit: (stream, H, W, render, warped, mask, affine_out, status_out, scratch, bytes, phases)
    good = [None, 8, 8, 128, 128, 128, 128, 128, 128, big, _lib.EXPO_FIT]
    for k, v in ((1, 0), (2, 0), (1, 65537), (2, -3)):
        args = list(good)
        args[k] = v
        assert fit(*args) < 0 and b"expo_fit" in err() and b"out of range" in err(), (k, v)
    for v in (0, 4, -1):
        args = list(good)
        args[10] = v
        assert fit(*args) < 0 and b"phases" in err()
    for ks, msg in (((3, 4, 5), b"null image"), ((6, 7), b"null outputs"), ((8,), b"null scratch")):
        for k in ks:
            args = list(good)
            args[k] = None
            assert fit(*args) < 0 and msg in err(), k
    for k, v, msg in ((8, 64, b"aligned"), (9, 16, b"needed")):
        args = list(good)
        args[k] = v
        assert fit(*args) < 0 and msg in err(), k
    # apply, apply_backward: (stream, H, W, affine, status, image, out)
    for f, who in ((app, b"expo_apply:"), (bwd, b"expo_apply_backward:")):
        good = [None, 8, 8, 128, 128, 128, 128]
        for k, v in ((1, 0), (2, 65537)):
            args = list(good)
            args[k] = v
            assert f(*args) < 0 and who in err() and b"out of range" in err()
        for k, msg in ((3, b"null affine or status"), (4, b"null affine or status"), (5, b"null image"), (6, b"null outputs")):
            args = list(good)
            args[k] = None
            assert f(*args) < 0 and who in err() and msg in err(), k


# ---- 3. the Python surface -------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_the_function(built_lib):
    name = "exposure_correct"
    h, w = 6, 8
    g = torch.Generator().manual_seed(2)
    render, mask = torch.rand(3, h, w, generator=g), torch.ones(1, h, w, dtype=torch.int32)
    for warped in (torch.rand(9, h, w, generator=g), torch.rand(3, 3, h, w, generator=g), torch.rand(3, h, w, generator=g), torch.rand(5, 3, h, w, generator=g)):
        for m in (mask, mask[0]):
            with pytest.raises(RuntimeError, match=r"ibgs_amd\.exposure runs on the MI355X only \(exposure_correct's render"):
                exposure.exposure_correct(render, warped, m)
    warped = torch.rand(9, h, w, generator=g)
    def bad(args, kind=ValueError, match=""):
        with pytest.raises(kind, match=name + ".*" + match):
            exposure.exposure_correct(*args)
    bad((torch.rand(1, h, w), warped, mask), match="render")
    bad((torch.rand(3, 0, w), warped, mask), match="empty")
    bad((torch.rand(2, 3, h, w), warped, mask), match="render")
    bad((render, torch.rand(10, h, w), mask), match="warped_image")
    bad((render, torch.rand(18, h, w), mask), match="warped_image holds 6 sources")
    bad((render, torch.rand(0, 3, h, w), mask), match="warped_image holds 0 sources")
    bad((render, torch.rand(9, h, w + 1), mask), match="warped_image")
    bad((render, torch.rand(2, 4, h, w), mask), match="warped_image")
    bad((render, warped, torch.ones(1, h, w + 1, dtype=torch.int32)), match="use_first_src_frame_mask")
    bad((render, warped, torch.ones(2, h, w, dtype=torch.int32)), match="use_first_src_frame_mask")
    bad((render, warped, torch.ones(h * w, dtype=torch.int32)), match="use_first_src_frame_mask")
    for dtype in (torch.float32, torch.int64, torch.bool, torch.uint8):
        bad((render, warped, torch.ones(1, h, w).to(dtype)), match="int32")
    bad((render.numpy(), warped, mask), TypeError, "render")
    bad((render, warped.numpy(), mask), TypeError, "warped_image")
    bad((render, warped, mask.numpy()), TypeError, "use_first_src_frame_mask")
    src = open(os.path.join(ROOT, "ibgs_amd", "exposure.py")).read()
    assert not re.search(r"^(import|from)\s+(oracle|tests)\b", src, re.M)
    assert ".item()" not in src and ".cpu()" not in src and "synchronize" not in src and "lstsq" not in src.split('"""')[2]          # nothing reads back; no torch solve


def test_keyword_is_checked_before_any_gpu_work():
    h, w = 6, 8
    g = torch.Generator().manual_seed(3)
    pkg = dict(render=torch.rand(3, h, w, generator=g), warped_image=torch.rand(9, h, w, generator=g), cam_feat=torch.rand(12, h, w, generator=g),
               camera_ray=torch.rand(3, h, w, generator=g), min_depth_diff=torch.rand(1, h, w, generator=g))
    net = hourglass.ColorAggregationNet()
    with torch.no_grad():
        for call, name in ((lambda p: hourglass.fuse_color(p, net, enable_exposure_correction=True), "fuse_color"),
                           (lambda p: net(p, enable_exposure_correction=True), "fuse_color"),
                           (lambda p: hourglass.fuse_color_train(p, net, enable_exposure_correction=True), "fuse_color_train"),
                           (lambda p: hourglass.fuse_color_train(p, net, iter_count=1, burn_start=0, burn_end=10, enable_exposure_correction=True), "fuse_color_train"),
                           (lambda p: coloragg.fuse_color_inputs(p, net.front_end, enable_exposure_correction=True), "fuse_color_inputs")):
            with pytest.raises(KeyError, match=name + ": render_pkg lacks 'use_first_src_frame_mask'"):
                call(pkg)
            with_mask = dict(pkg, use_first_src_frame_mask=torch.ones(1, h, w, dtype=torch.int32))
            with pytest.raises(RuntimeError, match=r"exposure runs on the MI355X only"):
                call(with_mask)
            with pytest.raises(ValueError, match="exposure_correct.*int32"):
                call(dict(pkg, use_first_src_frame_mask=torch.ones(1, h, w)))
    # the keyword is the last one everywhere and off by default
    import inspect
    for f in (hourglass.fuse_color, hourglass.fuse_color_train, hourglass.ColorAggregationNet.forward, coloragg.fuse_color_inputs):
        p = list(inspect.signature(f).parameters.values())[-1]
        assert p.name == "enable_exposure_correction" and p.default is False, f


# ---- 4. the restatement against the reference's recorded run ---------------------------------------------------------------------------------------------
BAR = 1e-6          # the recording is a float32 LAPACK run: measured 1.8e-7 from the float64 restatement; the bar is about five times that


def test_restatement_reproduces_the_reference_run():
    z = np.load(GOLDEN)
    render, warped, mask = z["oracle_color"], z["oracle_warped_image"], z["oracle_use_first_src_frame_mask"]
    h, w = int(z["H"]), int(z["W"])
    assert (h, w) == (32, 48) and int((mask == 1).sum()) == 409 and mask.size == 1536
    assert 60 < ref.cond(render, mask) < 66
    corrected, affine, ok = ref.correct_ref(render, warped, mask)
    assert ok and corrected.dtype == np.float64 and affine.shape == (3, 4)
    want = z["exposure_c_3dgs"].T.reshape(3, h, w)
    d = np.abs(corrected - want).max()
    print("corrected image: the recording is %.3e from the float64 restatement" % d)
    assert d <= BAR
    assert np.abs(want - render).max() > 1e-3          # the correction did something in the recording
    # multiplying the warped image by the mask first, as the reference does, changes nothing: only masked pixels enter
    assert np.array_equal(ref.fit_ref(render, warped * np.concatenate([mask] * 15, 0), mask)[0], affine)
    x, ray, c, levels = scenes.fuse_color_inputs(corrected, z["oracle_cam_feat"], z["oracle_warped_image"], z["oracle_camera_ray"], nb_visible_src_frames=3)
    assert levels == int(z["exposure_levels"]) == 3
    dx = np.abs(x - z["exposure_x_views"]).max()
    print("features: %.3e" % dx)
    assert dx <= BAR and np.abs(c - z["exposure_c_3dgs"]).max() <= BAR and np.array_equal(ray.astype(np.float32), z["exposure_ray_dir"])
    # the gradient restatement is the transpose of the application
    g = np.random.default_rng(0).standard_normal((3, h, w))
    eps = np.random.default_rng(1).standard_normal((3, h, w))
    lhs = (ref.apply_ref(affine, render + 1e-3 * eps) - ref.apply_ref(affine, render)) * g
    assert abs(lhs.sum() - 1e-3 * (ref.apply_backward_ref(affine, g) * eps).sum()) < 1e-12


# ---- 5. the yardstick where float32 loses digits ----------------------------------------------------------------------------------------------------------
def test_yardstick_agrees_with_the_restatement_on_a_near_grey_image():
    """cond(X) about 1.5e3: a float32 QR keeps about 1e-7 x cond of the matrix's digits.  The yardstick must neither be exact (it would then not be float32)
    nor lose the fit (a rank-truncating driver would: the corrected image would be off by the near-grey directions it dropped)."""
    render, warped, mask = ref.case(32, 48, 0.3, grey=True)
    k = ref.cond(render, mask)
    assert 5e2 < k < 5e3, k
    a64, ok = ref.fit_ref(render, warped, mask)
    assert ok
    up = np.random.default_rng(4).standard_normal((3, 32, 48)).astype(np.float32)
    c32, a32, g32 = ref.yardstick(render, warped, mask, up)
    da, dc = np.abs(a32 - a64).max(), np.abs(c32 - ref.apply_ref(a64, render)).max()
    dg = np.abs(g32 - ref.apply_backward_ref(a32, up)).max()
    print("near-grey, cond %.3g: float32 matrix %.3e from float64, corrected image %.3e, gradient %.3e from the transposed apply of its own matrix" % (k, da, dc, dg))
    assert 0 < da <= 1e-7 * k * 20 and 0 < dc <= 1e-5 and dg <= 1e-5
    # ... and on a colourful one it is float32-exact
    render, warped, mask = ref.case(32, 48, 0.3)
    c32, a32 = ref.yardstick(render, warped, mask)
    a64 = ref.fit_ref(render, warped, mask)[0]
    assert np.abs(a32 - a64).max() <= 2e-6 and np.abs(c32 - ref.apply_ref(a64, render)).max() <= 2e-6
    # the rank rule of the restatement on the cases the device tests use
    r2 = render.copy()
    r2[:, mask[0] == 1] = np.float32([0.3, 0.5, 0.7])[:, None]
    r3 = render.copy()
    r3[1] = r3[0]
    few = np.zeros_like(mask)
    few.reshape(-1)[[5, 77, 900]] = 1
    assert not ref.determined(r2, mask) and not ref.determined(r3, mask) and not ref.determined(render, few) and not ref.determined(render, np.zeros_like(mask))
    few.reshape(-1)[1234] = 1
    assert ref.determined(render, few) and ref.determined(render, mask)
