"""The frame export on a CPU-only box: the restatement (tests/frame_export_ref.py) against the recorded run of the reference's own colorize
(tests/golden/frame_export.npz) and against np.percentile; the C ABI (include/ibgs_export.h <-> _lib.FEXP_EXPORTS <-> the built library); the build
registration; the entry points' validation with null pointers and bad sizes; the argument checks of ibgs_amd.frame_export, which run before any GPU work;
the `quantize` keyword of image_eval; and which inputs can tell a contracted kernel from an uncontracted one."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, frame_export, image_eval
from tests import frame_export_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "export.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_export.npz")
NAMES = ["ibgs_fexp_sizeof_frame", "ibgs_required_export", "ibgs_fexp_frame_u8", "ibgs_fexp_percentile", "ibgs_fexp_quantize"]
MAPS = ["m17x300_block", "m2x2", "m33x65", "m40x40_constant", "m5x7", "m64x48_zero_rows"]


# ---- 1. the restatement against the reference's recorded run and against numpy ---------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_colorize_pixel_for_pixel():
    z = np.load(GOLDEN)
    assert sorted(str(n) for n in z["names"]) == MAPS and z["lut"].shape == (256, 3) and z["lut"].dtype == np.uint8
    shapes = {}
    for name in MAPS:
        value, want = z["in_" + name], z["out_" + name]
        got, status = ref.colorize(value, z["lut"])
        assert status == 0 and got.dtype == np.uint8 and got.shape == want.shape == value.shape[1:] + (3,)
        assert np.array_equal(got, want), "%s: %d pixels differ" % (name, int((got != want).any(-1).sum()))
        shapes[name] = value.shape[1:]
    assert shapes == {"m5x7": (5, 7), "m33x65": (33, 65), "m17x300_block": (17, 300), "m64x48_zero_rows": (64, 48), "m2x2": (2, 2), "m40x40_constant": (40, 40)}
    # the maps are what they are meant to be: the invalid block is grey, the zero rows tie across the 2nd percentile, the constant map is one colour
    blk = z["in_m17x300_block"][0] == -99
    assert int(blk.sum()) == 6 * 36 and (z["out_m17x300_block"][blk] == 128).all() and not (z["out_m17x300_block"][~blk] == 128).all(-1).any()
    zr = z["in_m64x48_zero_rows"]
    assert int((zr == 0).sum()) == 480 and ref.percentile(zr, (2,))[0][0] == 0
    assert len(np.unique(z["out_m40x40_constant"].reshape(-1, 3), axis=0)) == 1 and np.array_equal(z["out_m40x40_constant"][0, 0], z["lut"][0])
    try:
        import matplotlib
    except ImportError:
        return
    if str(z["matplotlib_version"]) == matplotlib.__version__:
        assert np.array_equal((matplotlib.colormaps["magma_r"](np.arange(256))[:, :3] * 255).astype(np.uint8), z["lut"])


@pytest.mark.skipif(int(np.__version__.split(".")[0]) < 2, reason="rule 4 restates np.percentile as numpy 2.x evaluates it for float32 (numpy 1.x works in float64)")
@pytest.mark.parametrize("ties", [False, True], ids=["distinct", "a_third_tied_at_0"])
def test_restatement_percentile_is_numpys_bit_for_bit(ties):
    for n in ref.SELECT_SIZES:
        v = ref.depth_values(n, ties)
        got, status = ref.percentile(v, (2, 85))
        want = np.asarray([np.percentile(v, 2), np.percentile(v, 85)])
        assert status == 0 and want.dtype == np.float32 and np.array_equal(got.view(np.uint32), (want + np.float32(0)).view(np.uint32)), (n, got, want)
    for name, v, qs, inv, mask in ref.percentile_cases():
        if inv is None and mask is None and not np.isnan(v).any():
            want = np.asarray([np.percentile(v, q) for q in qs], np.float32)
            assert np.array_equal(ref.percentile(v, qs)[0], want), name          # (== : -0.0 is +0.0)


def test_which_inputs_can_tell_a_contracted_kernel():
    """Rule 1 is two rounded operations, t = fl(255 x), fl(t + 0.5).  One fma rounds 255 x + 0.5 once.  The two can only store different BYTES where the sum
    t + 0.5 is inexact next to an integer, i.e. where t and t + 0.5 lie in different binades just below one: t in [0.25, 0.5), t + 0.5 in [0.75, 1) -- byte 0
    against byte 1, decided by the one value t = 0.5 - 2^-25 (the tie rounds to 1.0).  That needs 255 x in [0.5 - 1.5 * 2^-25, 0.5 - 2^-25), a window of 2^-26,
    while consecutive float32 x near 0.5 / 255 move 255 x by 255 * 2^-32, about 2^-24: no float32 falls inside.  Everywhere else t + 0.5 is exact and both
    forms round the same real number at the same place.  So the search the rule's test was to keep comes back empty, here over the neighbourhood asked for
    and over every float32 of two whole binades; what a contracted unit WOULD change is the percentile's interpolation, and the shared cases hold such inputs."""
    assert ref.fma_sensitive_inputs().size == 0
    for lo, hi in ((2.0 ** -9, 2.0 ** -8), (0.5, 1.0)):          # the binade of 0.5 / 255, and the top one: every float32 in them
        bits = np.arange(np.float32(lo).view(np.uint32), np.float32(hi).view(np.uint32) + 1, dtype=np.uint32)
        x = bits.view(np.float32)
        assert np.array_equal(ref.round_u8(x), ref.fma_u8(x))
        assert (ref.round_u8(x).astype(np.float32) != (x.astype(np.float64) * 255.0 + 0.5).astype(np.float32)).any()          # (the bytes are not trivially equal: x is off the grid)
    t = np.float32(0.5) - np.float32(2.0 ** -25)
    assert np.float32(t + np.float32(0.5)) == 1.0 and np.float64(t) + 0.5 < 1.0          # the one tie: the two-step form says 1, the exact sum is below 1
    near = np.float32(0.5 / 255) + np.arange(-8, 9) * np.float32(2.0 ** -32)
    assert not ((near.astype(np.float64) * 255 >= 0.5 - 1.5 * 2.0 ** -25) & (near.astype(np.float64) * 255 < 0.5 - 2.0 ** -25)).any()
    differ = [name for name, v, qs, inv, mask in ref.percentile_cases() if inv is None and mask is None and not np.isnan(v).any()
              and not np.array_equal(ref.percentile_contracted(v, qs).view(np.uint32), ref.percentile(v, qs)[0].view(np.uint32))]
    print("percentile cases a contracted interpolation changes:", differ)
    assert differ
    # the inputs of rules 1-3 do hold the boundaries, and every special value
    x = ref.rule_inputs(33, 65)
    k = np.arange(255)
    assert np.isin(np.float32((k + 0.5) / 255.0), x).sum() > 20 and all(np.isin(np.float32(v), x) for v in (0.0, 1.0, -1.0, 0.5 / 255, 2.0, -2.0))
    assert x.min() < 0 and x.max() > 1 and np.abs(x).argmax() == x.size - 1
    assert ref.to_u8(x).shape == (33, 65, 3) and len(np.unique(ref.to_u8(x))) == 256


# ---- 2. the ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_export.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.FEXP_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    for n in ("frame_u8", "percentile", "quantize"):          # the stream first, like the other unit headers
        assert re.search(r"ibgs_fexp_%s\(void\* stream," % n, text), n
    defines = dict(re.findall(r"#define\s+IBGS_(FEXP_[A-Z_]+)\s+([0-9]+)", text))
    assert sorted(defines) == ["FEXP_COLORIZE", "FEXP_MAX_IMAGES", "FEXP_MAX_PIXELS", "FEXP_MAX_Q", "FEXP_MAX_SELECT", "FEXP_MAX_SIDE", "FEXP_NORMAL", "FEXP_NO_VALID",
                               "FEXP_RESIDUAL", "FEXP_ROUND", "FEXP_TRUNCATE", "FEXP_ZERO_RESIDUAL"]
    for name, val in defines.items():
        assert getattr(_lib, name) == int(val), name
    assert _lib.FEXP_MAX_SELECT == 2 ** 24 and float(np.float32(2 ** 24 - 1)) == 2 ** 24 - 1 and float(np.float32(2 ** 24 + 1)) != 2 ** 24 + 1          # n - 1 exact
    import ctypes
    assert built_lib.ibgs_fexp_sizeof_frame() == ctypes.sizeof(_lib.FexpFrame)
    for struct, mirror in (("ibgs_fexp_image", _lib.FexpImage), ("ibgs_fexp_frame", _lib.FexpFrame)):          # the same fields in the same order
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        fields = [re.sub(r"\[\w+\]", "", part).split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
        assert fields == [f for f, _ in mirror._fields_], struct
    assert frame_export.ZERO_RESIDUAL == ref.ZERO_RESIDUAL == _lib.FEXP_ZERO_RESIDUAL and frame_export.NO_VALID == ref.NO_VALID == _lib.FEXP_NO_VALID


def test_unit_is_registered_and_its_kernels_attributed():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["fexp_hist_kernel", "fexp_narrow_kernel", "fexp_quantize_kernel", "fexp_status_kernel", "fexp_write_kernel"]
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "export"]
    for k in kernels:
        assert _build.tu_of(k) == "export", k
        assert not any(sub in k for sub in others), k          # whatever the order of the table
    assert [e for e in _build.KERNEL_TU if e[1] == "export"] == [("fexp_", "export")]
    assert "export" in _build.SOURCES and [os.path.basename(h) for h in _build.UNIT_HEADERS["export"]] == ["ibgs_export.h"]
    assert _build.SOURCES.index("export") < _build.SOURCES.index("hourglass") and os.path.join(_build.OBJ, "export.o") in [os.path.join(_build.OBJ, n + ".o") for n in _build.SOURCES]
    # built, rebuilt on an edit of its header and attributed like every unit; no profile stamp: no committed summary holds its kernels, bench.py quotes none
    assert _build.UNSTAMPED == ("export",) and "export" not in _build.tu_shas() and sorted(_build.tu_shas()) == sorted(n for n in _build.SOURCES if n != "export")
    assert _build._newest_dep() >= os.path.getmtime(_build.UNIT_HEADERS["export"][0])
    assert "export" not in _build.EXTRA and _build.compile_flags("export") == _build.compile_flags("exposure")
    for name in _build.SOURCES:          # no kernel of another unit is claimed by the new entry
        if name != "export":
            text = open(os.path.join(ROOT, "ibgs_amd", "csrc", name + ".hip")).read()
            for k in re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", text):
                assert "fexp_" not in k, (name, k)
    code = _build._code_only(src)
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "block_ops.h", "../../include/ibgs_export.h"]
    # the library's flags allow contraction: the unit switches it off for all of its code, ahead of the first function
    assert code.index("#pragma clang fp contract(off)") < code.index("namespace ibgs")
    assert "fmaf(" not in code and "__builtin_fma" not in code and "rcp" not in code and "__fdividef" not in code and "fast" not in code.lower()
    # integer atomics only, and on integers only
    atomics = re.findall(r"\batomic\w+\(&?(\w+)", code)
    assert atomics and set(re.findall(r"\b(atomic\w+)\(", code)) == {"atomicAdd", "atomicMax"} and set(atomics) <= {"s_h", "s_max", "hist", "tab"}
    for name in ("s_h", "s_max", "hist", "tab"):
        assert re.search(r"uint32_t\s*\*?\s*(?:__restrict__\s+)?%s\b" % name, code), name
    assert "hipDeviceSynchronize" not in code and "hipStreamSynchronize" not in code and "hipMemcpy" not in code          # nothing waits, nothing is read back
    assert re.search(r"block_exclusive_scan<FT>\(", code)


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    import ctypes
    need = built_lib.ibgs_required_export
    assert need(1, 1) == need(1080, 1920) == need(4096, 4096) > 0 and need(1080, 1920) < 160 * 1024          # the tables do not grow with the frame
    assert need(0, 8) == 0 and need(8, 0) == 0 and need(-1, 8) == 0 and need(65537, 8) == 0 and need(65536, 65536) == 0 and need(32768, 32768) > 0
    err = lambda: built_lib.ibgs_last_error()
    big = need(8, 8)

    def frame(**kw):
        f = _lib.FexpFrame()
        f.H, f.W, f.n_images = 8, 8, 1
        f.images[0].src, f.images[0].dst, f.images[0].mode, f.images[0].channels = 256, 256, _lib.FEXP_ROUND, 3
        f.status, f.scratch, f.scratch_bytes, f.lut = 256, 256, big, 256
        for k, v in kw.items():
            if k.startswith("im_"):
                setattr(f.images[0], k[3:], v)
            else:
                setattr(f, k, v)
        return f
    call = lambda f: built_lib.ibgs_fexp_frame_u8(None, ctypes.byref(f))
    assert built_lib.ibgs_fexp_frame_u8(None, None) < 0 and b"null frame" in err()
    for kw, msg in ((dict(H=0), b"out of range"), (dict(W=65537), b"out of range"), (dict(H=65536, W=65536), b"out of range"), (dict(n_images=0), b"0 images"),
                    (dict(n_images=9), b"9 images"), (dict(status=None), b"null status"), (dict(im_src=None), b"null src"), (dict(im_dst=None), b"null dst"),
                    (dict(im_dst=258), b"dst is not 4-byte aligned"), (dict(im_src=257), b"src is not 4-byte aligned"), (dict(im_mode=5), b"mode 5"), (dict(im_mode=-1), b"mode -1"),
                    (dict(im_channels=2), b"2 channels"), (dict(im_mode=_lib.FEXP_COLORIZE), b"COLORIZE reads one plane"), (dict(im_channels=1, im_bgr=1), b"bgr needs 3"),
                    (dict(im_mode=_lib.FEXP_COLORIZE, im_channels=1, lut=None), b"null lut"),
                    (dict(im_mode=_lib.FEXP_COLORIZE, im_channels=1, scratch=None), b"null scratch"),
                    (dict(im_mode=_lib.FEXP_COLORIZE, im_channels=1, scratch=192), b"aligned"),
                    (dict(im_mode=_lib.FEXP_COLORIZE, im_channels=1, scratch_bytes=big - 1), b"needed"),
                    (dict(im_mode=_lib.FEXP_COLORIZE, im_channels=1, H=4097, W=4096), b"percentiles of"),
                    (dict(im_mode=_lib.FEXP_RESIDUAL, scratch=None), b"null scratch")):
        assert call(frame(**kw)) < 0 and b"fexp_frame_u8" in err() and msg in err(), (kw, err())
    f = frame(n_images=2)
    for mode, msg in ((_lib.FEXP_RESIDUAL, b"more than one RESIDUAL"), (_lib.FEXP_COLORIZE, b"more than one COLORIZE")):
        for i in range(2):
            f.images[i].src, f.images[i].dst, f.images[i].mode, f.images[i].channels = 256, 256, mode, 1
        assert call(f) < 0 and msg in err()
    f = frame(im_mode=_lib.FEXP_COLORIZE, im_channels=1)
    f.q32[0], f.q32[1] = 0.02, 1.5
    assert call(f) < 0 and b"outside [0, 1]" in err()
    # percentile: (stream, n, values, invalid_mask, use_invalid_val, invalid_val, nq, q32, out, status, scratch, bytes)
    q = (ctypes.c_float * 4)(0.02, 0.85, 0.5, 1.0)
    good = [None, 64, 256, None, 0, 0.0, 2, q, 256, 256, 256, big]
    for k, v, msg in ((1, -1, b"-1 values"), (1, 2 ** 24 + 1, b"16777217 values"), (6, 0, b"0 percentiles"), (6, 5, b"5 percentiles"), (7, None, b"null q32"), (2, None, b"null values"),
                      (2, 258, b"values is not 4-byte aligned"), (8, None, b"null outputs"), (9, None, b"null outputs"), (10, None, b"null scratch"), (10, 320, b"aligned"), (11, 64, b"needed")):
        args = list(good)
        args[k] = v
        assert built_lib.ibgs_fexp_percentile(*args) < 0 and b"fexp_percentile" in err() and msg in err(), (k, v, err())
    args = list(good)
    args[7] = (ctypes.c_float * 4)(0.02, float("nan"), 0, 0)
    assert built_lib.ibgs_fexp_percentile(*args) < 0 and b"outside [0, 1]" in err()
    for args, msg in (([None, 0, 256, 256], b"0 values"), ([None, 8, None, 256], b"null in"), ([None, 8, 256, None], b"null out"), ([None, 8, 258, 256], b"4-byte aligned")):
        assert built_lib.ibgs_fexp_quantize(*args) < 0 and b"fexp_quantize" in err() and msg in err()


# ---- 3. the Python surface -------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_gpu_work():
    fe = frame_export
    g = torch.Generator().manual_seed(4)
    h, w = 6, 8
    img, plane = torch.rand(3, h, w, generator=g), torch.rand(1, h, w, generator=g)
    lut = torch.zeros(256, 3, dtype=torch.uint8)
    pkg = dict(render=img, median_intersected_depth=plane, rendered_normal=img)
    cpu = r"ibgs_amd\.frame_export runs on the MI355X only \(%s's %s"
    for call, who, what in ((lambda: fe.to_u8(img), "to_u8", "image"), (lambda: fe.to_u8(plane, "truncate"), "to_u8", "image"), (lambda: fe.normal_to_u8(img), "normal_to_u8", "normal"),
                            (lambda: fe.residual_vis_u8(img), "residual_vis_u8", "residual"), (lambda: fe.percentile(plane, (2, 85)), "percentile", "values"),
                            (lambda: fe.percentile(plane, [50], invalid_val=-99, invalid_mask=plane > 0.5), "percentile", "values"),
                            (lambda: fe.colorize(plane, lut), "colorize", "value"), (lambda: fe.colorize(plane[0], lut, vmin=0, vmax=1), "colorize", "value"),
                            (lambda: fe.export_frame(pkg, lut=lut), "export_frame", "render"), (lambda: fe.export_frame(pkg, dict(image_pred=img, residual=img), img, lut, "train"), "export_frame", "render"),
                            (lambda: fe.quantize(img), "quantize", "image")):
        with pytest.raises(RuntimeError, match=cpu % (who, what)):
            call()

    def bad(call, kind, match):
        with pytest.raises(kind, match=match):
            call()
    bad(lambda: fe.to_u8(torch.rand(2, h, w)), ValueError, "to_u8: image must be")
    bad(lambda: fe.to_u8(torch.rand(h, w)), ValueError, "to_u8: image must be")
    bad(lambda: fe.to_u8(torch.rand(3, 0, w)), ValueError, "to_u8: image of 0 x 8 is empty")
    bad(lambda: fe.to_u8((img * 255).to(torch.uint8)), ValueError, "to_u8: image must be")
    bad(lambda: fe.to_u8(img.numpy()), TypeError, "to_u8: image must be a tensor")
    bad(lambda: fe.to_u8(img, rule="nearest"), ValueError, "rule must be")
    bad(lambda: fe.to_u8(img, order="gbr"), ValueError, "order must be")
    bad(lambda: fe.to_u8(plane, order="bgr"), ValueError, "order must be")
    bad(lambda: fe.normal_to_u8(plane), ValueError, "normal_to_u8: normal must be")
    bad(lambda: fe.residual_vis_u8(torch.rand(4, h, w)), ValueError, "residual_vis_u8: residual must be")
    bad(lambda: fe.percentile(plane, (1, 2, 3, 4, 5)), ValueError, "5 percentiles asked for")
    bad(lambda: fe.percentile(plane, ()), ValueError, "0 percentiles asked for")
    bad(lambda: fe.percentile(plane, (2, 101)), ValueError, r"must lie in \[0, 100\]")
    bad(lambda: fe.percentile(plane, 50), TypeError, "qs must be a sequence")
    bad(lambda: fe.percentile(plane.long(), (2,)), ValueError, "values must be float32")
    bad(lambda: fe.percentile(plane, (2,), invalid_mask=torch.zeros(h * w + 1, dtype=torch.bool)), ValueError, "invalid_mask must hold 48")
    bad(lambda: fe.percentile(plane, (2,), invalid_mask=plane), ValueError, "invalid_mask must hold")
    bad(lambda: fe.percentile(plane, (2,), invalid_val="x"), TypeError, "invalid_val must be a number")
    huge = torch.zeros(1).expand(4097, 4096)          # H W = 2^24 + 4096, no memory behind it
    bad(lambda: fe.percentile(huge, (2, 85)), ValueError, r"percentile: 16781312 values \(limit: 2\^24")
    bad(lambda: fe.colorize(huge, lut), ValueError, r"colorize: percentiles of 4097 x 4096 values \(limit: 2\^24")
    bad(lambda: fe.export_frame(dict(render=torch.zeros(1).expand(3, 4097, 4096), median_intersected_depth=huge[None], rendered_normal=torch.zeros(1).expand(3, 4097, 4096)), lut=lut),
        ValueError, r"export_frame: percentiles of 4097 x 4096")
    with pytest.raises(RuntimeError, match="MI355X only"):          # with both bounds given no percentile is needed: the size passes, the CPU tensor does not
        fe.colorize(huge, lut, vmin=0.0, vmax=1.0)
    bad(lambda: fe.colorize(plane, lut[:255]), ValueError, r"lut must be a \(256, 3\) uint8")
    bad(lambda: fe.colorize(plane, lut.float()), ValueError, "lut must be")
    bad(lambda: fe.colorize(torch.rand(2, h, w), lut), ValueError, "colorize: value must be")
    bad(lambda: fe.colorize(plane, lut, background=(1, 2)), ValueError, "background must be three")
    bad(lambda: fe.colorize(plane, lut, background=(1, 2, 256)), ValueError, "background must be three")
    bad(lambda: fe.colorize(plane, lut, vmin="a"), TypeError, "vmin must be a number")
    bad(lambda: fe.colorize(plane, lut, invalid_mask=torch.zeros(h, w + 1, dtype=torch.bool)), ValueError, "invalid_mask must hold 6 x 8")
    bad(lambda: fe.export_frame(pkg, lut=lut, split="val"), ValueError, "split must be")
    bad(lambda: fe.export_frame(dict(render=img), lut=lut), KeyError, "render_pkg lacks 'median_intersected_depth'")
    bad(lambda: fe.export_frame(pkg, dict(image_pred=img), lut=lut), KeyError, "fusion_out lacks 'residual'")
    bad(lambda: fe.export_frame(pkg, gt=torch.rand(3, h, w + 1), lut=lut), ValueError, "export_frame: gt is")
    bad(lambda: fe.export_frame(dict(pkg, median_intersected_depth=torch.rand(1, h + 1, w)), lut=lut), ValueError, "median_intersected_depth is")
    bad(lambda: fe.export_frame(dict(pkg, rendered_normal=plane), lut=lut), ValueError, "export_frame: normal must be")
    bad(lambda: fe.quantize(torch.zeros(3, dtype=torch.int32)), TypeError, "quantize: image must be a float tensor")
    bad(lambda: fe.to_host(dict(packed=torch.zeros(64, dtype=torch.uint8), layout={}), pinned=torch.zeros(8, dtype=torch.uint8)), ValueError, "pinned must be")
    src = open(os.path.join(ROOT, "ibgs_amd", "frame_export.py")).read()
    assert not re.search(r"^(import|from)\s+(oracle|tests)\b", src, re.M)
    body = src.split('"""', 2)[2]
    assert ".item()" not in body and ".cpu()" not in body and ".tolist()" not in body and "torch.quantile" not in body and "torch.sort" not in body
    # the one wait and the one copy are to_host's
    assert body.count("synchronize") == 1 and body.count(".copy_(") == 1 and body.index("def to_host") < body.index("synchronize") < body.index("def quantize")
    assert re.search(r"^import matplotlib|^from matplotlib", src, re.M) is None and "import matplotlib" in body          # lazily, inside colormap_lut


def test_colormap_lut_is_the_fixtures_table():
    matplotlib = pytest.importorskip("matplotlib")
    z = np.load(GOLDEN)
    lut = frame_export.colormap_lut("magma_r", "cpu")
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and frame_export.colormap_lut("magma_r", "cpu") is lut
    if str(z["matplotlib_version"]) == matplotlib.__version__:
        assert np.array_equal(lut.numpy(), z["lut"])


def test_quantize_keyword_is_off_by_default_and_leaves_the_old_path_alone():
    for fn in (image_eval.image_metrics, image_eval.evaluate_images):
        p = list(inspect.signature(fn).parameters.values())
        assert p[-1].name == "quantize" and p[-1].default is False and p[-2].name == "lpips_net" and p[-2].default is None, fn
    src = inspect.getsource(image_eval.image_metrics)
    body = src.split('"""')[2]
    # one branch, taken only with the keyword; the lines after it are the parent's, untouched
    assert body.count("quantize") == 3 and re.search(r"\n    if quantize:\n        renders, gts = frame_export\.quantize\(renders\), frame_export\.quantize\(gts\)\n    x = renders\.detach\(\)\.float\(\)\.contiguous\(\)\n", body)
    assert "image_metrics(torch.stack([r[i] for i in idx]), torch.stack([g[i] for i in idx]), lpips_net, quantize)" in inspect.getsource(image_eval.evaluate_images)
    x = torch.rand(1, 3, 16, 16)
    for q in (False, True):          # CPU tensors are refused by the check in front of the branch, either way
        with pytest.raises(RuntimeError):
            image_eval.image_metrics(x, x, quantize=q)
    # the restatement's quantisation: bytes / 255 in float32, idempotent
    v = ref.rule_inputs(5, 7)
    qv = ref.quantize(v)
    assert qv.dtype == np.float32 and np.array_equal(qv, ref.to_u8(v).transpose(2, 0, 1).astype(np.float32) / np.float32(255)) and np.array_equal(ref.quantize(qv), qv)
