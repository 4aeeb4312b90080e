"""Training at a reduced residual resolution on a CPU-only box: the C ABI (include/ibgs_resample_train.h <-> _lib.RZT_EXPORTS <-> the built library), the build
registration (the kernels' attribution, no atomics, every header the unit includes in its dependency and stamp lists, the tap and value rule and the per-slot
backward each defined once under csrc/shared/ and called by both of their units, every other unit's stamp unchanged), the entry points' validation with null pointers and bad sizes, the refusals of
ibgs_amd.resample_train (which run before any GPU work), the arbiter (tests/resample_train_ref.py) against torch's own float64 F.interpolate composition with
autograd and against the recorded gradients of the reference's fuse_color at residual_resolution_scale 0.5 (tests/golden/consumer_resized_train.npz), and the
decided seeds of the device tests."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, hourglass, resample, resample_train
from tests import resample_ref as ref
from tests import resample_train_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ibgs_amd", "csrc")
SRC = os.path.join(CSRC, "rsztrain.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["ibgs_rzt_required_scratch", "ibgs_rzt_features_backward", "ibgs_rzt_upsample_backward"]
BWD_H, TAPS_H = os.path.join(CSRC, "shared", "pv_mlp_bwd.h"), os.path.join(CSRC, "shared", "rsz_taps.h")
KERNELS = ["rzt_features_bwd_kernel", "rzt_gather_kernel", "rzt_upsample_bwd_kernel"]          # the final pass of the parameter gradients is coloragg.hip's cagg_final_kernel
# _build.tu_shas() of the commit that gave coloragg, resample and rsztrain one definition of the tap rule and of the per-view backward: those three stamps are
# that commit's; lpips, hgtrain and hourglass are those of the commit that gave them csrc/shared/conv_tile.h; hghalf and hghtrain (which had no stamp before) are
# those of the commit that gave the two csrc/shared/conv_tile_f16.h and left conv_tile.h's and hg_net.h's code alone; every other one is still that of the
# commit rsztrain was added to
PARENT_SHAS = {"api": "d2cea40a3180", "preprocess": "de228898d0b1", "scan_sort": "01e63032a313", "binning": "f337b73e1959", "render_fwd": "6ae05116c8bc",
               "render_bwd": "052d2dbf3751", "preprocess_bwd": "a45a137dac86", "knn": "e9bfb2e02f4f", "adam": "6a3146aa7716", "compact": "99a39d9227b5",
               "deterministic": "a24d88fa046d", "loss": "1f16fa584baf", "depth_normal": "6cf4fb76b878", "activate": "62185582088c", "tsdf": "80be8448d09b",
               "mesh": "59c42111558a", "mesh_eval": "8214092e1449", "registration": "5a0bad737c95", "dtu": "f17c4e79d7ed", "ssim": "da26b26bfdb8",
               "geoloss": "9a7cae8f65e6", "coloragg": "0e34556dbaa7", "exposure": "315be22df182", "resample": "7bb6e6901370", "rsztrain": "c66c6940738e", "lpips": "4e4cd0b29e2b",
               "hgtrain": "f5c55b05eb06", "hghalf": "524cc488b11b", "hghtrain": "695f31dcc08f", "hourglass": "d97fb1d55e22"}


# ---- 1. the ABI and the build ----------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_resample_train.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.RZT_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
        if n != "ibgs_rzt_required_scratch":
            assert re.search(r"%s\(void\* stream," % n, text), n          # the stream first, like the other unit headers
    assert re.findall(r"#define\s+(IBGS_\w+)", text) == ["IBGS_RESAMPLE_TRAIN_H"]          # the limits and modes are ibgs_resample.h's
    assert _lib.RSZ_EXPORTS == ["ibgs_rsz_features_forward", "ibgs_rsz_residual_upsample"] and not any("rzt" in n for n in _lib.RSZ_EXPORTS + _lib.CAGG_EXPORTS + _lib.EXPORTS)


def test_unit_is_registered_and_its_kernels_attributed():
    src = open(SRC).read()
    found = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert found == KERNELS
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "rsztrain"]
    for k in found:
        assert _build.tu_of(k) == "rsztrain", k
        assert "rsz_" not in k and not any(sub in k for sub in others), k          # whatever the order of the table
    at = _build.KERNEL_TU.index(("rsz_", "resample"))
    assert _build.KERNEL_TU[at + 1] == ("rzt_", "rsztrain") and [e for e in _build.KERNEL_TU if e[1] == "rsztrain"] == [("rzt_", "rsztrain")]
    assert _build.SOURCES.index("rsztrain") < _build.SOURCES.index("hourglass") and "rsztrain" in _build.tu_shas()
    assert "rsztrain" not in _build.EXTRA and _build.compile_flags("rsztrain") == _build.compile_flags("resample") == _build.compile_flags("coloragg")
    for name in _build.SOURCES:          # no kernel of another unit is claimed by the new entry
        if name != "rsztrain":
            for k in re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", open(os.path.join(CSRC, name + ".hip")).read()):
                assert "rzt_" not in k, (name, k)
    code = _build._code_only(src)
    assert "atomic" not in code.lower()          # sums in a fixed order: no atomics of any kind
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "shared/pv_mlp_bwd.h", "shared/rsz_taps.h", "../../include/ibgs_resample.h", "../../include/ibgs_resample_train.h"]
    assert re.findall(r'#include "([^"]+)"', open(BWD_H).read()) == ["pv_mlp.h"] and re.findall(r'#include "([^"]+)"', open(TAPS_H).read()) == ["../common.h", "../../../include/ibgs_resample.h"]
    assert re.search(r"pv_mlp\(", code) and re.search(r"pv_slot\(", code) and not re.search(r"mfma", code.replace("pv_mfma", ""))          # the forward's own chain
    assert sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) == ["adam_math.h", "blend.h", "block_ops.h", "common.h", "sh_color.h", "wave_bits.h", "wave_reduce.h"]
    assert sorted(os.listdir(os.path.join(CSRC, "shared"))) == ["conv_tile.h", "conv_tile_f16.h", "hg_net.h", "pv_mlp.h", "pv_mlp_bwd.h", "rsz_taps.h", "ssim_window.h"]


def test_borrowed_headers_reach_the_rebuild_check_and_the_stamp(tmp_path, monkeypatch):
    """UNIT_HEADERS lists, per unit, every header it includes outside csrc/*.h (there is no second table): an edit of a header must change the stamps of exactly
    the units that include it and count as a newer dependency."""
    base = lambda hs: [os.path.basename(h) for h in hs]
    assert base(_build.UNIT_HEADERS["rsztrain"]) == ["ibgs_resample_train.h", "ibgs_resample.h", "pv_mlp.h", "pv_mlp_bwd.h", "rsz_taps.h"]
    assert all(os.path.exists(h) for hs in _build.UNIT_HEADERS.values() for h in hs)
    assert not hasattr(_build, "BORROWED_HEADERS") and not hasattr(_build, "unit_headers") and "api" not in _build.UNIT_HEADERS
    before = _build.tu_shas()
    for header, users in (("pv_mlp.h", {"coloragg", "resample", "rsztrain"}), ("pv_mlp_bwd.h", {"coloragg", "rsztrain"}), ("rsz_taps.h", {"resample", "rsztrain"}),
                          ("ibgs_resample.h", {"resample", "rsztrain"}), ("ibgs_resample_train.h", {"rsztrain"}), ("conv_tile_f16.h", {"hghalf", "hghtrain"})):
        assert {k for k, hs in _build.UNIT_HEADERS.items() if header in base(hs)} == users, header
        real = [h for h in _build.UNIT_HEADERS[sorted(users)[-1]] if os.path.basename(h) == header][0]          # (any of its users lists it: rsztrain, hghtrain)
        edited = tmp_path / header
        edited.write_text(open(real).read() + "\nstatic const int edited_for_the_test = 1;\n")
        swap = lambda hs: [str(edited) if os.path.basename(h) == header else h for h in hs]
        monkeypatch.setattr(_build, "UNIT_HEADERS", {k: swap(v) for k, v in _build.UNIT_HEADERS.items()})
        after = _build.tu_shas()
        assert {k for k in before if after[k] != before[k]} == users, header
        assert _build._newest_dep() >= os.path.getmtime(str(edited))
        monkeypatch.undo()
    assert _build.tu_shas() == before
    # the table is the truth: what a unit's source and its shared headers include, outside csrc/*.h and include/ibgs_rast.h, is what it lists
    for unit in ("coloragg", "resample", "rsztrain"):
        seen, todo = set(), [os.path.join(CSRC, unit + ".hip")]
        while todo:
            f = todo.pop()
            for inc in re.findall(r'#include "([^"]+)"', open(f).read()):
                path = os.path.normpath(os.path.join(os.path.dirname(f), inc))
                if os.path.dirname(path) != CSRC and os.path.basename(path) != "ibgs_rast.h" and path not in seen:
                    seen.add(path)
                    todo.append(path)
        assert seen == {os.path.normpath(h) for h in _build.UNIT_HEADERS[unit]}, unit


def test_every_other_units_stamp_is_the_parents():
    now = _build.tu_shas()
    assert sorted(now) == sorted(PARENT_SHAS)
    assert {k: now[k] for k in PARENT_SHAS} == PARENT_SHAS


def _csrc_code():
    """{path relative to csrc/: its code without comments} for every .hip and .h under csrc/, shared/ included"""
    files = [f for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))] + ["shared/" + f for f in os.listdir(os.path.join(CSRC, "shared"))]
    return {f: _build._code_only(open(os.path.join(CSRC, f)).read()) for f in files}


OURS = ["coloragg.hip", "resample.hip", "rsztrain.hip", "shared/pv_mlp.h", "shared/pv_mlp_bwd.h", "shared/rsz_taps.h"]          # the colour tail's units and their shared headers
DEFINES = r"^(?:template[^\n]*\n)?(?:__device__|__host__|__global__|static|inline)[^\n;]*\b%s\s*\("          # a function's definition (these sources declare nothing ahead)


def test_tap_and_blend_are_defined_once_and_both_units_call_them():
    code = _csrc_code()
    for what, pattern in (("struct RszTap", r"\bstruct RszTap\b"), ("rsz_tap(", DEFINES % "rsz_tap"), ("rsz_blend(", DEFINES % "rsz_blend"), ("rsz_sides_ok(", DEFINES % "rsz_sides_ok")):
        assert [f for f, text in code.items() for _ in re.findall(pattern, text, re.M)] == ["shared/rsz_taps.h"], what
    assert "struct RszTap { uint32_t i0, i1; float t, u; };" in code["shared/rsz_taps.h"]
    for unit in ("resample.hip", "rsztrain.hip"):
        assert not re.search(DEFINES % r"r[sz][zt]_(?:tap|blend|sides_ok)", code[unit], re.M) and not re.search(r"\bstruct\s+R[sz][zt]Tap\b", code[unit]), unit
        assert not re.search(r"\br[z]t_(?:tap|blend|sides_ok)\b|\bRztTap\b", code[unit]), unit
        assert re.search(r"= rsz_tap\(", code[unit]) and re.search(r"= rsz_blend\(", code[unit]) and re.search(r"!rsz_sides_ok\(who,", code[unit]), unit
    assert sorted(f for f, text in code.items() if re.search(r"r[sz][zt]_tap\(", text)) == ["resample.hip", "rsztrain.hip", "shared/rsz_taps.h"]          # no other user


def test_per_view_backward_is_defined_once_and_both_units_call_it():
    code = _csrc_code()
    for name in ("pv_bwd_setup", "pv_bwd_hmax", "pv_bwd_slot", "pv_bwd_end_chunk", "pv_bwd_flush", "pv_levels_of", "pv_bwd_groups"):
        assert [f for f, text in code.items() for _ in re.findall(DEFINES % name, text, re.M)] == ["shared/pv_mlp_bwd.h"], name
    assert "pv_bwd" not in code["resample.hip"] and "pv_mlp_bwd.h" not in open(os.path.join(CSRC, "resample.hip")).read()          # forward only
    for unit in ("coloragg.hip", "rsztrain.hip"):
        for name in ("pv_bwd_setup<IG>(", "pv_bwd_hmax<MODE>(", "pv_bwd_slot<MODE, IG>(", "pv_bwd_end_chunk(", "pv_bwd_flush(", "pv_launch_final(st,", "pv_bwd_groups("):
            assert name in code[unit], (unit, name)
        # the unit's own text touches none of the backward's state: with the calls into the shared header taken out, no cross-half exchange, no weight columns, no
        # transposed operand, no accumulator, no staged row
        rest = re.sub(r"\bpv_\w+(?:<[^>\n]*>)?\([^;]*\);", "", code[unit])
        for word in ("__shfl_xor", "s_w1c", "a2t", "acc2", "acc1", "accb", "s_t[", "s_x[", ".t[", ".x[", ".at[") + (("__syncthreads",) if unit == "rsztrain.hip" else ()):
            assert word not in rest, (unit, word)          # (coloragg.hip's level count and final pass have barriers of their own)
        # the two statements of how a slot is loaded: one loader per kernel, called by the pre-pass and by the slot loop
        assert len(re.findall(r"const auto load = \[&\]\(int k, float \(&x\)\[PV_INP\]\)", code[unit])) == 1 and "load(k, x);" in code[unit], unit
    # one final pass: cagg_final_kernel is the only kernel under csrc/ whose body adds rows of PVB_PARTIAL partials, and coloragg.hip owns its launcher
    adds = []
    for f, text in code.items():
        for m in re.finditer(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(.*?\n\}\n", text, flags=re.S):
            if re.search(r"\+=\s*partials\[", m.group(0)) and (f in OURS or "PVB_PARTIAL" in m.group(0)):          # (other units have partials and final passes
                adds.append((f, m.group(1)))                                                                       # of their own: not rows of PVB_PARTIAL)
    assert adds == [("coloragg.hip", "cagg_final_kernel")] and "PVB_PARTIAL + e]" in code["coloragg.hip"]
    assert re.search(r"^void pv_launch_final\(hipStream_t st, const double\* partials, int groups, float\* d_w1, float\* d_b1, float\* d_w2, float\* d_b2\);$", code["shared/pv_mlp_bwd.h"], re.M)
    assert len(re.findall(r"^void pv_launch_final\([^;]*\)\n\{", code["coloragg.hip"], re.M)) == 1 and code["coloragg.hip"].count("hipLaunchKernelGGL(cagg_final_kernel") == 1
    assert "cagg_final_kernel" not in code["rsztrain.hip"] and "rzt_final" not in "".join(code.values())
    # each of these lines of the backward is written in one file only
    for line, where in ((r"mine\[PV_F \* PV_F", "shared/pv_mlp_bwd.h"), (r"taken \|= 1u", "shared/pv_mlp_bwd.h"), (r"__shfl_xor", "shared/pv_mlp_bwd.h"),
                        (r"acc2d\[r\] \+=", "shared/pv_mlp_bwd.h"), (r"s_sum\[series\]", "coloragg.hip")):
        assert [f for f in OURS if re.search(line, code[f])] == [where], line


def test_validation_before_any_gpu_work(built_lib):
    err = lambda: built_lib.ibgs_last_error()
    size, bwd, up = built_lib.ibgs_rzt_required_scratch, built_lib.ibgs_rzt_features_backward, built_lib.ibgs_rzt_upsample_backward
    # at most 512 workgroups x 1312 f64 partials, then S x 3 planes of Hr x Wr floats, and 128 bytes of slack (both offsets are multiples of 128 here)
    assert size(3, 8, 8, 4, 4) == 1 * 1312 * 8 + 9 * 16 * 4 + 128 and size(3, 1080, 1920, 540, 960) == 512 * 1312 * 8 + 9 * 540 * 960 * 4 + 128
    for bad in ((0, 8, 8, 4, 4), (6, 8, 8, 4, 4), (3, 0, 8, 4, 4), (3, 8, 65537, 4, 4), (3, 8, 8, 0, 4), (3, 8, 8, 9, 4), (3, 8, 8, 4, 9)):
        assert size(*bad) == 0, bad
    need = size(3, 8, 8, 4, 4)
    # backward: (stream, S, H, W, Hr, Wr, mode, render, warped, feat, w1, b1, w2, b2, levels, grad_out, 6 gradients, scratch, bytes)
    good = [None, 3, 8, 8, 4, 4, 0] + [128] * 9 + [128] * 6 + [128, need]
    for k, v, msg in ((1, 0, b"sources"), (1, 6, b"sources"), (2, 0, b"a frame of"), (3, 65537, b"a frame of"), (4, 0, b"a reduced frame of"), (5, 65537, b"a reduced frame of")):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and b"rzt_features_backward" in err() and b"out of range" in err() and msg in err(), (k, v)
    for k, v in ((4, 9), (5, 9)):          # an upscaled network: both sizes are named
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and b"upscaled" in err() and (b"%d x %d" % (args[4], args[5])) in err() and b"8 x 8" in err(), (k, v)
    for v in (2, -1):
        args = list(good)
        args[6] = v
        assert bwd(*args) < 0 and b"mode" in err()
    for ks, msg in (((7, 8, 9), b"null image"), ((10, 11, 12, 13), b"null parameters"), ((14,), b"null levels"), ((15,), b"null grad_out"), ((22,), b"null scratch")):
        for k in ks:
            args = list(good)
            args[k] = None
            assert bwd(*args) < 0 and msg in err(), k
    args = list(good)
    args[16:22] = [None] * 6
    assert bwd(*args) < 0 and b"no gradient is asked for" in err()
    args = list(good)
    args[23] = need - 1
    assert bwd(*args) < 0 and b"needed" in err()
    args = list(good)
    args[22] = 192
    assert bwd(*args) < 0 and b"not 128-byte aligned" in err()
    # upsample: (stream, H, W, Hr, Wr, grad_residual_out, grad_image_pred, grad_residual_r)
    good = [None, 8, 8, 4, 4, 128, 128, 128]
    for k, v, msg in ((1, 0, b"a frame of"), (2, 65537, b"a frame of"), (3, 0, b"a reduced frame of"), (4, 65537, b"a reduced frame of")):
        args = list(good)
        args[k] = v
        assert up(*args) < 0 and b"rzt_upsample_backward" in err() and b"out of range" in err() and msg in err(), (k, v)
    args = list(good)
    args[5] = args[6] = None
    assert up(*args) < 0 and b"both null" in err()
    args = list(good)
    args[7] = None
    assert up(*args) < 0 and b"null outputs" in err()


# ---- 2. the Python surface -----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_the_function():
    (render, warped, feat, ray), params = ref.seeded_case(8, 10)
    ok = (render, warped, feat, ray) + params

    def bad(fn, args, kind=ValueError, match="", **kw):
        with pytest.raises(kind, match="(?=.*%s).*%s" % (fn.__name__, match)):
            fn(*args, **kw)
    f = resample_train.resized_features_train
    bad(f, ok + ((4, 5), 3), RuntimeError, r"ibgs_amd\.resample_train runs on the MI355X only \(resized_features_train's render")
    bad(f, (torch.rand(2, 8, 10),) + ok[1:] + ((4, 5), 3), match="render")
    bad(f, ok[:2] + (torch.rand(8, 8, 10),) + ok[3:] + ((4, 5), 3), match="warped_image holds 3 sources, cam_feat 2")
    bad(f, ok[:7] + (torch.rand(31),) + ((4, 5), 3), match="b2")
    for size in ((0, 5), (4,), 4, (4.5, 5), (4, 65537), (True, 5)):
        bad(f, ok + (size, 3), match="size|reduced")
    for size in ((9, 5), (4, 11), (16, 20)):          # upscaling, in either side: refused before the CPU tensors are, with both sizes named
        bad(f, ok + (size, 3), match=r"a reduced frame of %d x %d is larger than the frame of 8 x 10: training an upscaled network" % size)
    bad(f, ok + ((4, 5), -1), match="levels")
    bad(f, ok + ((4, 5), torch.zeros((), dtype=torch.int64)), match="levels must be an int or a 0-d int32 tensor")
    bad(f, ok + ((4, 5), 3, "sum"), match="mode")
    u = resample_train.upsample_residual_train
    bad(u, (torch.rand(3, 4, 5, requires_grad=True), render), RuntimeError, r"ibgs_amd\.resample_train runs on the MI355X only \(upsample_residual_train's residual")
    bad(u, (torch.rand(4, 5), render), match="residual")
    bad(u, (torch.rand(3, 4, 5), torch.rand(1, 8, 10)), match="render")
    bad(u, (torch.rand(3, 4, 5), render, "x"), TypeError, "render_scale")
    # the forward-only functions keep refusing grad
    with pytest.raises(RuntimeError, match="resized_features is forward only"):
        resample.resized_features(*(ok[:4] + (params[0].clone().requires_grad_(True),) + ok[5:]), (4, 5), 3)
    with pytest.raises(RuntimeError, match="upsample_residual is forward only"):
        resample.upsample_residual(torch.rand(3, 4, 5, requires_grad=True), render)
    src = open(os.path.join(ROOT, "ibgs_amd", "resample_train.py")).read()
    assert not re.search(r"^(import|from)\s+(oracle|tests)\b", src, re.M)
    assert ".item()" not in src and ".cpu()" not in src and "synchronize" not in src and "interpolate(" not in src          # nothing reads back; no torch resampling
    assert "ibgs_rsz_features_forward" in src and "ibgs_rsz_residual_upsample" in src          # the forwards are resample's own entry points
    assert src.count("once_differentiable") == 2          # double backward raises


def test_scale_is_checked_before_any_gpu_work():
    h, w = 16, 24
    g = torch.Generator().manual_seed(3)
    pkg = dict(render=torch.rand(3, h, w, generator=g), warped_image=torch.rand(9, h, w, generator=g), cam_feat=torch.rand(12, h, w, generator=g),
               camera_ray=torch.rand(3, h, w, generator=g), min_depth_diff=torch.rand(1, h, w, generator=g))
    net = hourglass.ColorAggregationNet()
    f = resample_train.fuse_color_train_scaled
    with pytest.raises(ValueError, match=r"fuse_color_train_scaled: residual_resolution_scale 0\.2 turns the frame of 16 x 24 into 3 x 4, which is out of the hourglass's range \(sides 4 \.\. 8192\)"):
        f(pkg, net, 0.2)
    with pytest.raises(ValueError, match=r"into 6400 x 9600"):
        f(pkg, net, 400)
    with pytest.raises(ValueError, match=r"fuse_color_train_scaled: residual_resolution_scale 1\.5 turns the frame of 16 x 24 into 24 x 36: training an upscaled network"):
        f(pkg, net, 1.5)
    for s, kind in ((0, ValueError), (-1.0, ValueError), (float("nan"), ValueError), ("half", TypeError), (None, TypeError)):
        with pytest.raises(kind, match="scaled_size"):
            f(pkg, net, s)
    with pytest.raises(TypeError, match="fuse_color_train_scaled: net must be a ColorAggregationNet"):
        f(pkg, net.cnn, 0.5)
    with pytest.raises(KeyError, match="fuse_color_train_scaled: render_pkg lacks 'cam_feat'"):
        f({k: v for k, v in pkg.items() if k != "cam_feat"}, net, 0.5)
    # in range: the first thing that needs the device refuses the CPU tensors
    with pytest.raises(RuntimeError, match=r"resample runs on the MI355X only \(count_levels's warped_image"):
        f(pkg, net, 0.5)
    with pytest.raises(KeyError, match="fuse_color_train_scaled: render_pkg lacks 'use_first_src_frame_mask'"):
        f(pkg, net, 0.5, enable_exposure_correction=True)
    for s in (1, 1.0, np.float32(1)):          # == 1 in any spelling: fuse_color_train itself
        with pytest.raises(RuntimeError, match=r"coloragg runs on the MI355X only"):
            f(pkg, net, s)
    p = list(inspect.signature(f).parameters)
    assert p == ["render_pkg", "net", "residual_resolution_scale"] + list(inspect.signature(hourglass.fuse_color_train).parameters)[2:]
    assert "residual_resolution_scale" not in inspect.signature(hourglass.fuse_color_train).parameters


# ---- 3. the arbiter against torch's float64 composition with autograd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_arbiter_agrees_with_torch_autograd_in_float64(mode):
    for h, w, s in tr.FRAMES:
        case, params = ref.seeded_case(h, w, seed=tr.SEEDS[(h, w, s)])
        size = ref.scaled_size(h, w, s)
        go = torch.randn((1, 38) + size, generator=torch.Generator().manual_seed(h * w))
        for levels in (0, 1, 3):
            mine, out = tr.feature_grads(case, params, size, levels, mode, go)
            theirs, t_out = tr.feature_grads(case, params, size, levels, mode, go, interpolate=True)
            want, _ = ref.features_ref(*case, *params, size, mode=mode, levels=levels)
            assert np.abs(out - want).max() <= 1e-12 * np.abs(want).max()          # the differentiable composition is resample_ref's arbiter
            for k in tr.NAMES:
                top = max(np.abs(theirs[k]).max(), 1e-300)
                d = np.abs(mine[k] - theirs[k]).max()
                print("%dx%d s %.2f %s levels %d %-7s arbiter against torch float64 %.3e (max %.3e)" % (h, w, s, mode, levels, k, d, top))
                assert mine[k].shape == theirs[k].shape and d <= 1e-10 * top, (k, d, top)
            if levels == 0:
                assert not any(mine[k].any() for k in tr.NAMES[1:]) and mine["render"].any()
    for full, reduced in (((9, 11), (4, 5)), ((9, 11), (1, 5)), ((9, 12), (4, 1)), ((6, 7), (1, 1)), ((1, 1), (4, 5)), ((1, 9), (4, 5)), ((48, 72), (32, 48))):
        rng = np.random.default_rng(full[0] * 100 + reduced[1])
        res, render = rng.standard_normal((3,) + reduced), rng.random((3,) + full)
        g_up, g_pred = rng.standard_normal((3,) + full), rng.standard_normal((3,) + full)
        for scale in (1.0, 0.5, 0.0):
            for a, b in ((g_up, None), (None, g_pred), (g_up, g_pred)):
                mine, theirs = tr.upsample_grads(res, render, scale, a, b), tr.upsample_grads(res, render, scale, a, b, interpolate=True)
                for k in mine:
                    assert np.abs(mine[k] - theirs[k]).max() <= 1e-10 * max(np.abs(theirs[k]).max(), 1e-300), (full, reduced, scale, k)


# ---- 4. the decided seeds ----------------------------------------------------------------------------------------------------------------------------------
def test_every_frame_has_its_decided_seed():
    assert tr.FRAMES == [(8, 8, 0.5), (9, 11, 0.5), (9, 13, 0.56), (33, 65, 0.5), (32, 48, 0.75), (35, 37, 0.5)] and [tr.SEEDS[f] for f in tr.FRAMES] == [0, 0, 1, 0, 4, 2]
    for h, w, s in tr.FRAMES:
        assert tr.decided_seed(h, w, s) == tr.SEEDS[(h, w, s)], (h, w, s)
        case, params = ref.seeded_case(h, w, seed=tr.SEEDS[(h, w, s)])
        pre, gap = tr.margin(case, params, ref.scaled_size(h, w, s))
        print("%dx%d s %.2f seed %d: smallest |pre-activation| %.3e, smallest non-zero max gap %.3e" % (h, w, s, tr.SEEDS[(h, w, s)], pre, gap))
        assert pre >= tr.MARGIN and gap >= tr.MARGIN and tr.MARGIN == 2e-6
        v = ref.coloragg_ref.valid_ref(case[2])
        assert not v[1].any() and all((v[k][:, 1:] != v[k][:, :-1]).mean() > 0.2 for k in (0, 2))          # validity varies between neighbours; one slot all-invalid


def test_the_frame_beyond_one_pass_is_decided_by_its_biases():
    h, w, s = tr.BIG
    size = ref.scaled_size(h, w, s)
    assert size == (258, 256) and (size[0] * size[1] + 127) // 128 == 516 > 512          # the chunks against PVB_MAX_GROUPS
    assert re.search(r"constexpr int PVB_MAX_GROUPS = 512;", open(BWD_H).read()) and re.search(r"constexpr int PVB_CHUNK = PVB_WAVES \* PVB_B;", open(BWD_H).read())
    assert re.search(r"constexpr int PVB_WAVES = PVB_T / 64;", open(BWD_H).read()) and re.search(r"constexpr int PVB_T = 256;", open(BWD_H).read()) and re.search(r"constexpr int PVB_B = 32;", open(BWD_H).read())
    assert "pv_bwd_groups(plane_r)" in open(SRC).read()
    case, params = ref.seeded_case(h, w)
    raised = tr.raised_biases(case, params, size)
    with torch.no_grad():
        _, (z1, z2) = tr.features(*case, *raised, size, 3, "mean", torch.float64, return_preacts=True)
    print("516x512: smallest pre-activations %.3f, %.3f after raising the biases by %.2f, %.2f" % (float(z1.min()), float(z2.min()), float((raised[1] - params[1])[0]), float((raised[3] - params[3])[0])))
    assert float(z1.min()) >= 0.5 and float(z2.min()) >= 0.5
    assert torch.equal(raised[0], params[0]) and torch.equal(raised[2], params[2])


# ---- 5. the arbiter against the reference's recorded gradients -----------------------------------------------------------------------------------------------
FIXTURE_KEYS = {"render": "render", "warped": "warped_image", "w1": "per_view_mlp.0.weight", "b1": "per_view_mlp.0.bias", "w2": "per_view_mlp.2.weight", "b2": "per_view_mlp.2.bias"}
FIXTURE_KEYS.update({mine: "conv_decoder." + theirs for theirs, mine in hourglass.REFERENCE_KEYS.items()})


def fixture():
    """-> (the recorded run, the planes, (w1, b1, w2, b2), the CNN's eighteen tensors): numpy"""
    z, c, made = (np.load(os.path.join(GOLDEN, f)) for f in ("consumer_resized_train.npz", "consumer.npz", "consumer_resized.npz"))
    planes = {k: c["oracle_" + k] for k in ("color", "warped_image", "cam_feat", "camera_ray", "min_depth_diff", "use_first_src_frame_mask")}
    sd = {k[3:]: made[k] for k in made.files if k.startswith("sd/")}
    mlp = tuple(sd["per_view_mlp." + k] for k in ("0.weight", "0.bias", "2.weight", "2.bias"))
    cnn = {mine: sd["conv_decoder." + theirs] for theirs, mine in hourglass.REFERENCE_KEYS.items()}
    return z, planes, mlp, cnn


def test_arbiter_reproduces_the_reference_gradients():
    z, planes, mlp, cnn = fixture()
    assert (int(z["H"]), int(z["W"]), float(z["scale"]), int(z["fixed_bits"])) == (32, 48, 0.5, tr.FIXED_BITS) and z["g"].shape == (3, 32, 48) and z["g"].dtype == np.float32
    assert os.path.getsize(os.path.join(GOLDEN, "consumer_resized_train.npz")) < 1 << 20
    assert all(z[k].dtype.kind in "iuf" for k in z.files)          # data only
    assert len(FIXTURE_KEYS) == 24
    for tag, expo in (("half", False), ("half_exposure", True)):
        got, pred = tr.tail_grads(planes, mlp, cnn, (16, 24), z["g"], 1.0, expo)
        assert abs(np.abs(pred).max() - float(z[tag + "_image_pred_max"])) <= 1e-12
        for k, key in FIXTURE_KEYS.items():
            want = tr.unpack_fixed(z, "%s_grad/%s" % (tag, key))
            top, d = np.abs(want).max(), np.abs(got[k].reshape(want.shape) - want).max()
            print("%-14s %-14s the arbiter is %.3e from the reference's float64 run (max %.3e); its float32 run was %.3e away" % (tag, k, d, top, float(z["%s_d32/%s" % (tag, key)])))
            assert top > 0 and d <= 1e-9 * top, (tag, k, d, top)
            assert 0 < float(z["%s_d32/%s" % (tag, key)]) < 1e-3 * top
    plain, corrected = tr.unpack_fixed(z, "half_grad/render"), tr.unpack_fixed(z, "half_exposure_grad/render")
    assert np.abs(plain - corrected).max() > 1e-3 * np.abs(plain).max()          # the correction did something in the recording
