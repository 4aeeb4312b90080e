"""The half-precision backward of the hourglass (csrc/hghtrain.hip, include/ibgs_hg_half_train.h, the `precision` keyword of ibgs_amd.hourglass's training
entry points) on a CPU-only box: the C ABI (header <-> _lib.HGHT_EXPORTS <-> the built library), the build registration and what the source may not
contain, the entry point's validation with null pointers and bad sizes (validation precedes every HIP call), the keywords' refusals (before any GPU work),
the arbiter of tests/hghalf_bwd_ref.py against tests/hourglass_bwd_ref.backward_ref, the yardstick's reproducibility and the scale rule."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, hourglass, resample_train
from tests import hghalf_bwd_ref as hbref
from tests import hourglass_bwd_ref as bref
from tests import hourglass_ref as ref
from tests import test_gpu_hourglass as fwd
from tests.test_resample_train_host import DEFINES, _csrc_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "hghtrain.hip")
TILE_H = os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "conv_tile_f16.h")          # the f16 tile, the octet read and fuse_input as this unit and hghalf.hip share them
HEADER = os.path.join(ROOT, "include", "ibgs_hg_half_train.h")


# ---- the ABI and the build -----------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(["ibgs_hgh_train_required_scratch", "ibgs_hgh_train_backward"]) == sorted(_lib.HGHT_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    args = re.search(r"ibgs_hgh_train_backward\((.*?)\);", text, re.S).group(1)
    layers = [(n, n) for n, _, _, _ in hourglass.LAYERS]
    assert re.findall(r"const float\* (\w+)_w,\s*const float\* (\w+)_b", args) == layers
    assert re.findall(r"float\* grad_(\w+)_w,\s*float\* grad_(\w+)_b", args) == layers
    assert args.startswith("void* stream, int32_t H, int32_t W, const float* x,") and re.sub(r"\s+", " ", args).endswith("void* scratch, size_t scratch_bytes")
    assert len(built_lib.ibgs_hgh_train_backward.argtypes) == 4 + 18 + 8 + 18 + 2 == len(args.split(","))
    defines = dict(re.findall(r"#define\s+IBGS_(HGHT_[A-Z_]+)\s+(\d+)", text))
    assert defines == {"HGHT_E_TARGET": str(_lib.HGHT_E_TARGET), "HGHT_SCALE_AUTO": str(_lib.HGHT_SCALE_AUTO), "HGHT_SCALE_FIXED": str(_lib.HGHT_SCALE_FIXED),
                       "HGHT_PACKED_WEIGHT_BYTES": str(_lib.HGHT_PACKED_WEIGHT_BYTES)}
    assert _lib.HGHT_E_TARGET == hbref.E_TARGET
    # the other export lists keep their lengths
    assert len(_lib.HG_EXPORTS) == 2 and len(_lib.HGB_EXPORTS) == 2 and len(_lib.HGH_EXPORTS) == 2
    assert not any("_hgh_train" in n for n in _lib.EXPORTS + _lib.HG_EXPORTS + _lib.HGB_EXPORTS + _lib.HGH_EXPORTS)


def test_build_registration_and_the_kernels():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["hght_conv3_kernel", "hght_pack_kernel", "hght_scale_kernel", "hght_status_kernel", "hght_unpool_kernel", "hght_unup_kernel", "hght_wgrad_kernel",
                       "hght_wsum_kernel"]
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "hghtrain"]
    for k in kernels:
        assert _build.tu_of(k) == "hghtrain", k
        assert not any(sub in k for sub in others), k          # whatever the order of the table
    assert [e for e in _build.KERNEL_TU if e[1] == "hghtrain"] == [("hght_", "hghtrain")]
    assert _build.tu_of("hgh_conv3_kernel") == "hghalf" and _build.tu_of("hgb_wgrad_kernel") == "hgtrain" and _build.tu_of("hg_conv3_kernel") == "hourglass"
    # registered like every other unit: one table of sources, one of headers, a profile stamp
    assert _build.SOURCES[-1] == "hourglass" and _build.SOURCES.index("hghalf") < _build.SOURCES.index("hghtrain") < _build.SOURCES.index("hourglass")
    assert "hghtrain" in _build.UNIT_HEADERS and "hghtrain" in _build.tu_shas() and _build.UNSTAMPED == ("export",)
    assert not hasattr(_build, "SIDE_UNITS") and not hasattr(_build, "_headers_of")
    assert "hghtrain" not in _build.EXTRA and _build.compile_flags("hghtrain") == _build.compile_flags("hghalf")
    assert [os.path.basename(h) for h in _build.UNIT_HEADERS["hghtrain"]] == ["ibgs_hg_half_train.h", "ibgs_hg_half.h", "ibgs_hourglass.h", "hg_net.h", "conv_tile.h",
                                                                              "conv_tile_f16.h"]
    assert all(os.path.exists(h) for h in _build.UNIT_HEADERS["hghtrain"])
    for h in _build.UNIT_HEADERS["hghtrain"]:
        assert _build._newest_dep() >= os.path.getmtime(h)
    assert {k for k, hs in _build.UNIT_HEADERS.items() if TILE_H in [os.path.normpath(h) for h in hs]} == {"hghalf", "hghtrain"}
    for unit in ("hghtrain", "hghalf"):          # the table is the truth: what the unit and its shared headers include outside csrc/*.h and include/ibgs_rast.h
        seen, todo = set(), [os.path.join(os.path.dirname(SRC), unit + ".hip")]
        while todo:
            f = todo.pop()
            for inc in re.findall(r'#include "([^"]+)"', open(f).read()):
                path = os.path.normpath(os.path.join(os.path.dirname(f), inc))
                if os.path.dirname(path) != os.path.dirname(SRC) and os.path.basename(path) != "ibgs_rast.h" and path not in seen:
                    seen.add(path)
                    todo.append(path)
        assert seen == {os.path.normpath(h) for h in _build.UNIT_HEADERS[unit]}, unit
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "shared/hg_net.h", "shared/conv_tile.h", "shared/conv_tile_f16.h", "../../include/ibgs_hourglass.h",
                                                      "../../include/ibgs_hg_half.h", "../../include/ibgs_hg_half_train.h"]
    mine, tile = _build._code_only(src), _build._code_only(open(TILE_H).read())
    code = mine + "\n" + tile          # the unit's own code and the shared header's: the pins hold on both
    assert "asm" not in code.lower()          # builtins only
    assert sorted(set(re.findall(r"\b(atomic\w*)\s*\(", code))) == ["atomicAdd", "atomicMax"] and "atomic" not in tile          # integer words only: the control block's
    assert re.search(r"struct HghtCtrl \{ unsigned m_bits; int k; int nonfinite; unsigned ticket; \};", mine)
    assert "__builtin_amdgcn_mfma_f32_16x16x32_f16" in code and len(re.findall(r"__builtin_amdgcn_mfma_\w+", code)) == 1 and "16x16x4f32" not in code
    assert "__builtin_amdgcn_mfma" not in mine          # the one builtin is the header's
    assert "pkrtz" not in code and "(_Float16)" in mine and "(_Float16)" in tile          # conversions are casts: to nearest even
    assert re.search(r"constexpr int HGHT_E_TARGET = IBGS_HGHT_E_TARGET;", mine)


def test_the_f16_tile_is_defined_once_and_both_units_call_it():
    """csrc/shared/conv_tile_f16.h: the mfma wrapper, the octet read, the main loop of the implicit GEMM, an accumulator tile as an operand, fuse_input on
    [d1 | h(x)] (the forward's last launch and the backward's recomputed head: no test could see two copies drift, neither d1 nor f is stored by the forward)
    and the order of a forward fragment's elements."""
    code = _csrc_code()
    shared = ("cth_mfma", "cth_round", "cth_read", "cth_start", "cth_conv3", "cth_as_operand", "cth_fuse_input", "cth_frag3_channel", "cth_acc_channel", "cth_frag1_channel")
    for name in shared:
        assert [f for f, text in code.items() for _ in re.findall(DEFINES % name, text, re.M)] == ["shared/conv_tile_f16.h"], name
    units = ("hghalf.hip", "hghtrain.hip")
    users = lambda pattern: sorted(f for f, text in code.items() if re.search(pattern, text))
    for name in shared:          # no other user, and no second name for the same thing
        assert set(users(r"\b%s\b" % name)) <= {"shared/conv_tile_f16.h", "hghalf.hip", "hghtrain.hip"}, name
    assert users(r"\bhgh?t?_(?:mfma|round|octets|frags3?|as_operand|h8|h4|f32x4)\b") == [] and users(r"\bHGHT?_(?:ROWS|WIN|NPIX|PSTRIDE|XO|FUSE_STEPS)\b") == []
    for unit in units:
        for call in (r"cth_mfma\(", r"cth_conv3<CA, CB, COUT, \w+>\(acc, a\.a, a\.b, a\.wfrag,", r"cth_start<COUT>\(acc, a\.bias, kq\)", r"cth_as_operand<3, (?:true|false)>\(",
                     r"cth_fuse_input<(?:true|false)>\(f, acc, a\.fuse_frag, a\.fuse_b, a\.xh, h, w\)", r"= cth_frag3_channel\(o, j, L\.ca, L\.cb\)",
                     r"= cth_frag1_channel\(s, kq, j, L\.ca, L\.cb\)"):
            assert re.search(call, code[unit]), (unit, call)
        # the unit's own text holds none of the shared state: no maximum of a 2 x 2 window, no staged window, no vector type, no second lane-map constant
        assert "__builtin_elementwise_max" not in code[unit] and not re.search(r"__shared__ \w+ s_(?:in|w)\[", code[unit]), unit
        assert not re.search(r"typedef\s+_Float16\b[^;]*ext_vector_type", code[unit]) and "__builtin_amdgcn_mfma" not in code[unit], unit
    # the octet read: the chunk loop and h(x) in the header; G and the two inputs of a weight gradient in hghtrain.hip (the forward reads through cth_conv3 only)
    calls = {f: re.findall(r"cth_read<(\w+)>\(", text) for f, text in code.items() if re.search(r"cth_read<", text)}
    assert calls == {"shared/conv_tile_f16.h": ["MODE", "CT_PLAIN"], "hghtrain.hip": ["CT_PLAIN", "MODE", "CT_PLAIN"]}
    tile = code["shared/conv_tile_f16.h"]
    assert len(re.findall(r"__builtin_elementwise_max", tile)) == 3 and len(re.findall(r"__shared__ cth_h8 s_(?:in|w)\[", tile)) == 2 and len(re.findall(r"__syncthreads\(\)", tile)) == 2
    assert re.search(r"typedef _Float16 cth_h8 __attribute__\(\(ext_vector_type\(8\)\)\);", tile)
    # the two kernels differ in how the accumulators start and in the epilogue, and the head hands the product clamped and rounded values
    assert re.search(r"ct_f32x4 acc\[MT\]\[CT_ROWS\] = \{\};\n\s*if constexpr \(EPI == HGHT_EPI_HEAD\) cth_start<COUT>", code["hghtrain.hip"])
    assert re.search(r"cth_fuse_input<true>", code["hghalf.hip"]) and re.search(r"cth_fuse_input<false>", code["hghtrain.hip"])


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_hgh_train_required_scratch
    assert need(1080, 1920) % 128 == 0 and need(4, 4) % 128 == 0 and need(4, 4) > _lib.HGHT_PACKED_WEIGHT_BYTES
    assert 1.0e9 < need(1080, 1920) < 1.6e9
    for h, w in ((3, 8), (8, 3), (0, 8), (-1, 8), (8193, 8), (8, 8193), (1 << 40, 8)):
        assert need(h, w) == 0, (h, w)
    err = lambda: built_lib.ibgs_last_error()
    bwd = built_lib.ibgs_hgh_train_backward
    big = 1 << 40
    # (stream, H, W, x, 18 parameters, burned, forward arena, grad_residual, grad_image_pred, scale mode, k, status, grad_x, 18 gradients, scratch, bytes)
    good = [None, 8, 8, 128] + [128] * 18 + [1.0, 128, 128, 128, 0, 0, None, 128] + [128] * 18 + [128, big]
    for k, v in ((1, 3), (2, 3), (1, 0), (2, -5), (1, 8193), (2, 8193)):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and b"out of range" in err() and b"hgh_train_backward" in err(), (k, v)
    args = list(good)
    args[3] = None
    assert bwd(*args) < 0 and b"null input" in err()
    for i, (layer, _, _, _) in enumerate(hourglass.LAYERS):
        for j, what in enumerate((b"weight", b"bias")):
            args = list(good)
            args[4 + 2 * i + j] = None
            assert bwd(*args) < 0 and b"null parameters" in err() and layer.encode() in err() and what in err(), (layer, what)
            args = list(good)
            args[30 + 2 * i + j] = None
            assert bwd(*args) < 0 and b"null gradients" in err() and layer.encode() in err() and what in err(), (layer, what)
    args = list(good)
    args[23] = None
    assert bwd(*args) < 0 and b"null stages arena" in err()
    args = list(good)
    args[23] = 64
    assert bwd(*args) < 0 and b"aligned" in err()
    args = list(good)
    args[24] = args[25] = None
    assert bwd(*args) < 0 and b"null upstream" in err()
    args = list(good)
    args[26] = 2
    assert bwd(*args) < 0 and b"scale_mode" in err()
    args = list(good)
    args[26], args[27] = 1, 301
    assert bwd(*args) < 0 and b"grad_scale_log2" in err()
    args = list(good)
    args[29:48] = [None] * 19
    assert bwd(*args) < 0 and b"null outputs" in err()
    for k, v, msg in ((48, None, b"null scratch"), (48, 64, b"aligned"), (49, need(8, 8) - 1, b"needed")):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and msg in err(), k


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------------------------
def test_keywords_are_validated_before_any_gpu_work(built_lib):
    net = hourglass.HourglassCNN()
    x = torch.rand(1, 38, 8, 9)
    g = torch.rand(3, 8, 9)
    arena = torch.empty(built_lib.ibgs_hgh_required_scratch(8, 9), dtype=torch.uint8)
    calls = (lambda **kw: hourglass.hourglass_backward(x, net, arena, g, **kw), lambda **kw: hourglass.hourglass_train(x, net, **kw))
    for call in calls:
        for bad in ("bfloat16", "half", torch.float16, None):
            with pytest.raises(ValueError, match=r'"float32" or "float16"'):
                call(precision=bad)
        for bad in (1.0, "3", True, torch.tensor(3)):
            with pytest.raises(TypeError, match="grad_scale_log2 must be None"):
                call(precision="float16", grad_scale_log2=bad)
        with pytest.raises(ValueError, match="out of range"):
            call(precision="float16", grad_scale_log2=301)
        for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)[::2], [0, 0]):
            with pytest.raises(ValueError, match="status must be a contiguous int32 tensor of two words"):
                call(precision="float16", status=bad)
        with pytest.raises(ValueError, match='belong to precision="float16"'):          # the float32 unit has no scale
            call(grad_scale_log2=3)
        with pytest.raises(ValueError, match='belong to precision="float16"'):
            call(status=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="MI355X only"):          # and only then the device
            call(precision="float16", grad_scale_log2=3, status=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match='belong to precision="float16"'):
        hourglass.hourglass_backward(x, net, arena, g, return_decisions=True)
    for call in calls:          # the options are keyword only, and nothing else is swallowed
        with pytest.raises(TypeError, match="unexpected keyword argument 'precison'"):
            call(precison="float16")
    with pytest.raises(TypeError, match="unexpected keyword argument 'return_decisions'"):
        hourglass.hourglass_train(x, net, return_decisions=True)
    with pytest.raises(TypeError):
        hourglass.hourglass_train(x, net, None, "float16")
    full = hourglass.ColorAggregationNet()
    h, w = 6, 8
    pkg = dict(render=torch.rand(3, h, w), warped_image=torch.rand(9, h, w), cam_feat=torch.rand(12, h, w), camera_ray=torch.rand(3, h, w), min_depth_diff=torch.rand(1, h, w))
    # the two tails keep their signatures: their precision is the block's
    for bad in ("bfloat16", None):
        with pytest.raises(ValueError, match=r'train_precision: precision must be "float32" or "float16"'):
            with hourglass.train_precision(bad):
                pass
    with hourglass.train_precision("float16"):
        with pytest.raises(TypeError, match="grad_scale_log2 must be None"):          # the block's precision is hourglass_train's default: its options are checked
            hourglass.hourglass_train(x, net, grad_scale_log2=1.5)
        with pytest.raises(ValueError, match='belong to precision="float16"'):          # ... and the keyword overrides the block
            hourglass.hourglass_train(x, net, precision="float32", grad_scale_log2=3)
        assert hourglass._TRAINING.precision == "float16"
        with hourglass.train_precision("float32"):
            assert hourglass._TRAINING.precision == "float32"
        assert hourglass._TRAINING.precision == "float16"
        for call in (lambda: hourglass.fuse_color_train(pkg, full), lambda: resample_train.fuse_color_train_scaled(pkg, full, 0.75)):
            with pytest.raises(RuntimeError, match="MI355X only"):
                call()
        with pytest.raises(ValueError, match="ends the block"):
            with hourglass.train_precision("float32"):
                raise ValueError("an exception ends the block")
        assert hourglass._TRAINING.precision == "float16"
    assert hourglass._TRAINING.precision == "float32"
    import threading
    other = []
    with hourglass.train_precision("float16"):
        t = threading.Thread(target=lambda: other.append(getattr(hourglass._TRAINING, "precision", "float32")))
        t.start()
        t.join()
    assert other == ["float32"]          # per thread
    for fn in (hourglass.hourglass_train, hourglass.hourglass_backward):
        assert list(inspect.signature(fn).parameters.values())[-1].kind is inspect.Parameter.VAR_KEYWORD


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------------------------
def test_arbiter_with_the_float64_decisions_is_backward_ref():
    h, w = 16, 24
    p = fwd._params("default")
    x = ref.seeded_input(1000 * h + w, h, w)
    g = np.random.default_rng(h * w)
    g_res, g_ip = g.standard_normal((3, h, w)), g.standard_normal((3, h, w))
    stages = ref.forward_ref(x, p, 0.75)
    decisions = hbref.decisions_of(stages)
    assert sorted(decisions) == sorted(bref.RELU_STAGES) and all(v.dtype == np.bool_ for v in decisions.values())
    for a, b in ((g_res, g_ip), (g_res, None), (None, g_ip)):
        mine, theirs = hbref.backward_decided(x, p, stages, decisions, stages, a, b, 0.75), bref.backward_ref(x, p, stages, a, b, 0.75)
        for k in bref.GRADS:
            assert mine[k].dtype == np.float64 and mine[k].shape == theirs[k].shape, k
            assert np.abs(mine[k] - theirs[k]).max() <= 1e-12 * np.abs(theirs[k]).max(), k
    # a handed decision is what decides: with f's mask cleared nothing but final's gradients and the burned-in image gradient is left
    dead = dict(decisions, f=np.zeros_like(decisions["f"]))
    out = hbref.backward_decided(x, p, stages, dead, stages, g_res, g_ip, 0.75)
    assert np.all(out["dec1_w"] == 0) and np.all(out["x"][:35] == 0) and np.array_equal(out["x"][35:], 0.75 * g_ip) and np.abs(out["final_w"]).max() > 0


def test_the_yardstick_is_reproducible():
    h, w = 5, 7
    p = fwd._params("default")
    x = ref.seeded_input(1000 * h + w, h, w)
    g = np.random.default_rng(3)
    g_res, g_ip = g.standard_normal((3, h, w)).astype(np.float32), g.standard_normal((3, h, w)).astype(np.float32)
    k = hbref.scale_k(np.abs(g_res + g_ip).max())
    a, da, pa = hbref.autocast_backward(x, p, g_res, g_ip, 0.75, k)
    b, db, pb = hbref.autocast_backward(x, p, g_res, g_ip, 0.75, k)
    assert sorted(a) == sorted(bref.GRADS) and all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[n], b[n]) for n in a) and all(np.array_equal(da[n], db[n]) for n in da) and all(np.array_equal(pa[n], pb[n]) for n in pa)
    # it differentiates the same network: within binary16's reach of the arbiter on its own decisions
    stages = ref.forward_ref(x, p, 0.75)
    want = hbref.backward_decided(x, p, stages, da, pa, g_res, g_ip, 0.75)
    for n in bref.GRADS:
        assert 0 < np.abs(a[n] - want[n]).max() < 2.0 ** -5 * np.abs(want[n]).max(), n


def test_the_scale_rule():
    e = hbref.E_TARGET
    below = float(np.nextafter(np.float32(0.125), np.float32(0)))
    cases = ((0.125, e + 3), (below, e + 4), (1.0, e), (1.5, e), (2.0 ** 20, e - 20), (2.0 ** -140, e + 140), (float(np.float32(3 * 2.0 ** -149)), e + 148), (0.0, 0),
             (float("inf"), 0), (float("nan"), 0))
    for m, want in cases:
        assert hbref.scale_k(m) == want, (m, want)
        if want and np.isfinite(m):          # the scaled maximum lies in [2^E_TARGET, 2^(E_TARGET + 1)): far from binary16's overflow and its subnormals
            assert 2.0 ** e <= float(np.ldexp(np.float64(m), want)) < 2.0 ** (e + 1)
    assert 2.0 ** (e + 1) < 65504
