"""The backward of the hourglass (csrc/hgtrain.hip, include/ibgs_hg_train.h, ibgs_amd.hourglass's training entry points) on a CPU-only box: the C ABI
(header <-> _lib.HGB_EXPORTS <-> the built library), the build registration, the entry point's validation with null pointers and bad sizes (validation
precedes every HIP call), the Python layer's refusals, the restatements of tests/hourglass_bwd_ref.py against torch autograd at float64, the routing rules
against torch's, and the DECIDED cases the GPU tests run on: seeds at which float64 and float32 differentiate the same function (every ReLU pre-activation
at least 4 d_ref from zero, every pool window's gap at least 8 d_ref, d_ref the case's own forward yardstick)."""
import functools
import hashlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ibgs_amd import _build, _lib, hourglass
from tests import hourglass_bwd_ref as bref
from tests import hourglass_ref as ref
from tests import test_gpu_hourglass as fwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "hgtrain.hip")
HEADER = os.path.join(ROOT, "include", "ibgs_hg_train.h")
# the forward unit's two files as sha256.  hourglass.hip's is that of the file after its tile moved to csrc/shared/conv_tile.h, which the backward's
# hgb_conv_kernel runs too: what says that the forward is untouched by this unit is then the header's ABI hash, the kernels each unit defines
# (test_kernels_attributed_to_the_new_unit_and_the_forward_is_untouched, tests/test_hourglass_host.py) and the forward's own device suite; that move kept every
# instantiation's matrix-core instruction count, LDS, occupancy and absence of spills, and the forward's bits
FORWARD_SHA = {os.path.join("ibgs_amd", "csrc", "hourglass.hip"): "2043863632828887246acf850826cfcad793e0b5d1147703b299ba78ad17cb3d",
               os.path.join("include", "ibgs_hourglass.h"): "141e221ca65d13d7447a1fb473be08fb820a2b158e7ebb23acdb56be264438c1"}


def _constants():
    code = _build._code_only(open(SRC).read())
    return {k: int(v) for k, v in re.findall(r"constexpr int (HGB_[A-Z_]+) = (\d+);", code)}


def wgrad_frames():
    """The smallest frames at which a weight gradient is summed from two or more workgroups AND a workgroup takes two or more steps along its strip: three
    tiles of the wgrad kernel (a strip holds at least HGB_MIN_STRIP_TILES of them) down, and across."""
    k = _constants()
    assert k["HGB_MIN_STRIP_TILES"] == 2 and k["HGB_MAX_STRIPS"] >= 2
    return [(k["HGB_MIN_STRIP_TILES"] * k["HGB_WT_H"] + 1, _lib.HG_MIN_SIDE), (_lib.HG_MIN_SIDE, k["HGB_MIN_STRIP_TILES"] * k["HGB_WT_W"] + 1)]


FRAMES = [(4, 4), (5, 7), (16, 24), (17, 67), (4, 17), (17, 4), (35, 37)]
# the first decided seed of a frame and parameter set (a case's seed is the first decided one of 1000 h + w, + 1, ..., + 31)
DECIDED = {(4, 4): (4004, 4004), (5, 7): (5007, 5007), (16, 24): (16024, 16025), (17, 67): (17069, 17069), (4, 17): (4017, 4017), (17, 4): (17004, 17004),
           (35, 37): (35042, 35041)}
KINDS = ("default", "half_dead")


def forward_yardsticks(x, p):
    """-> (float64 stages, {stage: d_ref}) with d_ref = max(|torch float32 - f64|, |chain float32 - f64|) as tests/test_gpu_hourglass._yardsticks forms it,
    for the eight ReLU stages (d1 and f included)."""
    want = ref.forward_ref(x, p)
    t32, chain = ref.torch_composition(x, p, torch.float32), ref.chain_f32(x, p)
    d = {k: max(float(np.abs(t32[k].numpy().astype(np.float64) - want[k]).max()), float(np.abs(chain[k].astype(np.float64) - want[k]).max())) for k in bref.RELU_STAGES}
    return want, d


@functools.lru_cache(maxsize=None)
def decided_seed(h, w, kind):
    """The seed search: the first decided seed of the case.  Asserts that there is one, and prints it."""
    p = fwd._params(kind)
    for seed in range(1000 * h + w, 1000 * h + w + 32):
        x = ref.seeded_input(seed, h, w)
        _, d = forward_yardsticks(x, p)
        if bref.decided(x, p, d):
            print("%d x %d %s: decided seed %d" % (h, w, kind, seed))
            return seed
    assert False, "no decided seed among 32 for %d x %d %s" % (h, w, kind)


# ---- the ABI and the build -----------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(["ibgs_hgb_required_scratch", "ibgs_hgb_backward"]) == sorted(_lib.HGB_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    args = re.search(r"ibgs_hgb_backward\((.*?)\);", text, re.S).group(1)
    layers = [(n, n) for n, _, _, _ in hourglass.LAYERS]
    assert re.findall(r"const float\* (\w+)_w,\s*const float\* (\w+)_b", args) == layers
    assert re.findall(r"float\* grad_(\w+)_w,\s*float\* grad_(\w+)_b", args) == layers
    assert args.startswith("void* stream, int32_t H, int32_t W, const float* x,") and args.rstrip().endswith("void* scratch, size_t scratch_bytes")
    assert len(built_lib.ibgs_hgb_backward.argtypes) == 4 + 18 + 5 + 18 + 2 == len(args.split(","))
    # the other export lists keep their lengths
    assert len(_lib.HG_EXPORTS) == 2 and len(_lib.CAGG_EXPORTS) == 4 and len(_lib.SSIM_EXPORTS) == 4 and len(_lib.DTU_EXPORTS) == 8 and len(_lib.PCREG_EXPORTS) == 8
    assert len(_lib.GEOLOSS_EXPORTS) == 6 and not any("_hgb_" in n for n in _lib.EXPORTS + _lib.HG_EXPORTS + _lib.CAGG_EXPORTS)


def test_kernels_attributed_to_the_new_unit_and_the_forward_is_untouched():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["hgb_add_kernel", "hgb_conv_kernel", "hgb_unpool_kernel", "hgb_unup_kernel", "hgb_wgrad_kernel", "hgb_wsum_kernel"]
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "hgtrain"]
    for k in kernels:
        assert _build.tu_of(k) == "hgtrain", k
        assert not any(sub in k for sub in others), k
    assert _build.tu_of("hg_conv3_kernel") == "hourglass"
    at = [i for i, (sub, tu) in enumerate(_build.KERNEL_TU) if tu == "hgtrain"]
    assert len(at) == 1 and 0 < at[0] < len(_build.KERNEL_TU) - 1
    assert _build.SOURCES.index("hgtrain") < _build.SOURCES.index("hourglass") and "hgtrain" in _build.UNIT_HEADERS and "hgtrain" in _build.tu_shas()
    assert "hgtrain" not in _build.EXTRA and _build.compile_flags("hgtrain") == _build.compile_flags("hourglass")
    assert "hourglass" not in os.path.basename(SRC)
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "shared/hg_net.h", "shared/conv_tile.h", "../../include/ibgs_hourglass.h", "../../include/ibgs_hg_train.h"]
    assert [os.path.basename(h) for h in _build.UNIT_HEADERS["hgtrain"]] == ["ibgs_hg_train.h", "ibgs_hourglass.h", "hg_net.h", "conv_tile.h"]
    code = _build._code_only(src)
    assert "atomic" not in code.lower() and "asm" not in code
    tile = _build._code_only(open(os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "conv_tile.h")).read())          # the 16 x 16 tile it shares with the forward and lpips.hip
    assert "mfma_f32_16x16x4f32" in tile and "ct_mfma(" in code and "__builtin_amdgcn_mfma" not in code
    k = _constants()
    assert k["HGB_WT_H"] == 8 and k["HGB_WT_W"] == 16 and "HGB_TILE" not in k and "HGB_THREADS" not in k
    assert re.search(r"constexpr int CT_TILE = 16;", tile) and re.search(r"constexpr int CT_THREADS = 256;", tile) and re.search(r"constexpr int HGB_THREADS = CT_THREADS;", code)
    assert re.search(r"__launch_bounds__\(HGB_THREADS, 2\) hgb_conv_kernel", code)
    assert re.search(r"const dim3 grid\(\(unsigned\)\(\(w \+ CT_TILE - 1\) / CT_TILE\), \(unsigned\)\(\(h \+ CT_TILE - 1\) / CT_TILE\)\);", code)
    for rel, sha in FORWARD_SHA.items():
        assert hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() == sha, rel


def test_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_hgb_required_scratch
    assert need(1080, 1920) % 128 == 0 and need(1080, 1920) > 4 * 38 * 1080 * 1920 * 4 and need(4, 4) % 128 == 0 and need(4, 4) > 0
    for h, w in ((3, 8), (8, 3), (0, 8), (-1, 8), (8193, 8), (8, 8193), (1 << 40, 8)):
        assert need(h, w) == 0, (h, w)
    err = lambda: built_lib.ibgs_last_error()
    bwd = built_lib.ibgs_hgb_backward
    big = 1 << 40
    # (stream, H, W, x, 18 parameters, burned, stages arena, grad_residual, grad_image_pred, grad_x, 18 gradients, scratch, bytes)
    good = [None, 8, 8, 128] + [128] * 18 + [1.0, 128, 128, 128, 128] + [128] * 18 + [128, big]
    for k, v in ((1, 3), (2, 3), (1, 0), (2, -5), (1, 8193), (2, 8193)):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and b"out of range" in err(), (k, v)
    args = list(good)
    args[3] = None
    assert bwd(*args) < 0 and b"null input" in err()
    for i, (layer, _, _, _) in enumerate(hourglass.LAYERS):
        for j, what in enumerate((b"weight", b"bias")):
            args = list(good)
            args[4 + 2 * i + j] = None
            assert bwd(*args) < 0 and b"null parameters" in err() and layer.encode() in err() and what in err(), (layer, what)
            args = list(good)
            args[27 + 2 * i + j] = None
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
    args[26:45] = [None] * 19
    assert bwd(*args) < 0 and b"null outputs" in err()
    for k, v, msg in ((45, None, b"null scratch"), (45, 64, b"aligned"), (46, need(8, 8) - 1, b"needed")):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and msg in err(), k


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    net = hourglass.HourglassCNN()
    x = torch.rand(1, 38, 8, 9)
    g = torch.rand(3, 8, 9)
    arena = torch.empty(built_lib.ibgs_hg_required_scratch(8, 9), dtype=torch.uint8)
    for call in (lambda t, n: hourglass.hourglass_backward(t, n, arena, g), lambda t, n: hourglass.hourglass_train(t, n), lambda t, n: hourglass.hourglass_train(t, n, 0.5)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call(x, net)
        with pytest.raises(ValueError, match="implies hidden_dim = 70"):
            call(torch.rand(1, 70, 8, 8), net)
        with pytest.raises(ValueError, match="out of range"):
            call(torch.rand(38, 3, 8), net)
        with pytest.raises(ValueError, match="must be"):
            call(torch.rand(2, 38, 8, 8), net)
        with pytest.raises(TypeError, match="HourglassCNN"):
            call(x, torch.nn.Conv2d(38, 3, 1))
        with pytest.raises(TypeError, match="cnn_input"):
            call(x.numpy(), net)
        bad = hourglass.HourglassCNN()
        bad.dec2_w = torch.nn.Parameter(torch.zeros(19, 39, 3, 3))
        with pytest.raises(ValueError, match="dec2_w must be"):
            call(x, bad)
    # fuse_color_train
    full = hourglass.ColorAggregationNet()
    h, w = 6, 8
    pkg = dict(render=torch.rand(3, h, w), warped_image=torch.rand(9, h, w), cam_feat=torch.rand(12, h, w), camera_ray=torch.rand(3, h, w), min_depth_diff=torch.rand(1, h, w))
    with pytest.raises(RuntimeError, match="MI355X only"):
        hourglass.fuse_color_train(pkg, full)
    with pytest.raises(TypeError, match="ColorAggregationNet"):
        hourglass.fuse_color_train(pkg, full.cnn)
    with pytest.raises(KeyError, match="cam_feat"):
        hourglass.fuse_color_train({k: v for k, v in pkg.items() if k != "cam_feat"}, full)
    with pytest.raises(ValueError, match="out of range"):
        hourglass.fuse_color_train(dict(pkg, render=torch.rand(3, 3, w)), full)
    # the forward-only entry points keep refusing grad mode, in their words
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\).*training keeps torch's CNN"):
        hourglass.fuse_color(pkg, full)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\).*training keeps torch's CNN"):
        hourglass.hourglass_forward(x, net)


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(5, 7), (16, 24)])
def test_backward_ref_is_torch_autograd_at_float64(h, w):
    p = fwd._params("default")
    x = ref.seeded_input(1000 * h + w, h, w)
    g = np.random.default_rng(h * w)
    g_res, g_ip = g.standard_normal((3, h, w)), g.standard_normal((3, h, w))
    stages = ref.forward_ref(x, p, 0.75)
    for a, b in ((g_res, g_ip), (g_res, None), (None, g_ip)):
        mine, theirs = bref.backward_ref(x, p, stages, a, b, 0.75), bref.torch_grads(x, p, a, b, 0.75, torch.float64)
        for k in bref.GRADS:
            assert mine[k].dtype == np.float64 and mine[k].shape == theirs[k].shape, k
            assert np.abs(mine[k] - theirs[k]).max() <= 1e-12 * np.abs(theirs[k]).max(), k
    chain = bref.backward_chain_f32(x, p, stages, g_res.astype(np.float32), g_ip.astype(np.float32), 0.75)
    for k in bref.GRADS:          # the float32 chain evaluates the same gradients: within float32 rounding of them, and not identical
        scale = np.abs(mine[k]).max()
        assert chain[k].dtype == np.float32 and np.abs(chain[k] - bref.backward_ref(x, p, stages, g_res, g_ip, 0.75)[k]).max() <= 2.0 ** -18 * scale, k


def test_pool_transposed_tie_rule_is_torchs():
    g = np.random.default_rng(3)
    t = g.integers(1, 3, size=(4, 7, 9)).astype(np.float64)          # windows of equal positive values, an odd last row and column
    t[0, :2, :2] = 2.0
    gp = g.standard_normal((4, 3, 4))
    tt = torch.tensor(t, requires_grad=True)
    F.max_pool2d(tt[None], 2).backward(torch.tensor(gp)[None])
    mine = bref.pool_bwd(gp, t)
    assert np.array_equal(mine, tt.grad.numpy()) and np.all(mine[:, 6] == 0) and np.all(mine[:, :, 8] == 0)
    assert mine[0, 0, 0] == gp[0, 0, 0] and mine[0, 0, 1] == 0 and mine[0, 1, 0] == 0 and mine[0, 1, 1] == 0


def test_up_transposed_is_autograd_of_nearest_interpolation():
    for n_out in range(4, 68):
        n_in = n_out // 2
        g = np.random.default_rng(n_out).standard_normal((2, n_out, 5))
        src = torch.zeros(1, 2, n_in, 2, dtype=torch.float64, requires_grad=True)
        F.interpolate(src, size=(n_out, 5), mode="nearest").backward(torch.tensor(g)[None])
        assert np.abs(bref.up_bwd(g, n_in, 2) - src.grad[0].numpy()).max() <= 1e-14, n_out
        src = torch.zeros(1, 2, 2, n_in, dtype=torch.float64, requires_grad=True)
        F.interpolate(src, size=(5, n_out), mode="nearest").backward(torch.tensor(g.transpose(0, 2, 1).copy())[None])
        assert np.abs(bref.up_bwd(g.transpose(0, 2, 1).copy(), 2, n_in) - src.grad[0].numpy()).max() <= 1e-14, n_out
    counts = np.bincount(ref.up_index(5, 2))
    assert list(counts) == [3, 2]          # uneven children


# ---- the decided cases -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FRAMES)
def test_every_listed_case_has_its_decided_seed(h, w):
    for kind, want in zip(KINDS, DECIDED[(h, w)]):
        assert decided_seed(h, w, kind) == want, (h, w, kind)


def test_the_wgrad_frames_have_decided_seeds():
    frames = wgrad_frames()
    assert frames == [(17, 4), (4, 33)]
    for h, w in frames:
        for kind in KINDS:
            assert 0 <= decided_seed(h, w, kind) - (1000 * h + w) < 32
