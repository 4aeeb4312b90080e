"""The half-precision hourglass unit on a CPU-only box: the C ABI (include/ibgs_hg_half.h <-> _lib.HGH_EXPORTS <-> the built library), the build
registration, the kernel list and what the source may not contain, the arena's documented layout and every validation message of ibgs_hgh_forward with null
pointers and bad sizes (validation precedes every HIP call), the `precision` keyword's refusals (which run before any GPU work), the recorded autocast run of
the reference's own network (tests/golden/hghalf.npz) against tests/hghalf_ref.autocast_composition, and that composition's distance from the float64
arbiter on the fixture inputs (printed: DESIGN.md section 15 quotes it)."""
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, hourglass
from tests import hghalf_ref as href
from tests import hourglass_ref as ref
from tests.test_hourglass_host import _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "hghalf.hip")
TILE_H = os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "conv_tile_f16.h")          # the f16 tile, the octet read and fuse_input as hghalf.hip and hghtrain.hip share them
HEADER = os.path.join(ROOT, "include", "ibgs_hg_half.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _decoder_params(z):
    return {name + s: z["sd/conv_decoder.%s.%s" % (theirs, t)] for name, theirs in ref.REFERENCE_NAMES.items() for s, t in (("_w", "weight"), ("_b", "bias"))}


# ---- the ABI and the build ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(["ibgs_hgh_required_scratch", "ibgs_hgh_forward"]) == sorted(_lib.HGH_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    # the same eighteen parameters, same names, same order as ibgs_hg_forward; the rest of the signature alike
    theirs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_hourglass.h")).read(), flags=re.S)
    mine_args = re.sub(r"\s+", " ", re.search(r"ibgs_hgh_forward\((.*?)\);", text, re.S).group(1))
    their_args = re.sub(r"\s+", " ", re.search(r"ibgs_hg_forward\((.*?)\);", theirs, re.S).group(1))
    assert mine_args == their_args
    assert re.findall(r"const float\* (\w+)_w,\s*const float\* (\w+)_b", mine_args) == [(n, n) for n, _, _, _ in hourglass.LAYERS]
    assert dict(re.findall(r"#define\s+IBGS_(HGH_[A-Z_]+)\s+(\d+)", text)) == {"HGH_PACKED_WEIGHT_BYTES": str(_lib.HGH_PACKED_WEIGHT_BYTES)}
    # the other export lists are untouched
    assert len(_lib.HG_EXPORTS) == 2 and len(_lib.HGB_EXPORTS) == 2 and len(_lib.CAGG_EXPORTS) == 4
    others = (_lib.EXPORTS + _lib.SSIM_EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS + _lib.GEOLOSS_EXPORTS
              + _lib.CAGG_EXPORTS + _lib.HG_EXPORTS + _lib.HGB_EXPORTS)
    assert not any("_hgh_" in n for n in others) and not any("_hg_" in n or "_hgb_" in n for n in _lib.HGH_EXPORTS)


def test_build_registration_and_the_kernels():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["hgh_conv3_kernel", "hgh_pack_kernel"]          # the packing launch and ONE templated convolution
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "hghalf"]
    for k in kernels:
        assert k.startswith("hgh_") and _build.tu_of(k) == "hghalf", k
        assert not any(sub in k for sub in others), k
    at = [i for i, (sub, tu) in enumerate(_build.KERNEL_TU) if tu == "hghalf"]
    assert len(at) == 1 and 0 < at[0] < len(_build.KERNEL_TU) - 1 and _build.KERNEL_TU[at[0]] == ("hgh_", "hghalf")
    assert _build.KERNEL_TU[-1] == ("hg_", "hourglass") and _build.KERNEL_TU[0] == ("meval_", "mesh_eval")
    assert _build.SOURCES[-1] == "hourglass" and _build.SOURCES.index("hghalf") < _build.SOURCES.index("hourglass")
    assert "hghalf" in _build.UNIT_HEADERS and "hghalf" in _build.tu_shas() and "hghalf" not in _build.EXTRA
    assert _build.compile_flags("hghalf") == _build.compile_flags("hourglass")
    assert [os.path.basename(h) for h in _build.UNIT_HEADERS["hghalf"]] == ["ibgs_hg_half.h", "ibgs_hourglass.h", "hg_net.h", "conv_tile.h", "conv_tile_f16.h"]
    assert all(os.path.exists(h) for h in _build.UNIT_HEADERS["hghalf"])
    # the float32 unit's kernel still goes where it went
    assert _build.tu_of("hg_conv3_kernel") == "hourglass" and _build.tu_of("hgb_wgrad_kernel") == "hgtrain"
    mine, tile = _build._code_only(src), _build._code_only(open(TILE_H).read())
    code = mine + "\n" + tile          # the unit's own code and the shared header's: the pins hold on both
    assert "atomic" not in code.lower() and "asm" not in code.lower()          # nothing crosses a workgroup; builtins only
    assert "__builtin_amdgcn_mfma_f32_16x16x32_f16" in code and "16x16x4f32" not in code
    assert len(re.findall(r"__builtin_amdgcn_mfma_\w+", code)) == 1 and "__builtin_amdgcn_mfma" not in mine          # the one f16 form, nothing else, and it is the header's
    assert "pkrtz" not in code and "(_Float16)" in mine and "(_Float16)" in tile          # conversions are casts: to nearest even
    assert re.search(r"constexpr int HGH_TILE = 16;", mine) and re.search(r"constexpr int HGH_THREADS = 256;", mine)
    assert re.search(r"static_assert\(HGH_TILE == CT_TILE && HGH_THREADS == CT_THREADS,", mine)          # the tile is conv_tile.h's, which the header includes
    assert re.search(r"const dim3 grid\(\(unsigned\)\(\(a\.w \+ HGH_TILE - 1\) / HGH_TILE\), \(unsigned\)\(\(a\.h \+ HGH_TILE - 1\) / HGH_TILE\)\);", mine)
    assert len(re.findall(r"hgh_launch<", code)) == 7 and len(re.findall(r"hipLaunchKernelGGL\(hgh_pack_kernel", code)) == 1
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "shared/hg_net.h", "shared/conv_tile.h", "shared/conv_tile_f16.h", "../../include/ibgs_hourglass.h",
                                                      "../../include/ibgs_hg_half.h"]
    assert re.findall(r'#include "([^"]+)"', open(TILE_H).read()) == ["conv_tile.h", "hg_net.h"]


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_hgh_required_scratch
    assert _lib.HGH_PACKED_WEIGHT_BYTES == 17600 * 16
    for h, w in ((4, 4), (5, 7), (16, 24), (17, 67), (1080, 1920), (8192, 8192), (4, 8192)):
        total, offs = _layout(h, w, half=True)
        assert need(h, w) == total and total % 128 == 0, (h, w)
        if h * w > 1 << 22:
            continue
        views = hourglass._arena_views(torch.empty(total, dtype=torch.uint8), h, w, half=True)
        assert [n for n, _, _ in hourglass.STAGES] == list(views) == [n for n in offs if n not in ("xh", "packed")]
        base = views["e1"].untyped_storage().data_ptr()
        for (n, ch, level), v in zip(hourglass.STAGES, views.values()):
            cp = (ch + 7) // 8 * 8
            assert v.dtype == torch.float16 and v.data_ptr() - base == offs[n] and v.shape[0] == ch and v.stride() == (1, v.shape[2] * cp, cp), (h, w, n)
        assert tuple(views["b"].shape) == (9, h // 4, w // 4) and tuple(views["u1"].shape) == (38, h, w) and tuple(views["d2"].shape) == (19, h // 2, w // 2)
    # half the float32 arena's stage bytes and a little (the channel padding, h(x), the packed weights)
    assert need(1080, 1920) < 0.9 * built_lib.ibgs_hg_required_scratch(1080, 1920)
    for h, w in ((3, 8), (8, 3), (0, 8), (-1, 8), (8193, 8), (8, 8193), (1 << 40, 8)):
        assert need(h, w) == 0, (h, w)
    err = lambda: built_lib.ibgs_last_error()
    fwd = built_lib.ibgs_hgh_forward
    big = 1 << 30
    # (stream, H, W, x, 18 parameters, burned, residual, image_pred, scratch, bytes)
    good = [None, 8, 8, 128] + [128] * 18 + [1.0, 128, None, 128, big]
    for k, v in ((1, 3), (2, 3), (1, 0), (2, -5), (1, 8193), (2, 8193)):
        args = list(good)
        args[k] = v
        assert fwd(*args) < 0 and b"out of range" in err() and b"hgh_forward" in err(), (k, v)
    args = list(good)
    args[3] = None
    assert fwd(*args) < 0 and b"null input" in err()
    for i, (layer, _, _, _) in enumerate(hourglass.LAYERS):
        for j, what in enumerate((b"weight", b"bias")):
            args = list(good)
            args[4 + 2 * i + j] = None
            assert fwd(*args) < 0 and b"null parameters" in err() and layer.encode() in err() and what in err(), (layer, what)
    args = list(good)
    args[23] = None
    assert fwd(*args) < 0 and b"null outputs" in err()
    for k, v, msg in ((25, None, b"null scratch"), (25, 64, b"aligned"), (26, need(8, 8) - 1, b"needed")):
        args = list(good)
        args[k] = v
        assert fwd(*args) < 0 and msg in err(), k
    # the messages are those of ibgs_hg_forward but for the name
    for k, v in ((1, 3), (3, None), (4, None), (23, None), (25, None), (25, 64)):
        args = list(good)
        args[k] = v
        assert fwd(*args) < 0
        mine = err()
        assert built_lib.ibgs_hg_forward(*args) < 0
        assert mine.replace(b"hgh_forward", b"hg_forward") == err(), k


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------------
def test_precision_keyword_and_the_refusals(built_lib):
    net = hourglass.HourglassCNN()
    x = torch.rand(1, 38, 8, 9)
    with torch.no_grad():
        for t in (x, x[0], x.permute(0, 1, 3, 2)):
            with pytest.raises(RuntimeError, match="MI355X only"):          # a CPU tensor
                hourglass.hourglass_forward(t, net, precision="float16")
        with pytest.raises(RuntimeError, match="MI355X only"):
            net(x, render_scale=1.0, return_stages=True, precision="float16")
        with pytest.raises(ValueError, match="hidden_dim = 38 only"):          # 37 channels
            hourglass.hourglass_forward(torch.rand(1, 37, 8, 8), net, precision="float16")
        for shape in ((38, 3, 8), (1, 38, 8, 3)):          # side 3
            with pytest.raises(ValueError, match="out of range"):
                hourglass.hourglass_forward(torch.empty(shape), net, precision="float16")
        for bad in ("bfloat16", "half", torch.float16, None):
            with pytest.raises(ValueError, match=r'"float32" or "float16"'):
                hourglass.hourglass_forward(x, net, precision=bad)
            with pytest.raises(ValueError, match=r'"float32" or "float16"'):
                net(x, precision=bad)
    # grad mode
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\).*training keeps torch's CNN"):
        hourglass.hourglass_forward(x, net, precision="float16")
    # fuse_color
    full = hourglass.ColorAggregationNet()
    h, w = 6, 8
    pkg = dict(render=torch.rand(3, h, w), warped_image=torch.rand(9, h, w), cam_feat=torch.rand(12, h, w), camera_ray=torch.rand(3, h, w), min_depth_diff=torch.rand(1, h, w))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="MI355X only"):
            hourglass.fuse_color(pkg, full, precision="float16")
        with pytest.raises(RuntimeError, match="MI355X only"):
            full(pkg, precision="float16")
        with pytest.raises(ValueError, match=r'"float32" or "float16"'):
            hourglass.fuse_color(pkg, full, precision="bfloat16")
        with pytest.raises(ValueError, match=r'"float32" or "float16"'):
            full(pkg, precision="bfloat16")
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\).*training keeps torch's CNN"):
        hourglass.fuse_color(pkg, full, precision="float16")
    assert "float32 kernels" in hourglass.fuse_color.__doc__ and "closer to float64" in hourglass.fuse_color.__doc__
    assert "float16 views" in hourglass.hourglass_forward.__doc__
    # training is untouched: no precision keyword there
    import inspect
    for fn in (hourglass.hourglass_train, hourglass.hourglass_backward, hourglass.fuse_color_train):
        assert "precision" not in inspect.signature(fn).parameters
    for fn in (hourglass.hourglass_forward, hourglass.HourglassCNN.forward, hourglass.ColorAggregationNet.forward, hourglass.fuse_color):
        assert inspect.signature(fn).parameters["precision"].default == "float32"


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------------------
def test_rounding_helpers():
    assert href.h16(np.float32(1.0 + 2.0 ** -11)) == 1.0 and href.h16(np.float32(1.0 + 3 * 2.0 ** -11)) == 1.0 + 2.0 ** -9          # ties to even
    assert href.h16(np.float32(70000.0)) == np.inf and href.h16(np.float32(2.0 ** -25)) == 0.0 and href.h16(np.float32(2.0 ** -24)) == 2.0 ** -24
    assert href.ulp16(1.0) == 2.0 ** -10 and href.ulp16(0.999) == 2.0 ** -11 and href.ulp16(0.0) == 2.0 ** -24 and href.ulp16(-3.0) == 2.0 ** -9
    v = np.float16(0.3712)
    assert href.ulp16(float(v)) == float(np.spacing(v))


def test_autocast_composition_is_what_the_reference_runs():
    """tests/golden/hghalf.npz: the reference's own conv_decoder under CPU autocast float16, on the state dict and the two inputs of hourglass.npz.  Within one
    binary16 ulp per element: CPU blocking may move a tie."""
    z, g = np.load(os.path.join(GOLDEN, "hourglass.npz")), np.load(os.path.join(GOLDEN, "hghalf.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "hghalf.npz")) < 16 << 10 and sorted(g.files) == ["odd_residual", "residual"]
    p = _decoder_params(z)
    for key, tag, shape in (("cnn_input", "residual", (3, 16, 24)), ("odd_cnn_input", "odd_residual", (3, 13, 19))):
        assert g[tag].dtype == np.float16 and g[tag].shape == shape
        mine = href.autocast_composition(z[key], p)
        assert mine["residual"].dtype == torch.float16 and all(mine[k].dtype == torch.float16 for k in ref.STAGES)
        got, want = mine["residual"].double().numpy(), g[tag].astype(np.float64)
        off = np.abs(got - want) / href.ulp16(want)
        print("%s: %d of %d elements differ from the recorded run, at most %.1f ulp16" % (tag, int((off > 0).sum()), off.size, off.max()))
        assert off.max() <= 1.0
        # the recorded float32 run of the same network is the same function: half precision sits within its d_ref of it
        f32 = z["residual"].T.reshape(3, 16, 24) if tag == "residual" else z["odd_residual"][0]
        assert 0 < np.abs(want - f32).max() < 1e-3


def test_autocast_composition_against_the_arbiter():
    """d_ref of each stage on the fixture inputs (DESIGN.md section 15 quotes the printed figures): binary16 has 11 significant bits, the stages are 0.1 - 1,
    so a stage sits a few 2^-12 ~ 2.4e-4 from float64 and never as much as 2^-8."""
    z = np.load(os.path.join(GOLDEN, "hourglass.npz"))
    p = _decoder_params(z)
    for key in ("cnn_input", "odd_cnn_input"):
        want, d = href.d_ref(z[key], p)
        for k in href.CHECKED:
            print("%s %-8s d_ref %.3e   max |f64| %.3f" % (key, k, d[k], np.abs(want[k]).max()))
            assert 2.0 ** -16 < d[k] < 2.0 ** -8 * max(1.0, np.abs(want[k]).max()), (key, k, d[k])
    # one layer in float64 on rounded operands is what torch's half convolution rounds: within half an ulp16 and the float32 accumulation
    x = z["odd_cnn_input"][0]
    auto = href.autocast_composition(x, p)
    one = href.layer_f64(x, p["enc1_w"], p["enc1_b"])
    got = auto["e1"].double().numpy()
    assert np.all(np.abs(got - one) <= 0.5 * href.ulp16(one) + 2.0 ** -20)
    chain = href.layer_chain(x, p["enc1_w"], p["enc1_b"])
    assert chain.dtype == np.float32 and 0 < np.abs(chain - one).max() < 2.0 ** -20
