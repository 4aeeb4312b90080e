"""The hourglass unit on a CPU-only box: the C ABI (include/ibgs_hourglass.h <-> _lib.HG_EXPORTS <-> the built library), the build registration, the entry
point's validation with null pointers and bad sizes (validation precedes every HIP call), the arena's documented layout, the argument checks of
ibgs_amd.hourglass (which run before any GPU work), both key spellings and the whole-checkpoint load, the integer `up` rule against torch's float rule, and
the float64 restatement (tests/hourglass_ref.py) against the torch composition at float64 and against the two recorded runs of the reference's own network
(tests/golden/hourglass.npz)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ibgs_amd import _build, _lib, coloragg, hourglass
from tests import hourglass_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "hourglass.hip")
NET_H = os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "hg_net.h")          # the network as hourglass.hip, hgtrain.hip and hghalf.hip share it
TILE_H = os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "conv_tile.h")       # the 16 x 16 tile as hourglass.hip, hgtrain.hip and lpips.hip share it
GOLDEN = os.path.join(ROOT, "tests", "golden", "hourglass.npz")


def _state_dict(z):
    return {k[3:]: torch.tensor(z[k]) for k in z.files if k.startswith("sd/")}


def _decoder_params(z):
    return {name + s: z["sd/conv_decoder.%s.%s" % (theirs, t)] for name, theirs in ref.REFERENCE_NAMES.items() for s, t in (("_w", "weight"), ("_b", "bias"))}


# ---- the ABI and the build ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_hourglass.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(["ibgs_hg_required_scratch", "ibgs_hg_forward"])
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.HG_EXPORTS) == names
    assert re.search(r"ibgs_hg_forward\(void\* stream,", text)
    # the nine pairs, named as the layers, in the order of hourglass.LAYERS
    args = re.search(r"ibgs_hg_forward\((.*?)\);", text, re.S).group(1)
    assert re.findall(r"const float\* (\w+)_w,\s*const float\* (\w+)_b", args) == [(n, n) for n, _, _, _ in hourglass.LAYERS]
    defines = dict(re.findall(r"#define\s+IBGS_(HG_[A-Z_]+)\s+(\d+)", text))
    assert defines == {"HG_CHANNELS": "38", "HG_MIN_SIDE": "4", "HG_MAX_SIDE": "8192"}
    for name, val in defines.items():
        assert getattr(_lib, name) == int(val), name
    # the other export lists are untouched
    assert len(_lib.CAGG_EXPORTS) == 4 and len(_lib.SSIM_EXPORTS) == 4 and len(_lib.DTU_EXPORTS) == 8 and len(_lib.PCREG_EXPORTS) == 8 and len(_lib.GEOLOSS_EXPORTS) == 6
    others = (_lib.EXPORTS + _lib.SSIM_EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS + _lib.GEOLOSS_EXPORTS
              + _lib.CAGG_EXPORTS)
    assert not any("_hg_" in n for n in others)


def test_kernels_attributed_to_the_hourglass_unit():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["hg_conv3_kernel"]          # ONE templated kernel
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "hourglass"]
    for k in kernels:
        assert _build.tu_of(k) == "hourglass", k
        assert not any(sub in k for sub in others), k
    assert _build.KERNEL_TU[-1] == ("hg_", "hourglass") and _build.KERNEL_TU[0] == ("meval_", "mesh_eval")
    assert _build.SOURCES[-1] == "hourglass" and "hourglass" in _build.UNIT_HEADERS and "hourglass" in _build.tu_shas()
    assert "hourglass" not in _build.EXTRA          # a tolerance contract: no contraction flag
    assert _build.compile_flags("hourglass") == _build.compile_flags("coloragg")
    # the kernels of the other units still go where they went
    for k, tu in (("dtu_scan_kernel", "dtu"), ("meval_cell_count", "mesh_eval"), ("l1_rescale_kernel", "loss"), ("mesh_emit", "mesh"), ("scan_kernel", "scan_sort"),
                  ("ssim_fwd_kernel", "ssim"), ("geoloss_photo_fwd_kernel", "geoloss"), ("depth_normal_kernel", "depth_normal"), ("cagg_fwd_kernel", "coloragg"),
                  ("cagg_scan_l1_kernel", "coloragg"), ("knn_kernel", "knn"), ("adam_step_kernel", "adam"), ("compact_apply_kernel", "compact"), ("cell_count_kernel", "binning"),
                  ("expand_kernel", "binning")):
        assert _build.tu_of(k) == tu, k
    code = _build._code_only(src)
    assert "atomic" not in code.lower()          # nothing crosses a workgroup
    # the constants the GPU tests size their frames by; the grid is two-dimensional and uncapped
    # (they are the shared tile's, and this unit launches by them)
    tile = _build._code_only(open(TILE_H).read())
    assert re.search(r"constexpr int CT_TILE = 16;", tile) and re.search(r"constexpr int CT_THREADS = 256;", tile)
    assert not re.search(r"constexpr int \w*(TILE|THREADS) =", code) and re.search(r"__launch_bounds__\(CT_THREADS, 2\) hg_conv3_kernel", code)
    assert re.search(r"const dim3 grid\(\(unsigned\)\(\(a\.w \+ CT_TILE - 1\) / CT_TILE\), \(unsigned\)\(\(a\.h \+ CT_TILE - 1\) / CT_TILE\)\);", code)
    assert re.search(r"hipLaunchKernelGGL\(\(hg_conv3_kernel<CA, CB, COUT, MODE, FUSE>\), grid, dim3\(CT_THREADS\), 0, st, a\);", code)
    assert len(re.findall(r"hg_launch<", code)) == 7          # seven launches
    assert re.findall(r"__builtin_amdgcn_mfma_\w+", tile) == ["__builtin_amdgcn_mfma_f32_16x16x4f32"] and "ct_mfma(" in code and "__builtin_amdgcn_mfma" not in code
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc")) if "hourglass" in f and not f.startswith("_")) == ["hourglass.hip"]
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "shared/hg_net.h", "shared/conv_tile.h", "../../include/ibgs_hourglass.h"]
    assert [os.path.basename(h) for h in _build.UNIT_HEADERS["hourglass"]] == ["ibgs_hourglass.h", "hg_net.h", "conv_tile.h"]
    shared = _build._code_only(open(NET_H).read())
    assert re.search(r"enum \{ CT_PLAIN = 0, CT_POOL = 1, CT_UP = 2 \};", tile) and re.search(r"constexpr int HG_C = IBGS_HG_CHANNELS;", shared)
    assert not re.search(r"_PLAIN = 0", shared)
    for unit in ("hourglass", "hgtrain", "hghalf"):          # ... and nobody keeps a copy of what the header holds
        code = _build._code_only(open(os.path.join(ROOT, "ibgs_amd", "csrc", unit + ".hip")).read())
        assert not re.search(r"_PLAIN = 0|_shape_ok\(const char|names\[9\]|_blend\(float", code), unit


def test_layer_table_of_the_shared_header_is_LAYERS():
    """(name, Cout, Ca, Cb, kernel side, level of the output) in csrc/shared/hg_net.h against hourglass.LAYERS and, for the six layers whose output is kept,
    hourglass.STAGES."""
    code = _build._code_only(open(NET_H).read())
    table = re.search(r"HG_LAYERS\[HG_LAYER_COUNT\] = \{(.*?)\};", code, re.S).group(1)
    rows = [(n,) + tuple(int(v) for v in rest.split(",")) for n, rest in re.findall(r'\{"(\w+)",([\d,\s]+)\}', table)]
    assert [(n, cout, ca + cb, side) for n, cout, ca, cb, side, _ in rows] == list(hourglass.LAYERS)
    assert [(cout, level) for _, cout, _, _, _, level in rows[:len(hourglass.STAGES)]] == [(ch, level) for _, ch, level in hourglass.STAGES]
    assert all(level == 0 for *_, level in rows[len(hourglass.STAGES):]) and re.search(r"constexpr int HG_STAGE_COUNT = %d;" % len(hourglass.STAGES), code)
    ids = re.search(r"enum \{ (HG_ENC1,.*?), HG_LAYER_COUNT \};", code).group(1).split(", ")
    assert [i[3:].lower() for i in ids] == [n for n, _, _, _ in hourglass.LAYERS]
    # a concatenation's halves are its two inputs' channels: dec2 reads [u2, e2], dec1 [u1, e1], fuse_input [d1, x]
    assert [(n, ca, cb) for n, _, ca, cb, _, _ in rows if cb] == [("dec2", 19, 19), ("dec1", 38, 38), ("fuse_input", 38, 38)]


def _layout(h, w, half=False):
    """The documented arenas (include/ibgs_hourglass.h; half: include/ibgs_hg_half.h) from hourglass.STAGES: the one statement of the layout the tests hold
    the library's sizes and hourglass._arena_views against.  -> (bytes, {entry: offset})"""
    assert hourglass.STAGES == (("e1", 38, 0), ("e2", 19, 1), ("b", 9, 2), ("u2", 19, 1), ("d2", 19, 1), ("u1", 38, 0))
    size, pad = (2, 8) if half else (4, 1)
    entries = [(name, (ch + pad - 1) // pad * pad * (h >> level) * (w >> level) * size) for name, ch, level in ((("xh", 38, 0),) if half else ()) + hourglass.STAGES]
    at, offs = 0, {}
    for name, n in entries + ([("packed", _lib.HGH_PACKED_WEIGHT_BYTES)] if half else []):
        offs[name] = at = (at + 127) // 128 * 128
        at += n
    return (at + 127) // 128 * 128, offs


@pytest.mark.parametrize("h,w", [(4, 4), (5, 7), (17, 67), (4, 8192), (8192, 8192)])
def test_one_layout_for_both_arenas_and_their_views(built_lib, h, w):
    """Odd sides: the H / 2 / 2 rounding; the extremes: size_t (the float32 arena of 8192 x 8192 is 2^34.7 bytes).  The views are taken of a meta tensor."""
    for half, need in ((False, built_lib.ibgs_hg_required_scratch), (True, built_lib.ibgs_hgh_required_scratch)):
        total, offs = _layout(h, w, half)
        assert need(h, w) == total and total % 128 == 0 and all(o % 128 == 0 for o in offs.values()), (h, w, half)
        views = hourglass._arena_views(torch.empty(total, dtype=torch.uint8, device="meta"), h, w, half)
        assert list(views) == [n for n, _, _ in hourglass.STAGES] == [n for n in offs if n not in ("xh", "packed")]
        for (n, ch, level), v in zip(hourglass.STAGES, views.values()):
            assert v.storage_offset() * v.element_size() == offs[n] and tuple(v.shape) == (ch, h >> level, w >> level), (h, w, half, n)
            assert v.dtype == (torch.float16 if half else torch.float32), (h, w, half, n)
    assert (8192 * 8192 * 38 * 4 > 1 << 33) and built_lib.ibgs_hg_required_scratch(8192, 8192) > 1 << 34


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_hg_required_scratch
    for h, w in ((4, 4), (5, 7), (16, 24), (17, 67), (1080, 1920), (8192, 8192), (4, 8192)):
        total, offs = _layout(h, w)
        assert need(h, w) == total and total % 128 == 0, (h, w)
        views = hourglass._arena_views(torch.empty(total, dtype=torch.uint8), h, w)
        base = views["e1"].untyped_storage().data_ptr()
        assert [n for n, _, _ in hourglass.STAGES] == list(offs) == list(views)
        for n in offs:
            assert views[n].data_ptr() - base == offs[n] and views[n].is_contiguous(), (h, w, n)
        assert tuple(views["b"].shape) == (9, h // 4, w // 4) and tuple(views["u1"].shape) == (38, h, w) and tuple(views["d2"].shape) == (19, h // 2, w // 2)
    assert need(1080, 1920) > 2 * 38 * 1080 * 1920 * 4
    for h, w in ((3, 8), (8, 3), (0, 8), (-1, 8), (8193, 8), (8, 8193), (1 << 40, 8)):
        assert need(h, w) == 0, (h, w)
    err = lambda: built_lib.ibgs_last_error()
    fwd = built_lib.ibgs_hg_forward
    big = 1 << 30
    # (stream, H, W, x, 18 parameters, burned, residual, image_pred, scratch, bytes)
    good = [None, 8, 8, 128] + [128] * 18 + [1.0, 128, None, 128, big]
    for k, v in ((1, 3), (2, 3), (1, 0), (2, -5), (1, 8193), (2, 8193)):
        args = list(good)
        args[k] = v
        assert fwd(*args) < 0 and b"out of range" in err(), (k, v)
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


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    name = "hourglass_forward"
    net = hourglass.HourglassCNN()
    x = torch.rand(1, 38, 8, 9)
    with torch.no_grad():
        for t in (x, x[0], x.permute(0, 1, 3, 2)):
            with pytest.raises(RuntimeError, match="MI355X only"):
                hourglass.hourglass_forward(t, net)
        with pytest.raises(RuntimeError, match="MI355X only"):
            net(x, render_scale=1.0, return_stages=True)
    with pytest.raises(ValueError, match="implies hidden_dim = 70"):
        hourglass.hourglass_forward(torch.rand(1, 70, 8, 8), net)
    with pytest.raises(ValueError, match="hidden_dim = 38 only"):
        hourglass.hourglass_forward(torch.rand(19, 8, 8), net)
    for shape in ((38, 3, 8), (1, 38, 8, 3), (38, 8193, 4)):
        with pytest.raises(ValueError, match="out of range"):
            hourglass.hourglass_forward(torch.empty(shape), net)
    for shape in ((2, 38, 8, 8), (38, 8), (1, 1, 38, 8, 8)):
        with pytest.raises(ValueError, match=name):
            hourglass.hourglass_forward(torch.empty(shape), net)
    with pytest.raises(TypeError, match="HourglassCNN"):
        hourglass.hourglass_forward(x, torch.nn.Conv2d(38, 3, 1))
    with pytest.raises(TypeError, match="cnn_input"):
        hourglass.hourglass_forward(x.numpy(), net)
    # wrong parameter shapes, each named
    for layer, cout, cin, k in hourglass.LAYERS:
        bad = hourglass.HourglassCNN()
        setattr(bad, layer + "_w", torch.nn.Parameter(torch.zeros(cout, cin + 1, k, k)))
        with pytest.raises(ValueError, match=layer + "_w must be"):
            hourglass.hourglass_forward(x, bad)
        bad = hourglass.HourglassCNN()
        setattr(bad, layer + "_b", torch.nn.Parameter(torch.zeros(cout + 1)))
        with pytest.raises(ValueError, match=layer + "_b must be"):
            hourglass.hourglass_forward(x, bad)
    # fuse_color
    full = hourglass.ColorAggregationNet()
    h, w = 6, 8
    pkg = dict(render=torch.rand(3, h, w), warped_image=torch.rand(9, h, w), cam_feat=torch.rand(12, h, w), camera_ray=torch.rand(3, h, w), min_depth_diff=torch.rand(1, h, w))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="MI355X only"):
            hourglass.fuse_color(pkg, full)
        with pytest.raises(RuntimeError, match="MI355X only"):
            full(pkg)
        with pytest.raises(TypeError, match="ColorAggregationNet"):
            hourglass.fuse_color(pkg, full.cnn)
        with pytest.raises(KeyError, match="cam_feat"):
            hourglass.fuse_color({k: v for k, v in pkg.items() if k != "cam_feat"}, full)
        with pytest.raises(ValueError, match="out of range"):
            hourglass.fuse_color(dict(pkg, render=torch.rand(3, 3, w)), full)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\).*training keeps torch's CNN"):
        hourglass.fuse_color(pkg, full)          # the parameters require grad and grad mode is on
    with pytest.raises(ValueError, match="mode"):
        hourglass.ColorAggregationNet("median")
    src = open(os.path.join(ROOT, "ibgs_amd", "hourglass.py")).read()
    assert not re.search(r"^(import|from)\s+(oracle|tests)\b", src, re.M)
    assert "valid until" in hourglass.hourglass_forward.__doc__ and "not trimmed" in hourglass.fuse_color.__doc__.lower()


def test_grad_mode_is_refused():
    net = hourglass.HourglassCNN()
    x = torch.rand(1, 38, 8, 8)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\).*training keeps torch's CNN"):
        hourglass.hourglass_forward(x, net)          # the parameters require grad
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):
        hourglass.hourglass_forward(x.clone().requires_grad_(True), net)
    with pytest.raises(RuntimeError, match="MI355X only"):          # nothing requires grad: the call gets as far as the device check
        hourglass.hourglass_forward(x, net)


def test_both_key_spellings_and_the_whole_checkpoint():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 512 << 10
    sd = _state_dict(z)
    assert len(sd) == 22 and sorted(k.split(".")[0] for k in sd) == ["conv_decoder"] * 18 + ["per_view_mlp"] * 4
    theirs = {k[len("conv_decoder."):]: v for k, v in sd.items() if k.startswith("conv_decoder.")}
    assert sorted(theirs) == sorted(hourglass.REFERENCE_KEYS)
    a, b = hourglass.HourglassCNN(), hourglass.HourglassCNN()
    assert sorted(a.state_dict()) == sorted(n + s for n, _, _, _ in hourglass.LAYERS for s in ("_w", "_b")) and len(list(a.parameters())) == 18
    for layer, cout, cin, k in hourglass.LAYERS:          # nn.Conv2d's default initialisation: within 1 / sqrt(fan_in), and not degenerate
        wt, bt = getattr(a, layer + "_w").detach(), getattr(a, layer + "_b").detach()
        bound = 1.0 / (cin * k * k) ** 0.5
        assert tuple(wt.shape) == (cout, cin, k, k) and tuple(bt.shape) == (cout,) and getattr(a, layer + "_w").requires_grad
        assert 0.8 * bound < float(wt.abs().max()) <= bound and float(bt.abs().max()) <= bound and float(wt.std()) > 0.4 * bound
    assert not torch.equal(a.dec1_w.detach(), theirs["dec1.0.weight"])
    a.load_state_dict(theirs)
    b.load_state_dict(a.state_dict())
    for m in (a, b):
        for their_key, mine in hourglass.REFERENCE_KEYS.items():
            assert torch.equal(getattr(m, mine).detach(), theirs[their_key]), mine
    assert sorted(theirs) == sorted(hourglass.REFERENCE_KEYS)          # the caller's dictionary is left as it was
    with pytest.raises(RuntimeError):
        hourglass.HourglassCNN().load_state_dict({k: v for k, v in theirs.items() if k != "final.bias"})
    with pytest.raises(ValueError, match="both"):
        hourglass.HourglassCNN().load_state_dict(dict(theirs, enc1_w=theirs["enc1.0.weight"]))
    # the whole checkpoint of the reference, unchanged
    net = hourglass.ColorAggregationNet()
    assert isinstance(net.front_end, coloragg.PerViewFrontEnd) and isinstance(net.cnn, hourglass.HourglassCNN)
    net.load_state_dict(sd)
    assert len(sd) == 22 and all(k.startswith(("conv_decoder.", "per_view_mlp.")) for k in sd)
    assert torch.equal(net.front_end.w2.detach(), sd["per_view_mlp.2.weight"]) and torch.equal(net.front_end.b1.detach(), sd["per_view_mlp.0.bias"])
    for their_key, mine in hourglass.REFERENCE_KEYS.items():
        assert torch.equal(getattr(net.cnn, mine).detach(), sd["conv_decoder." + their_key]), mine
    other = hourglass.ColorAggregationNet("max")
    other.load_state_dict(net.state_dict())          # ... and this module's own keys
    assert torch.equal(other.cnn.final_w.detach(), sd["conv_decoder.final.weight"]) and sorted(net.state_dict())[0].startswith("cnn.")
    with pytest.raises(RuntimeError):
        hourglass.ColorAggregationNet().load_state_dict({k: v for k, v in sd.items() if k != "conv_decoder.enc3.0.bias"})


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def test_integer_up_rule_is_torchs_float_rule():
    """out[y] = in[min(y hin div h, hin - 1)] against F.interpolate(mode="nearest") on an index ramp, for every output size 2 .. MAX_SIDE with hin = h div 2."""
    for n_out in range(2, _lib.HG_MAX_SIDE + 1):
        n_in = n_out // 2
        ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
        theirs = F.interpolate(ramp, size=(n_out, 1), mode="nearest").view(-1).long().numpy()
        assert np.array_equal(theirs, ref.up_index(n_out, n_in)), n_out
    t = np.arange(2 * 3 * 5, dtype=np.float64).reshape(2, 3, 5)
    assert np.array_equal(ref.up_ref(t, 7, 11), F.interpolate(torch.tensor(t)[None], size=(7, 11), mode="nearest")[0].numpy())
    assert np.array_equal(ref.pool_ref(t), F.max_pool2d(torch.tensor(t)[None], 2)[0].numpy()) and ref.pool_ref(t).shape == (2, 1, 2)


@pytest.mark.parametrize("h,w,seed,shift", [(4, 4, 0, 0.0), (5, 7, 1, 0.0), (16, 24, 2, -0.05), (17, 35, 3, 0.0)])
def test_restatement_against_the_torch_composition_at_float64(h, w, seed, shift):
    p = ref.seeded_params(seed, shift)
    x = ref.seeded_input(seed, h, w, signed=bool(seed & 1))
    mine, theirs = ref.forward_ref(x, p, 0.75), ref.torch_composition(x, p, torch.float64)
    assert sorted(theirs) == sorted(k for k in mine if k != "image_pred")
    for k, v in theirs.items():
        assert mine[k].dtype == np.float64 and mine[k].shape == tuple(v.shape) and np.abs(mine[k] - v.numpy()).max() <= 1e-12, k
    assert mine["b"].shape == (9, h // 4, w // 4) and mine["e2"].shape == (19, h // 2, w // 2) and mine["residual"].shape == (3, h, w)
    assert np.array_equal(mine["image_pred"], 0.75 * x[0, 35:].astype(np.float64) + mine["residual"])
    # the float32 chain is an evaluation of the same network: within float32 rounding of it, and not identical to torch's
    chain = ref.chain_f32(x, p)
    for k in ("e1", "b", "residual"):
        assert chain[k].dtype == np.float32 and 0 < np.abs(chain[k] - mine[k]).max() <= 2.0 ** -20 * max(1.0, np.abs(mine[k]).max()), k


def test_restatement_reproduces_the_reference_runs():
    """The recorded runs are float32; a float32 evaluation sits 2^-23 .. 2^-22.5 of the output's magnitude from float64 with default-initialised weights.  The
    bar, 2^-20 of the largest recorded magnitude, is about six times that."""
    z = np.load(GOLDEN)
    p = _decoder_params(z)
    assert z["cnn_input"].shape == (1, 38, 16, 24) and z["residual"].shape == (16 * 24, 3) and z["odd_cnn_input"].shape == (1, 38, 13, 19)
    cagg = np.load(os.path.join(ROOT, "tests", "golden", "coloragg.npz"))
    assert np.array_equal(z["window"], cagg["window"]) and np.array_equal(z["cnn_input"][0, 32:], cagg["mean_cnn_input"][0, 32:])          # the same window: ray and colour
    x2 = z["odd_cnn_input"][0]
    assert x2[:32].min() >= 0 and np.abs(np.linalg.norm(x2[32:35], axis=0) - 1).max() < 1e-6 and 0 <= x2[35:].min() and x2[35:].max() <= 1
    s = ref.forward_ref(z["cnn_input"], p)
    want = z["residual"].T.reshape(3, 16, 24)
    assert np.abs(s["residual"] - want).max() <= 2.0 ** -20 * np.abs(want).max()
    assert np.abs(s["image_pred"] - z["image_pred"]).max() <= 2.0 ** -20 * np.abs(z["image_pred"]).max()
    s = ref.forward_ref(z["odd_cnn_input"], p)
    want = z["odd_residual"][0]
    assert np.abs(s["residual"] - want).max() <= 2.0 ** -20 * np.abs(want).max()
