"""The colour aggregation unit on a CPU-only box: the C ABI (include/ibgs_color_agg.h <-> _lib.CAGG_EXPORTS <-> the built library), the build
registration, the entry points' validation with null pointers and bad sizes, the argument checks of ibgs_amd.coloragg (which run before any GPU work),
PerViewFrontEnd's two key spellings, and the float64 restatement (tests/coloragg_ref.py) against the recorded run of the reference's own network
(tests/golden/coloragg.npz), against tests/scenes.fuse_color_inputs on consumer.npz, and against torch autograd of the float64 composition."""
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, coloragg
from tests import coloragg_ref as ref
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "coloragg.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- the ABI and the build ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_color_agg.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(["ibgs_cagg_required_scratch", "ibgs_cagg_levels", "ibgs_cagg_forward", "ibgs_cagg_backward"])
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.CAGG_EXPORTS) == names
    for n in ("levels", "forward", "backward"):          # the stream first, like the other unit headers
        assert re.search(r"ibgs_cagg_%s\(void\* stream," % n, text), n
    defines = dict(re.findall(r"#define\s+IBGS_(CAGG_[A-Z_]+)\s+(\d+)", text))
    assert sorted(defines) == ["CAGG_FEATURES", "CAGG_MAX", "CAGG_MAX_SIDE", "CAGG_MAX_SRC", "CAGG_MEAN"]
    for name, val in defines.items():
        assert getattr(_lib, name) == int(val), name
    assert _lib.CAGG_MAX_SRC == 5 == _lib.MAX_SRC
    # the other export lists are untouched
    assert len(_lib.SSIM_EXPORTS) == 4 and len(_lib.DTU_EXPORTS) == 8 and len(_lib.PCREG_EXPORTS) == 8 and len(_lib.GEOLOSS_EXPORTS) == 6
    others = _lib.EXPORTS + _lib.SSIM_EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS + _lib.GEOLOSS_EXPORTS
    assert not any("cagg" in n for n in others)


def test_kernels_attributed_to_the_coloragg_unit():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["cagg_bwd_kernel", "cagg_final_kernel", "cagg_fwd_kernel", "cagg_levels_kernel"]
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "coloragg"]
    for k in kernels:
        assert _build.tu_of(k) == "coloragg", k
        assert not any(sub in k for sub in others), k          # whatever the order of the table
    at = _build.KERNEL_TU.index(("geoloss_", "geoloss"))
    assert _build.KERNEL_TU[at + 1] == ("cagg_", "coloragg") and _build.KERNEL_TU[0] == ("meval_", "mesh_eval")
    assert "coloragg" in _build.SOURCES and "coloragg" in _build.UNIT_HEADERS and "coloragg" in _build.tu_shas()
    assert "coloragg" not in _build.EXTRA          # a tolerance contract: no contraction flag
    assert _build.compile_flags("coloragg") == _build.compile_flags("ssim")
    # the kernels of the other units still go where they went (a cagg_* name is matched before any later substring)
    for k, tu in (("dtu_scan_kernel", "dtu"), ("meval_cell_count", "mesh_eval"), ("l1_rescale_kernel", "loss"), ("mesh_emit", "mesh"), ("scan_kernel", "scan_sort"),
                  ("ssim_fwd_kernel", "ssim"), ("geoloss_photo_fwd_kernel", "geoloss"), ("depth_normal_kernel", "depth_normal"), ("cagg_scan_l1_kernel", "coloragg")):
        assert _build.tu_of(k) == tu, k
    code = _build._code_only(src)
    # the only atomics: the level count's two integer words; the float sums are per-workgroup partials and a fixed-order final pass
    assert sorted(set(re.findall(r"\b(\w*atomic\w*)\s*\(", code))) == ["__hip_atomic_fetch_add", "__hip_atomic_fetch_or", "__hip_atomic_load"]
    assert len(re.findall(r"atomic", code)) == 3
    # the backward's geometry is stated in the header it shares with rsztrain.hip; the forward's stays here (tests/test_gpu_coloragg.py sizes its frames by both)
    bwd = _build._code_only(open(os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "pv_mlp_bwd.h")).read())
    assert re.search(r"constexpr int PVB_MAX_GROUPS = 512;", bwd) and re.search(r"constexpr int CAGG_FWD_MAX_GROUPS = 4096;", code)
    assert re.search(r"constexpr int PVB_CHUNK = PVB_WAVES \* PVB_B;", bwd) and re.search(r"constexpr int PVB_T = 256;", bwd) and re.search(r"constexpr int PVB_B = 32;", bwd)
    assert re.search(r"constexpr int PVB_WAVES = PVB_T / 64;", bwd) and re.search(r"const size_t chunks = \(pixels \+ PVB_CHUNK - 1\) / PVB_CHUNK;", bwd)
    assert re.search(r"constexpr int CHUNK = CWAVES \* CB;", code) and re.search(r"constexpr int CT = 256;", code) and re.search(r"constexpr int CB = 32;", code)
    assert not re.search(r"constexpr int (CAGG_MAX_GROUPS|CAGG_PARTIAL|CROW|FIN_ELEMS)\b", code)          # stated once
    # no header of its own under csrc/ (every header there is hashed into every unit's profile stamp): the chain it shares with resample.hip lies a directory below
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc")) if "coloragg" in f and not f.startswith("_")) == ["coloragg.hip"]
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "shared/pv_mlp_bwd.h", "../../include/ibgs_color_agg.h"]          # (pv_mlp_bwd.h includes pv_mlp.h)
    assert re.findall(r'#include "([^"]+)"', open(os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "pv_mlp_bwd.h")).read()) == ["pv_mlp.h"]
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc")) if f.endswith(".h")) == ["adam_math.h", "blend.h", "block_ops.h", "common.h", "sh_color.h", "wave_bits.h", "wave_reduce.h"]
    assert sorted(os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc", "shared"))) == ["conv_tile.h", "conv_tile_f16.h", "hg_net.h", "pv_mlp.h", "pv_mlp_bwd.h", "rsz_taps.h", "ssim_window.h"]
    for unit, headers in (("coloragg", ["pv_mlp.h", "pv_mlp_bwd.h"]), ("resample", ["pv_mlp.h", "rsz_taps.h"]), ("ssim", ["ssim_window.h"]), ("geoloss", ["ssim_window.h"])):
        assert [os.path.basename(h) for h in _build.UNIT_HEADERS[unit]][1:] == headers, unit
    assert sum(any("shared" in h for h in hs) for hs in _build.UNIT_HEADERS.values()) == 10          # no other unit's stamp holds them (rsztrain is the eighth, lpips with conv_tile.h the ninth, hghtrain the tenth)


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_cagg_required_scratch
    small, hd, huge = need(3, 16, 24), need(3, 1080, 1920), need(5, 65536, 65536)
    assert 0 < small < hd == huge == need(1, 4000, 6000), "the arena is bounded by the backward's grid, not by the frame"
    assert hd < 8 << 20 and small % 128 == 0          # 512 workgroups x 1312 f64 sums
    assert need(0, 8, 8) == 0 and need(6, 8, 8) == 0 and need(1, 0, 8) == 0 and need(1, 8, 0) == 0 and need(-1, 8, 8) == 0 and need(1, 65537, 8) == 0
    err = lambda: built_lib.ibgs_last_error()
    lev, fwd, bwd = built_lib.ibgs_cagg_levels, built_lib.ibgs_cagg_forward, built_lib.ibgs_cagg_backward
    big = 8 << 20
    # levels: (stream, S, H, W, warped, nb, levels_out, scratch, bytes)
    for s, h, w in ((0, 8, 8), (6, 8, 8), (3, 0, 8), (3, 8, 65537), (-1, 8, 8)):
        assert lev(None, s, h, w, 128, 3, 128, 128, big) < 0 and b"out of range" in err()
    assert lev(None, 3, 8, 8, 128, 0, 128, 128, big) < 0 and b"nb_visible_src_frames" in err()
    assert lev(None, 3, 8, 8, None, 3, 128, 128, big) < 0 and b"null image" in err()
    assert lev(None, 3, 8, 8, 128, 3, None, 128, big) < 0 and b"null outputs" in err()
    assert lev(None, 3, 8, 8, 128, 3, 128, None, big) < 0 and b"null scratch" in err()
    assert lev(None, 3, 8, 8, 128, 3, 128, 64, big) < 0 and b"aligned" in err()
    assert lev(None, 3, 8, 8, 128, 3, 128, 128, 16) < 0 and b"needed" in err()
    # forward: (stream, S, H, W, mode, render, warped, feat, ray, w1, b1, w2, b2, levels, out)
    good = [None, 3, 8, 8, 0] + [128] * 10
    for k, v in ((1, 0), (1, 6), (2, 0), (3, 65537)):
        args = list(good)
        args[k] = v
        assert fwd(*args) < 0 and b"out of range" in err(), (k, v)
    for v in (2, -1):
        args = list(good)
        args[4] = v
        assert fwd(*args) < 0 and b"mode" in err()
    for ks, msg in (((5, 6, 7, 8), b"null image"), ((9, 10, 11, 12), b"null parameters"), ((13,), b"null levels"), ((14,), b"null outputs")):
        for k in ks:
            args = list(good)
            args[k] = None
            assert fwd(*args) < 0 and msg in err(), k
    # backward: (stream, S, H, W, mode, render, warped, feat, w1, b1, w2, b2, levels, grad_out, 6 gradients, scratch, bytes)
    good = [None, 3, 8, 8, 1] + [128] * 9 + [128] * 6 + [128, big]
    for k, v in ((1, 0), (1, 6), (2, 0), (3, 65537)):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and b"out of range" in err(), (k, v)
    args = list(good)
    args[4] = 7
    assert bwd(*args) < 0 and b"mode" in err()
    for ks, msg in (((5, 6, 7), b"null image"), ((8, 9, 10, 11), b"null parameters"), ((12,), b"null levels"), ((13,), b"null grad_out")):
        for k in ks:
            args = list(good)
            args[k] = None
            assert bwd(*args) < 0 and msg in err(), k
    args = list(good)
    args[14:20] = [None] * 6
    assert bwd(*args) < 0 and b"null outputs" in err()
    for k, v, msg in ((20, None, b"null scratch"), (20, 64, b"aligned"), (21, 16, b"needed")):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and msg in err(), k


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------------
def _cpu_args(s=3, h=6, w=8, flat=True):
    g = torch.Generator().manual_seed(1)
    r = lambda *shape: torch.rand(*shape, generator=g)
    warped, feat = (r(3 * s, h, w), r(4 * s, h, w)) if flat else (r(s, 3, h, w), r(s, 4, h, w))
    return [r(3, h, w), warped, feat, r(3, h, w), r(32, 7), r(32), r(32, 32), r(32)]


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    name = "per_view_features"
    for s in (1, 3, 5):
        for flat in (True, False):
            with pytest.raises(RuntimeError, match="MI355X only"):
                coloragg.per_view_features(*_cpu_args(s, flat=flat))
    h, w = 6, 8
    ok = _cpu_args()
    def bad(k, t, match=name):
        args = list(ok)
        args[k] = t
        with pytest.raises(ValueError, match=match):
            coloragg.per_view_features(*args)
    bad(0, torch.rand(1, h, w), "render")
    bad(0, torch.rand(3, h + 1, w))
    bad(0, torch.rand(3, 0, w), "empty")
    bad(3, torch.rand(3, h, w + 1), "camera_ray")
    bad(1, torch.rand(10, h, w), "warped_image")
    bad(1, torch.rand(18, h, w), "warped_image holds 6 sources")
    bad(1, torch.rand(0, 3, h, w), "warped_image holds 0 sources")
    bad(1, torch.rand(6, h, w), "warped_image holds 2 sources, cam_feat 3")
    bad(1, torch.rand(9, h, w + 1), "warped_image")
    bad(2, torch.rand(3, 3, h, w), "cam_feat")
    bad(2, torch.rand(13, h, w), "cam_feat")
    bad(4, torch.rand(32, 8), "w1")
    bad(5, torch.rand(31), "b1")
    bad(6, torch.rand(32, 31), "w2")
    bad(7, torch.rand(1, 32), "b2")
    # any other feature width is refused with a message that names it
    wide = list(ok)
    wide[4:] = [torch.rand(64, 7), torch.rand(64), torch.rand(64, 64), torch.rand(64)]
    with pytest.raises(ValueError, match="feature width of 64"):
        coloragg.per_view_features(*wide)
    for kw, match in ((dict(nb_visible_src_frames=0), "nb_visible_src_frames"), (dict(nb_visible_src_frames=1.5), "nb_visible_src_frames"), (dict(mode="sum"), "mode"),
                      (dict(levels=-1), "levels"), (dict(levels=2.5), "levels"), (dict(levels=torch.zeros(1, dtype=torch.int32)), "levels"),
                      (dict(levels=torch.zeros((), dtype=torch.int64)), "levels")):
        with pytest.raises(ValueError, match=match):
            coloragg.per_view_features(*ok, **kw)
    with pytest.raises(TypeError, match="render"):
        coloragg.per_view_features(ok[0].numpy(), *ok[1:])
    with pytest.raises(TypeError, match="w2"):
        coloragg.per_view_features(*ok[:6], ok[6].numpy(), ok[7])
    front = coloragg.PerViewFrontEnd()
    pkg = dict(render=ok[0], warped_image=ok[1], cam_feat=ok[2], camera_ray=ok[3], min_depth_diff=torch.rand(1, h, w))
    with pytest.raises(RuntimeError, match="MI355X only"):
        coloragg.fuse_color_inputs(pkg, front)
    with pytest.raises(TypeError, match="front_end"):
        coloragg.fuse_color_inputs(pkg, torch.nn.Linear(7, 32))
    with pytest.raises(KeyError, match="min_depth_diff"):
        coloragg.fuse_color_inputs({k: v for k, v in pkg.items() if k != "min_depth_diff"}, front)
    with pytest.raises(ValueError, match="mode"):
        coloragg.PerViewFrontEnd("median")
    src = open(os.path.join(ROOT, "ibgs_amd", "coloragg.py")).read()
    assert not re.search(r"^(import|from)\s+(oracle|tests)\b", src, re.M)
    assert "no gradient" in coloragg.per_view_features.__doc__.lower() or "NO gradient" in coloragg.per_view_features.__doc__


def test_front_end_loads_both_key_spellings():
    z = np.load(os.path.join(GOLDEN, "coloragg.npz"))
    theirs = {"per_view_mlp.0.weight": torch.tensor(z["w1"]), "per_view_mlp.0.bias": torch.tensor(z["b1"]), "per_view_mlp.2.weight": torch.tensor(z["w2"]),
              "per_view_mlp.2.bias": torch.tensor(z["b2"])}
    a, b = coloragg.PerViewFrontEnd(), coloragg.PerViewFrontEnd("max")
    assert sorted(a.state_dict()) == ["b1", "b2", "w1", "w2"] and [tuple(p.shape) for p in (a.w1, a.b1, a.w2, a.b2)] == [(32, 7), (32,), (32, 32), (32,)]
    assert not torch.equal(a.w1, torch.tensor(z["w1"]))
    a.load_state_dict(theirs)
    b.load_state_dict(a.state_dict())
    for m in (a, b):
        for n in ("w1", "b1", "w2", "b2"):
            assert torch.equal(getattr(m, n).detach(), torch.tensor(z[n])), n
    assert sorted(theirs) == sorted(coloragg.REFERENCE_KEYS)          # the caller's dictionary is left as it was
    # nested in a larger module: the prefix is honoured
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.front = coloragg.PerViewFrontEnd()
    net = Net()
    net.load_state_dict({"front." + k: v for k, v in theirs.items()})
    assert torch.equal(net.front.w2.detach(), torch.tensor(z["w2"]))
    with pytest.raises(RuntimeError):
        coloragg.PerViewFrontEnd().load_state_dict({k: v for k, v in theirs.items() if not k.endswith("2.bias")})
    with pytest.raises(ValueError, match="both"):
        coloragg.PerViewFrontEnd().load_state_dict(dict(theirs, w1=torch.tensor(z["w1"])))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def _fixture_inputs(z):
    return z["in_color"], z["in_warped_image"], z["in_cam_feat"], z["in_camera_ray"], z["w1"], z["b1"], z["w2"], z["b2"]


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_restatement_reproduces_the_reference_run(mode):
    """The recorded tensors are float32 results of sums of up to 16 x 24 x 3 terms: 2^-20 of the largest magnitude is some sixteen roundings of it."""
    z = np.load(os.path.join(GOLDEN, "coloragg.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "coloragg.npz")) <= os.path.getsize(os.path.join(GOLDEN, "consumer.npz"))
    assert tuple(z["window"][2:]) == (16, 24) and all(n > 0 for n in z["pixels_per_level"][:3]) and not any(z["pixels_per_level"][3:])
    out, cache = ref.forward_ref(*_fixture_inputs(z), 3, mode)
    assert cache["levels"] == 3 and out.shape == (1, 38, 16, 24) and out.dtype == np.float64
    want = z[mode + "_cnn_input"]
    assert np.abs(out - want).max() <= 2.0 ** -20 * np.abs(want).max()
    g = ref.backward_ref(cache, z["upstream"])
    for mine, theirs in (("w1", "w1"), ("b1", "b1"), ("w2", "w2"), ("b2", "b2"), ("render", "render"), ("warped", "warped_image")):
        want = z[mode + "_grad_" + theirs]
        assert np.abs(g[mine].reshape(want.shape) - want).max() <= 2.0 ** -20 * np.abs(want).max(), (mode, mine)
    assert np.abs(g["warped"][3:]).max() == 0.0 and np.abs(g["warped"][:3]).max() > 0


def test_assembly_is_the_consumers():
    z = np.load(os.path.join(GOLDEN, "consumer.npz"))
    args = z["oracle_color"], z["oracle_cam_feat"], z["oracle_warped_image"], z["oracle_camera_ray"]
    x, ray, c, levels = scenes.fuse_color_inputs(*args, nb_visible_src_frames=3)
    assert levels == 3 == ref.levels_ref(z["oracle_warped_image"], 3) and ref.levels_ref(z["oracle_warped_image"], 2) == 2
    mine = ref.assemble_ref(z["oracle_color"], z["oracle_warped_image"], z["oracle_cam_feat"], z["oracle_camera_ray"], levels)
    assert np.array_equal(mine[0].astype(np.float32), x) and np.array_equal(mine[1].astype(np.float32), ray) and np.array_equal(mine[2].astype(np.float32), c)
    assert np.array_equal(mine[0].astype(np.float32), z["plain_x_views"])          # ... and what the reference's fuse_color handed over
    # the torch composition assembles the same rows: with an identity first layer they come out again
    t = lambda a: torch.tensor(a)
    w1 = torch.zeros(32, 7, dtype=torch.float64)
    w1[:7] = torch.eye(7, dtype=torch.float64)
    w1[7:14] = -torch.eye(7, dtype=torch.float64)
    w2 = torch.zeros(32, 32, dtype=torch.float64)
    w2[:7, :7], w2[:7, 7:14] = torch.eye(7, dtype=torch.float64), -torch.eye(7, dtype=torch.float64)          # relu(x) - relu(-x) = x
    out = ref.torch_composition(t(args[0]), t(args[2]), t(args[1]), t(args[3]), w1, torch.zeros(32, dtype=torch.float64), w2, torch.full((32,), 4.0, dtype=torch.float64), 3, "mean",
                                torch.float64)
    want = mine[0].mean(1) + 4.0
    assert np.abs(out[0, :7].reshape(7, -1).T.numpy() - want).max() < 1e-12 and np.array_equal(out[0, 32:35].numpy(), args[3].astype(np.float64))


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("levels", [None, 2, 0])
def test_backward_restatement_against_autograd_at_float64(mode, levels):
    z = np.load(os.path.join(GOLDEN, "coloragg.npz"))
    inputs = _fixture_inputs(z)
    out, cache = ref.forward_ref(*inputs, 3, mode, levels)
    g = ref.backward_ref(cache, z["upstream"])
    leaves = [torch.tensor(a, dtype=torch.float64).requires_grad_(k in (0, 1, 4, 5, 6, 7)) for k, a in enumerate(inputs)]
    t = ref.torch_composition(*leaves, 3, mode, torch.float64, levels)
    assert np.abs(t.detach().numpy() - out).max() < 1e-13
    grads = torch.autograd.grad((t * torch.tensor(z["upstream"], dtype=torch.float64)).sum(), [leaves[k] for k in (0, 1, 4, 5, 6, 7)], allow_unused=True)
    for name, got in zip(("render", "warped", "w1", "b1", "w2", "b2"), grads):
        got = np.zeros_like(g[name]) if got is None else got.numpy().reshape(g[name].shape)
        assert np.abs(got - g[name]).max() <= 1e-12 * max(1.0, np.abs(g[name]).max()), (mode, levels, name)
    if levels == 0:
        assert np.abs(out[0, :32]).max() == 0.0 and np.array_equal(g["render"], z["upstream"][0, 35:].astype(np.float64)) and np.abs(g["w2"]).max() == 0.0
