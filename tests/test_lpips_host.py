"""The LPIPS unit on a CPU-only box: the C ABI (include/ibgs_lpips.h <-> _lib.LPIPS_EXPORTS <-> the built library), the build registration and the kernel
names, the arena's documented layout against a restatement (tests/lpips_ref.arena_layout) and every validation message of the entry points with null pointers
and bad sizes (validation precedes every HIP call), the three state-dict namings and the named refusals of `LPIPSNet.load_state_dict`, the refusals of
`lpips` (which run before any GPU work), and the arbiter: tests/lpips_ref.forward_ref and torch_composition at float64 are two independent statements that
agree to 1e-12."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, image_eval, lpips as lp
from tests import lpips_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "lpips.hip")
HEADER = os.path.join(ROOT, "include", "ibgs_lpips.h")


# ---- the ABI and the build ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(["ibgs_lpips_required_scratch", "ibgs_lpips_conv3", "ibgs_lpips_forward"]) == sorted(_lib.LPIPS_EXPORTS)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert dict(re.findall(r"#define\s+IBGS_(LPIPS_[A-Z_]+)\s+(\d+)", text)) == {"LPIPS_MIN_SIDE": str(_lib.LPIPS_MIN_SIDE), "LPIPS_MAX_SIDE": str(_lib.LPIPS_MAX_SIDE),
                                                                                 "LPIPS_CONVS": str(_lib.LPIPS_CONVS), "LPIPS_TAPS": str(_lib.LPIPS_TAPS)}
    assert (_lib.LPIPS_MIN_SIDE, _lib.LPIPS_MAX_SIDE, _lib.LPIPS_CONVS, _lib.LPIPS_TAPS) == (16, 4096, 13, 5)
    # the channel table is the restatement's, and the source's
    assert _lib.LPIPS_CHANNELS == ref.CHANNELS and _lib.LPIPS_TAP_CONV == ref.TAP_AFTER and lp.TAP_CHANNELS == ref.TAP_CHANNELS
    assert tuple(i for i in range(1, 13) if _lib.LPIPS_LEVEL[i] != _lib.LPIPS_LEVEL[i - 1]) == ref.POOL_BEFORE
    assert lp.CONV_NAMES == ref.CONVS and lp.FEATURE_INDEX == ref.FEATURE_INDEX and lp.LIN_NAMES == ref.LINS
    src = open(SRC).read()
    assert "{%s}" % ", ".join(map(str, _lib.LPIPS_CHANNELS)) in src and "{%s}" % ", ".join(map(str, _lib.LPIPS_LEVEL)) in src
    assert "{%s}" % ", ".join(map(str, _lib.LPIPS_TAP_CONV)) in src
    # the other export lists do not hold these
    others = (_lib.EXPORTS + _lib.SSIM_EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS + _lib.GEOLOSS_EXPORTS
              + _lib.CAGG_EXPORTS + _lib.HG_EXPORTS + _lib.HGB_EXPORTS + _lib.HGH_EXPORTS)
    assert not any("lpips" in n for n in others)


def test_build_registration_and_the_kernels():
    src = open(SRC).read()
    kernels = sorted(set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)))
    assert kernels == ["lpips_conv3_kernel", "lpips_final_kernel", "lpips_head_kernel"]          # ONE templated convolution, the head, the final sum
    at = [i for i, (sub, tu) in enumerate(_build.KERNEL_TU) if tu == "lpips"]
    assert len(at) == 1 and _build.KERNEL_TU[at[0]] == ("lpips_", "lpips")
    for k in kernels:
        assert k.startswith("lpips_") and _build.tu_of(k) == "lpips", k
        # no entry in front of it claims a kernel of this unit; the entries behind it (l1_, hg_, scan_, cell_, mesh_, ...) never get to
        assert not any(sub in k for sub, _ in _build.KERNEL_TU[:at[0]]), k
    assert "lpips" in _build.SOURCES and "lpips" in _build.tu_shas() and "lpips" not in _build.EXTRA
    assert _build.compile_flags("lpips") == _build.compile_flags("hourglass")
    assert [os.path.basename(h) for h in _build.UNIT_HEADERS["lpips"]] == ["ibgs_lpips.h", "conv_tile.h"] and all(os.path.exists(h) for h in _build.UNIT_HEADERS["lpips"])
    # the other units' kernels still go where they went
    assert _build.tu_of("hg_conv3_kernel") == "hourglass" and _build.tu_of("hgh_conv3_kernel") == "hghalf" and _build.tu_of("ssim_forward_kernel") == "ssim"
    assert _build.tu_of("l1_loss_kernel") == "loss" and _build.tu_of("meval_cell_count") == "mesh_eval"
    code = _build._code_only(src)
    assert "atomic" not in code.lower() and "asm" not in code.lower()          # nothing crosses a workgroup but the partials; builtins only
    tile = _build._code_only(open(os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "conv_tile.h")).read())          # the 16 x 16 tile it shares with the hourglass units
    assert re.findall(r"__builtin_amdgcn_mfma_\w+", tile) == ["__builtin_amdgcn_mfma_f32_16x16x4f32"]          # the exact f32 form, once
    assert "__builtin_amdgcn_mfma" not in code and "ct_mfma(" in code
    assert re.search(r"constexpr int CT_TILE = 16;", tile) and re.search(r"constexpr int CT_THREADS = 256;", tile)
    assert not re.search(r"constexpr int (\w*TILE|LP_THREADS) =", code) and re.search(r"__launch_bounds__\(CT_THREADS, 2\) lpips_conv3_kernel", code)
    assert re.search(r"const dim3 grid\(\(unsigned\)\(\(a\.w \+ CT_TILE - 1\) / CT_TILE\), \(unsigned\)\(\(a\.h \+ CT_TILE - 1\) / CT_TILE\), ", code)
    assert len(re.findall(r"grid, dim3\(CT_THREADS\), 0, st, a\)", code)) == 3
    assert len(re.findall(r"lpips_conv3_kernel<\w+, \w+>", code)) == 3          # three instantiations: plain, pooled, first
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "block_ops.h", "shared/conv_tile.h", "../../include/ibgs_lpips.h"]


def test_no_code_path_opens_a_url():
    text = open(os.path.join(ROOT, "ibgs_amd", "lpips.py")).read()
    for word in ("http:", "https:", "urllib", "requests", "load_state_dict_from_url", "download_url", "torch.hub.load"):
        assert word not in text, word
    assert "torch.load(path" in inspect.getsource(lp.LPIPSNet.from_files)
    assert "float16" in lp.__doc__ or "half-precision" in lp.__doc__          # the known follow-up is named


def test_arena_layout_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_lpips_required_scratch
    for h, w in ((16, 16), (33, 37), (1080, 1920), (17, 19), (4096, 4096), (16, 4096)):
        total, at, partial_at = ref.arena_layout(h, w)
        assert need(h, w) == total and total % 128 == 0, (h, w)
        mine, mine_partial = lp._stage_offsets(h, w)
        assert list(mine) == [at[name] for name in ref.CONVS] and mine_partial == partial_at, (h, w)
        assert all((4 * o) % 512 == 0 for o in mine)
    # the header writes the numbers down
    header = open(HEADER).read()
    assert "{:,}".format(need(1080, 1920)).replace(",", " ") in header and "{:,}".format(need(4096, 4096)).replace(",", " ") in header
    assert need(1080, 1920) == 2123452800 and need(4096, 4096) < 20 * 10 ** 9
    for h, w in ((15, 16), (16, 15), (0, 16), (-1, 16), (4097, 16), (16, 4097), (1 << 40, 16)):
        assert need(h, w) == 0, (h, w)
    # the taps are views at those offsets
    h, w = 33, 37
    arena = torch.zeros(need(h, w), dtype=torch.uint8)
    fx, fy = lp._tap_views(arena, h, w)
    _, at, _ = ref.arena_layout(h, w)
    sides = lp.level_sides(h, w)
    assert sides == ((33, 37), (16, 18), (8, 9), (4, 4), (2, 2))
    for k, conv in enumerate(("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3")):
        c = ref.TAP_CHANNELS[k]
        assert tuple(fx[k].shape) == tuple(fy[k].shape) == (c,) + sides[k] and fx[k].is_contiguous()
        assert fx[k].data_ptr() - arena.data_ptr() == 4 * at[conv] and fy[k].data_ptr() - fx[k].data_ptr() == 4 * c * sides[k][0] * sides[k][1]
    # no two taps overlap
    spans = sorted((at[c], at[c] + 2 * ch * s[0] * s[1]) for c, ch, s in zip(("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3"), ref.TAP_CHANNELS, sides))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))

    err = lambda: built_lib.ibgs_last_error()
    fwd = built_lib.ibgs_lpips_forward
    tab = lambda n, hole=None: (ctypes.c_void_p * n)(*[None if i == hole else 128 for i in range(n)])
    big = 1 << 40
    # (stream, H, W, x, y, conv_w, conv_b, lin_w, lpips, tap_values, maps, scratch, bytes)
    good = lambda: [None, 16, 16, 128, 128, tab(13), tab(13), tab(5), 128, None, None, 128, big]
    for k, v in ((1, 15), (2, 15), (1, 0), (2, -5), (1, 4097), (2, 4097)):
        args = good()
        args[k] = v
        assert fwd(*args) < 0 and b"out of range" in err() and b"lpips_forward" in err() and b"16 .. 4096" in err(), (k, v)
    for k, what in ((3, b"x"), (4, b"y")):
        args = good()
        args[k] = None
        assert fwd(*args) < 0 and b"null input: " + what in err()
    for k, what in ((5, b"conv_w"), (6, b"conv_b"), (7, b"lin_w")):
        args = good()
        args[k] = None
        assert fwd(*args) < 0 and b"null parameters" in err() and what in err()
    for i in (0, 7, 12):
        for k, what in ((5, b"weight"), (6, b"bias")):
            args = good()
            args[k] = tab(13, i)
            assert fwd(*args) < 0 and b"null parameters: convolution %d's " % i + what in err(), (i, what)
    args = good()
    args[7] = tab(5, 3)
    assert fwd(*args) < 0 and b"lin 3's weight" in err()
    args = good()
    args[8] = None
    assert fwd(*args) < 0 and b"null outputs" in err()
    for k, v, msg in ((11, None, b"null scratch"), (11, 64, b"aligned"), (12, need(16, 16) - 1, b"needed")):
        args = good()
        args[k] = v
        assert fwd(*args) < 0 and msg in err(), k
    conv = built_lib.ibgs_lpips_conv3
    # (stream, hs, ws, cin, cout, pool, zscore, in_x, in_y, weight, bias, out)
    good3 = [None, 16, 16, 64, 64, 0, 0, 128, 128, 128, 128, 128]
    for k, v, msg in ((1, 0, b"out of range"), (2, 4097, b"out of range"), (4, 48, b"cout"), (4, 576, b"cout"), (3, 3, b"cin"), (3, 62, b"cin"), (7, None, b"null input"),
                      (8, None, b"null input"), (9, None, b"null parameters"), (10, None, b"null parameters"), (11, None, b"null output")):
        args = list(good3)
        args[k] = v
        assert conv(*args) < 0 and msg in err() and b"lpips_conv3" in err(), (k, v)
    for hs, pool, z, cin in ((1, 1, 0, 64), (16, 1, 1, 3), (16, 0, 1, 64)):
        args = list(good3)
        args[1], args[3], args[5], args[6] = hs, cin, pool, z
        assert conv(*args) < 0, (hs, pool, z, cin)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_namings_and_named_refusals():
    p = ref.seeded_params(5)
    own, tv, theirs = ref.state_dicts(p)
    nets = []
    for sd in (own, tv, theirs):
        net = lp.LPIPSNet()
        result = net.load_state_dict(dict(sd))
        assert not result.missing_keys and not result.unexpected_keys
        nets.append(net)
    for net in nets:
        got = net.state_dict()
        assert list(got) == lp.LPIPSNet.parameter_names() and len(got) == 31
        assert all(torch.equal(got[k], own[k]) and got[k].dtype == torch.float32 for k in own)
        assert all(not q.requires_grad for q in net.parameters())
    assert tuple(nets[1].lin4_w.shape) == (512,) and tuple(nets[1].conv1_1_w.shape) == (64, 3, 3, 3)
    fresh = lp.LPIPSNet()
    assert all(not q.requires_grad for q in fresh.parameters()) and not torch.equal(fresh.conv2_1_w, lp.LPIPSNet().conv2_1_w)
    assert bool((fresh.lin3_w >= 0).all()) and 0.8 < float(fresh.conv4_2_w.std()) / (2.0 / (9 * 512)) ** 0.5 < 1.2
    twice = dict(tv)
    twice["conv3_2_w"] = own["conv3_2_w"]
    with pytest.raises(ValueError, match=r"conv3_2_w.*given twice"):
        lp.LPIPSNet().load_state_dict(twice)
    both = dict(tv)
    both["net.layers.0.bias"] = own["conv1_1_b"]
    with pytest.raises(ValueError, match=r"conv1_1_b.*given twice"):
        lp.LPIPSNet().load_state_dict(both)
    bad = dict(theirs)
    bad["net.layers.17.weight"] = torch.zeros(512, 256, 1, 1)
    with pytest.raises(ValueError, match=r"wrong shape.*conv4_1_w"):
        lp.LPIPSNet().load_state_dict(bad)
    bad = dict(own)
    bad["lin2_w"] = torch.zeros(1, 128)
    with pytest.raises(ValueError, match=r"wrong shape.*lin2_w"):
        lp.LPIPSNet().load_state_dict(bad)
    for key, name in (("features.28.bias", "conv5_3_b"), ("lin0.model.1.weight", "lin1_w"), ("features.0.weight", "conv1_1_w")):
        missing = dict(tv)
        del missing[key]
        with pytest.raises(KeyError, match=r"missing layer.*" + name):
            lp.LPIPSNet().load_state_dict(missing)


def test_from_files_reads_two_local_files(tmp_path):
    own, tv, _ = ref.state_dicts(ref.seeded_params(6))
    vgg = {k: v for k, v in tv.items() if not k.startswith("lin")}
    lin = {k: v for k, v in tv.items() if k.startswith("lin")}
    assert len(vgg) == 26 + 3 and len(lin) == 5
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    net = lp.LPIPSNet.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))
    assert all(torch.equal(v, own[k]) for k, v in net.state_dict().items())
    with pytest.raises(ValueError, match="in both files"):
        lp.LPIPSNet.from_files(str(tmp_path / "vgg.pth"), str(tmp_path / "vgg.pth"))
    torch.save({}, tmp_path / "empty.pth")
    with pytest.raises(KeyError, match="missing layer.*lin1_w"):
        lp.LPIPSNet.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "empty.pth"))


def test_refusals_without_a_gpu(built_lib):
    net = lp.LPIPSNet()
    x = torch.rand(2, 3, 16, 17)
    for a, b in ((x, x), (x[0], x[0]), (x.permute(0, 1, 3, 2), x.permute(0, 1, 3, 2))):
        with pytest.raises(RuntimeError, match="MI355X only"):          # CPU tensors
            lp.lpips(a, b, net)
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(x, x, return_maps=True)
    with pytest.raises(RuntimeError, match="MI355X only"):
        image_eval.evaluate_images([x[0]], [x[0]], lpips_net=net)
    for shape in ((4, 16, 16), (2, 1, 16, 16)):
        with pytest.raises(ValueError, match="channels"):
            lp.lpips(torch.rand(shape), torch.rand(shape), net)
    for shape in ((3, 15, 16), (3, 16, 15), (1, 3, 16, 4097), (3, 4097, 16)):
        with pytest.raises(ValueError, match=r"out of range \(sides 16 \.\. 4096"):
            lp.lpips(torch.empty(shape), torch.empty(shape), net)
    with pytest.raises(ValueError, match=r"\(N, 3, H, W\) or \(3, H, W\)"):
        lp.lpips(torch.rand(16, 16), torch.rand(16, 16), net)
    with pytest.raises(ValueError, match="renders are .* gts"):
        lp.lpips(torch.rand(3, 16, 16), torch.rand(3, 16, 17), net)
    with pytest.raises(TypeError, match="LPIPSNet"):
        lp.lpips(x, x, torch.nn.Linear(1, 1))
    with pytest.raises(TypeError, match="tensor"):
        lp.lpips(x.numpy(), x, net)
    with pytest.raises(TypeError, match="floating"):
        lp.lpips((x * 255).to(torch.uint8), (x * 255).to(torch.uint8), net)
    # the keyword's default leaves the two functions of image_eval as they were
    for fn in (image_eval.image_metrics, image_eval.evaluate_images):
        assert inspect.signature(fn).parameters["lpips_net"].default is None
    assert list(inspect.signature(lp.lpips).parameters)[:5] == ["renders", "gts", "net", "return_maps", "return_features"]
    assert "NOT computed" not in image_eval.__doc__ and "LPIPSNet" in image_eval.__doc__


# ---- the arbiter -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(16, 16), (17, 19)])
def test_the_arbiter_is_two_statements_that_agree(h, w):
    p = ref.seeded_params(5)
    x, y = ref.seeded_pair(100 * h + w, h, w)
    want = ref.forward_ref(x, y, p)
    t64 = ref.torch_composition(x, y, p, torch.float64)
    for (name, a), (_, b) in zip(ref.flat_items(want), ref.flat_items(t64)):
        assert a.dtype == np.float64 and b.dtype == torch.float64 and a.shape == tuple(b.shape), name
        diff = float(np.abs(a - b.numpy()).max())
        print("%dx%d %-8s max |f64| %.3g  ReLU-dead %.2f  all-zero pixels %d  numpy against torch at float64 %.1e"
              % (h, w, name, np.abs(a).max(), (a == 0).mean(), int((np.abs(a).reshape(a.shape[0], -1).max(0) == 0).sum()) if name.startswith("tap") else 0, diff))
        assert diff <= 1e-12, (name, diff)
        if name.startswith("tap"):
            assert 0.3 < (a == 0).mean() < 0.7 and 0.1 < np.abs(a).max() < 20
    assert np.abs(want["v"] - t64["v"].numpy()).max() <= 1e-12 and abs(float(want["lpips"]) - float(t64["lpips"])) <= 1e-12
    assert 0.01 < float(want["lpips"]) < 0.1 and abs(float(want["lpips"]) - float(want["v"].sum())) < 1e-15
    sides = lp.level_sides(h, w)
    assert [m.shape for m in want["maps"]] == list(sides) and [t.shape for t in want["taps_x"]] == [(c,) + s for c, s in zip(ref.TAP_CHANNELS, sides)]
    # dead_tap5: relu5_3 is exactly zero, its map and v_5 are 0 (not NaN), the rest is unchanged
    dead = ref.forward_ref(x, y, ref.seeded_params(5, "dead_tap5"))
    assert not dead["taps_x"][4].any() and not dead["maps"][4].any() and dead["v"][4] == 0 and np.isfinite(dead["lpips"])
    assert np.array_equal(dead["v"][:4], want["v"][:4])
    # the float32 chain is the same function, a few 1e-6 away
    if (h, w) == (16, 16):
        chain = ref.chain_f32(x, y, p)
        assert all(c.dtype == np.float32 for _, c in ref.flat_items(chain))
        assert 0 < max(float(np.abs(c - a).max()) for (_, a), (_, c) in zip(ref.flat_items(want), ref.flat_items(chain))) < 1e-4
        assert abs(float(chain["lpips"]) - float(want["lpips"])) < 1e-6
