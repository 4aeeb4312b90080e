"""The geometry-loss unit on a CPU-only box: the C ABI (include/ibgs_geo_loss.h <-> _lib.GEOLOSS_EXPORTS <-> the built library), the build registration,
the window it takes from the header it shares with ssim.hip, the entry points' validation with null pointers and bad sizes, the argument checks of
ibgs_amd.losses.photometric_loss / normal_consistency (which run before any GPU work), and the float64 restatement (tests/geoloss_ref.py) against the
float32 torch expression of train.py on one small case."""
import ctypes
import os
import re

import pytest
import torch

from ibgs_amd import _build, _lib, losses
from tests import geoloss_ref as ref
from tests import ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ibgs_amd", "csrc", "geoloss.hip")


# ---- the ABI and the build ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_geo_loss.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_[a-z_0-9]+)\s*\(", text)))
    assert len(names) == 6 and all(n.startswith("ibgs_geoloss_") and "ssim" not in n for n in names)
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.GEOLOSS_EXPORTS) == names
    defines = re.findall(r"#define\s+IBGS_(GEOLOSS_[A-Z_]+)\s+(\d+)", text)
    assert len(defines) == 2
    for name, val in defines:
        assert getattr(_lib, name) == int(val), name
    assert _lib.GEOLOSS_MAX_SRC == _lib.MAX_SRC
    # the other export lists are untouched
    assert len(_lib.SSIM_EXPORTS) == 4 and len(_lib.DTU_EXPORTS) == 8 and len(_lib.PCREG_EXPORTS) == 8
    assert not any("geoloss" in n for n in _lib.EXPORTS + _lib.SSIM_EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS)
    th, tw = losses.geoloss_tile()
    assert th >= 11 and tw >= 11 and (th, tw) == (32, 32)


def test_kernels_attributed_to_the_geoloss_unit():
    src = open(SRC).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)
    assert sorted(kernels) == ["geoloss_normal_final_kernel", "geoloss_normal_kernel", "geoloss_photo_bwd_kernel", "geoloss_photo_final_kernel",
                               "geoloss_photo_fwd_kernel", "geoloss_rescale_kernel"]
    others = [sub for sub, tu in _build.KERNEL_TU if tu != "geoloss"]
    for k in kernels:
        assert _build.tu_of(k) == "geoloss", k
        assert not any(sub in k for sub in others), k          # whatever the order of the table
    assert ("geoloss_", "geoloss") in _build.KERNEL_TU[1:]
    assert "geoloss" in _build.SOURCES and "geoloss" in _build.UNIT_HEADERS and "geoloss" in _build.tu_shas()
    assert "geoloss" not in _build.EXTRA          # a tolerance contract, as the ssim unit's
    assert _build.compile_flags("geoloss") == _build.compile_flags("ssim")
    # the kernels of the other units still go where they went
    for k, tu in (("dtu_scan_kernel", "dtu"), ("meval_cell_count", "mesh_eval"), ("l1_rescale_kernel", "loss"), ("mesh_emit", "mesh"), ("scan_kernel", "scan_sort"),
                  ("ssim_fwd_kernel", "ssim"), ("depth_normal_kernel", "depth_normal")):
        assert _build.tu_of(k) == tu, k
    assert not re.search(r"atomic", _build._code_only(src)), "the sums are per-workgroup partials and a fixed-order final pass"
    # no header of its own under csrc/: every header there is hashed into every unit's profile stamp; the one it shares with ssim.hip lies a directory below
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc")) if "geoloss" in f and not f.startswith("_")) == ["geoloss.hip"]
    assert re.findall(r'#include "([^"]+)"', src) == ["common.h", "block_ops.h", "shared/ssim_window.h", "../../include/ibgs_geo_loss.h"]
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "ibgs_amd", "csrc")) if f.endswith(".h")) == ["adam_math.h", "blend.h", "block_ops.h", "common.h", "sh_color.h", "wave_bits.h", "wave_reduce.h"]


def test_window_is_defined_once_in_the_shared_header():
    """Neither unit holds a weight or a C1 / C2 of its own: both include the header, whose values are the reference's."""
    shared = open(os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "ssim_window.h")).read()
    for path in (SRC, os.path.join(ROOT, "ibgs_amd", "csrc", "ssim.hip")):
        text = open(path).read()
        code = _build._code_only(text)
        assert not re.search(r"0[xX][0-9a-fA-F.]+[pP][+-]?\d+", code), path          # no hex-float literal
        assert not re.search(r"\b\w*C[12]\s*=", code), path          # no C1 / C2 defined here
        assert '#include "shared/ssim_window.h"' in text and "SSIMW_" in code, path
    mine = re.search(r"SSIMW_W\[6\]\s*=\s*\{([^}]*)\}", shared).group(1)
    assert len(re.findall(r"0[xX][0-9a-fA-F.]+[pP][+-]?\d+", _build._code_only(shared))) == 6          # the six taps and no other
    assert [float.fromhex(t.strip().rstrip("f")) for t in mine.split(",")] == [float(x) for x in ssim_ref.gaussian()[:6]]
    c1, c2 = re.search(r"SSIMW_C1\s*=\s*([^,;]*),\s*SSIMW_C2\s*=\s*([^,;]*);", shared).groups()
    assert (c1.strip(), c2.strip()) == ("0.01f * 0.01f", "0.03f * 0.03f")          # 0.01^2 and 0.03^2, formed in float32


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_geoloss_required_scratch
    assert need(3, 1080, 1920) >= 3 * 34 * 60 * 3 * 8 and need(1, 1, 1) > 0 and need(5, 65536, 65536) > 0
    assert need(0, 8, 8) == 0 and need(6, 8, 8) == 0 and need(1, 0, 8) == 0 and need(1, 8, 0) == 0 and need(-1, 8, 8) == 0 and need(1, 65537, 8) == 0
    err = lambda: built_lib.ibgs_last_error()
    fwd, bwd = built_lib.ibgs_geoloss_photo_forward, built_lib.ibgs_geoloss_photo_backward
    nfw, rsc = built_lib.ibgs_geoloss_normal_forward, built_lib.ibgs_geoloss_rescale
    big = 1 << 20
    # photometric forward: (stream, S, H, W, gt, warped, feat, w_p, w_s, dplanes, loss, nv, scratch, bytes)
    for s, h, w in ((0, 8, 8), (6, 8, 8), (3, 0, 8), (3, 8, 65537), (-1, 8, 8)):
        assert fwd(None, s, h, w, 128, 128, 128, 0.3, 1.0, None, 128, 128, 128, big) < 0 and b"out of range" in err()
    for k in (4, 5, 6):
        args = [None, 3, 8, 8, 128, 128, 128, 0.3, 1.0, None, 128, 128, 128, big]
        args[k] = None
        assert fwd(*args) < 0 and b"null image" in err()
    for k in (10, 11):
        args = [None, 3, 8, 8, 128, 128, 128, 0.3, 1.0, None, 128, 128, 128, big]
        args[k] = None
        assert fwd(*args) < 0 and b"null outputs" in err()
    assert fwd(None, 3, 8, 8, 128, 128, 128, float("nan"), 1.0, None, 128, 128, 128, big) < 0 and b"finite" in err()
    assert fwd(None, 3, 8, 8, 128, 128, 128, 0.3, float("inf"), None, 128, 128, 128, big) < 0 and b"finite" in err()
    assert fwd(None, 3, 8, 8, 128, 128, 128, 0.3, 1.0, None, 128, 128, None, big) < 0 and b"null scratch" in err()
    assert fwd(None, 3, 8, 8, 128, 128, 128, 0.3, 1.0, None, 128, 128, 64, big) < 0 and b"aligned" in err()
    assert fwd(None, 3, 8, 8, 128, 128, 128, 0.3, 1.0, None, 128, 128, 128, 16) < 0 and b"needed" in err()
    # photometric backward: (stream, S, S_total, H, W, gt, warped, feat, dplanes, nv, go, w_p, w_s, grad)
    good = [None, 3, 4, 8, 8, 128, 128, 128, 128, 128, 128, 0.3, 1.0, 128]
    for k, v in ((1, 0), (1, 6), (2, 0), (2, 6), (3, 0), (4, 65537)):
        args = list(good)
        args[k] = v
        assert bwd(*args) < 0 and b"out of range" in err(), (k, v)
    args = list(good)
    args[1], args[2] = 4, 3
    assert bwd(*args) < 0 and b"out of range" in err()
    for k in (5, 6, 7, 8, 9, 10, 13):
        args = list(good)
        args[k] = None
        assert bwd(*args) < 0 and b"null array" in err(), k
    args = list(good)
    args[11] = float("nan")
    assert bwd(*args) < 0 and b"finite" in err()
    # normal forward: (stream, H, W, n, dn, weight, gn, gdn, loss, scratch, bytes)
    good = [None, 8, 8, 128, 128, 0.03, None, None, 128, 128, big]
    for k, v in ((1, 0), (2, 0), (1, 65537)):
        args = list(good)
        args[k] = v
        assert nfw(*args) < 0 and b"out of range" in err()
    for k, msg in ((3, b"null image"), (4, b"null image"), (8, b"null outputs"), (9, b"null scratch")):
        args = list(good)
        args[k] = None
        assert nfw(*args) < 0 and msg in err(), k
    args = list(good)
    args[5] = float("nan")
    assert nfw(*args) < 0 and b"finite" in err()
    args = list(good)
    args[10] = 16
    assert nfw(*args) < 0 and b"needed" in err()
    # rescale: (stream, n, grad, scale)
    assert rsc(None, 0, 128, 128) < 0 and b"out of range" in err()
    assert rsc(None, -5, 128, 128) < 0 and b"out of range" in err()
    assert rsc(None, 8, None, 128) < 0 and b"null array" in err()
    assert rsc(None, 8, 128, None) < 0 and b"null array" in err()
    th, tw = ctypes.c_int32(-1), ctypes.c_int32(-1)
    built_lib.ibgs_geoloss_tile(ctypes.byref(th), None)
    built_lib.ibgs_geoloss_tile(None, ctypes.byref(tw))
    assert (th.value, tw.value) == losses.geoloss_tile()


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    h, w = 12, 14
    gt = torch.rand(3, h, w)
    for st in (1, 3, 5):
        for warped, feat in ((torch.rand(3 * st, h, w), torch.rand(4 * st, h, w)), (torch.rand(st, 3, h, w), torch.rand(st, 4, h, w)),
                             (torch.rand(st, 3, h, w), torch.rand(4 * st, h, w))):
            with pytest.raises(RuntimeError, match="MI355X only"):
                losses.photometric_loss(gt, warped, feat)
    with pytest.raises(RuntimeError, match="MI355X only"):
        losses.normal_consistency(torch.rand(3, h, w), torch.rand(3, h, w))
    ok_w, ok_f = torch.rand(9, h, w), torch.rand(12, h, w)
    bad = [
        (gt, torch.rand(0, h, w), torch.rand(0, h, w)),               # S_total = 0
        (gt, torch.rand(0, 3, h, w), torch.rand(0, 4, h, w)),
        (gt, torch.rand(18, h, w), torch.rand(24, h, w)),             # S_total = 6
        (gt, torch.rand(6, 3, h, w), torch.rand(6, 4, h, w)),
        (gt, torch.rand(10, h, w), torch.rand(12, h, w)),             # channels per source
        (gt, torch.rand(3, 4, h, w), torch.rand(3, 4, h, w)),
        (gt, ok_w, torch.rand(13, h, w)),
        (gt, ok_w, torch.rand(3, 3, h, w)),
        (gt, ok_w, torch.rand(8, h, w)),                              # the two disagree on S_total
        (gt, torch.rand(9, h, w + 1), ok_f),                          # H, W
        (gt, ok_w, torch.rand(12, h + 1, w)),
        (torch.rand(3, h + 1, w), ok_w, ok_f),
        (torch.rand(1, h, w), ok_w, ok_f),                            # gt_image itself
        (torch.rand(1, 3, h, w), ok_w, ok_f),
        (torch.rand(3, 0, w), torch.rand(9, 0, w), torch.rand(12, 0, w)),
        (gt, torch.rand(h, w), ok_f),
        (gt, ok_w, torch.rand(1, 3, 4, h, w)),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            losses.photometric_loss(*args)
    for kw in (dict(nb_visible_src_frames=0), dict(nb_visible_src_frames=-1), dict(nb_visible_src_frames=1.5), dict(photo_weight=float("nan")),
               dict(photo_ssim_weight=float("inf"))):
        with pytest.raises(ValueError):
            losses.photometric_loss(gt, ok_w, ok_f, **kw)
    with pytest.raises(ValueError, match="gt_image requires grad"):
        losses.photometric_loss(gt.clone().requires_grad_(True), ok_w, ok_f)
    with pytest.raises(TypeError):
        losses.photometric_loss(gt.numpy(), ok_w, ok_f)
    with pytest.raises(TypeError):
        losses.photometric_loss(gt, ok_w.numpy(), ok_f)
    n = torch.rand(3, h, w)
    for a, b in ((n, torch.rand(3, h, w + 1)), (n, torch.rand(2, h, w)), (torch.rand(1, 3, h, w), n), (torch.rand(h, w), torch.rand(h, w)), (torch.rand(3, 0, w), torch.rand(3, 0, w))):
        with pytest.raises(ValueError):
            losses.normal_consistency(a, b)
    with pytest.raises(ValueError, match="finite"):
        losses.normal_consistency(n, n, weight=float("nan"))
    with pytest.raises(TypeError):
        losses.normal_consistency(n.numpy(), n)
    src = open(os.path.join(ROOT, "ibgs_amd", "losses.py")).read()
    assert not re.search(r"^(import|from)\s+(oracle|tests)\b", src, re.M)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def _torch_photometric32(gt_image, warped_image, cam_feat, nb, photo_weight, photo_ssim_weight):
    """train.py:320-338 as written, at float32, with the reference's own convolution call for the map (ssim_ref's "conv2d" form)."""
    h, w = gt_image.shape[-2:]
    warped_image = warped_image.view(-1, 3, h, w)[:nb]
    cam_feat = cam_feat.view(-1, 4, h, w)[:nb]
    valid_mask = torch.sum(cam_feat, dim=1, keepdim=True) > 0
    ref_image = gt_image.unsqueeze(0)
    masked = valid_mask.float() * warped_image + (1 - valid_mask.float()) * ref_image
    if torch.sum(valid_mask) > 0:
        ssim_loss = 1 - torch.stack([ssim_ref.ssim_map_ref(ref_image[0], masked[i], torch.float32, "conv2d").mean(0) for i in range(len(masked))])
        ssim_loss = torch.sum(ssim_loss * valid_mask[:, 0]) / torch.sum(valid_mask[:, 0])
        l1 = torch.abs(ref_image - masked).mean(1)
        l1 = torch.sum(l1 * valid_mask[:, 0]) / torch.sum(valid_mask[:, 0])
        return (((1 - photo_ssim_weight) * l1 + photo_ssim_weight * ssim_loss) * photo_weight).mean()
    return torch.tensor(0.0)


def small_case(seed=0, st=4, h=13, w=17):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, h, w, generator=g)
    warped = (gt[None] + 0.08 * torch.randn(st, 3, h, w, generator=g)).clamp(0, 1)
    mask = torch.rand(st, 1, h, w, generator=g) < 0.4
    feat = (torch.randn(st, 4, h, w, generator=g) * 0.2 + 0.5) * mask          # zeros in the invalid slots, signed features with sums well above zero elsewhere
    feat[:, 0][mask[:, 0] & (feat.sum(1) < 0.3)] += 1.0
    ref.assert_decided(feat)
    assert bool(((feat.sum(1, keepdim=True) > 0) == mask).all())
    return gt, warped.reshape(3 * st, h, w), feat.reshape(4 * st, h, w), mask


def test_restatement_against_the_float32_torch_expression():
    gt, warped, feat, mask = small_case()
    for pw, ws in ((0.3, 1.0), (0.3, 0.0), (0.7, 0.35)):
        x64 = warped.clone().requires_grad_(True)
        l64 = ref.photometric_ref(gt, x64, feat, 3, pw, ws)
        assert l64.dtype == torch.float64 and l64.shape == ()
        g64, = torch.autograd.grad(l64, x64)
        x32 = warped.clone().requires_grad_(True)
        l32 = _torch_photometric32(gt, x32, feat, 3, pw, ws)
        g32, = torch.autograd.grad(l32, x32)
        assert abs(float(l64.detach()) - float(l32.detach())) < 2e-6 and float(l64.detach()) > 0
        assert float((g64 - g32.double()).abs().max()) < 1e-4 * float(g64.abs().max())
        g = g64.view(4, 3, 13, 17)
        assert float(g[3].abs().max()) == 0.0 and float(g[:3][~mask[:3].expand(3, 3, 13, 17)].abs().max()) == 0.0 and float(g[:3].abs().max()) > 0
        # both layouts, and the other forms of the window
        assert torch.equal(ref.photometric_ref(gt, warped.view(4, 3, 13, 17), feat.view(4, 4, 13, 17), 3, pw, ws), l64.detach())
        for form in ("conv2d", "separable"):
            assert abs(float(ref.photometric_ref(gt, warped, feat, 3, pw, ws, torch.float32, form)) - float(l64.detach())) < 2e-6
    # more sources asked for than there are; no valid pixel
    assert torch.equal(ref.photometric_ref(gt, warped, feat, 9), ref.photometric_ref(gt, warped, feat, 4))
    x = warped.clone().requires_grad_(True)
    zero = ref.photometric_ref(gt, x, torch.zeros_like(feat), 3)
    assert float(zero.detach()) == 0.0 and float(torch.autograd.grad(zero, x)[0].abs().max()) == 0.0
    m = ref.mean_map_ref(gt, warped, feat, 3)
    assert m.shape == (3, 13, 17) and float(m.max()) <= 1.0 + 1e-12
    # the condition on the inputs notices a sum that an order could flip
    close = torch.tensor([1.0, -1.0, 2.0 ** -30, 0.0]).view(1, 4, 1, 1)
    with pytest.raises(AssertionError):
        ref.assert_decided(close)
    # the normal term
    g = torch.Generator().manual_seed(5)
    n, dn = torch.nn.functional.normalize(torch.randn(3, 13, 17, generator=g), dim=0), torch.nn.functional.normalize(torch.randn(3, 13, 17, generator=g), dim=0)
    a, b = n.double().requires_grad_(True), dn.double().requires_grad_(True)
    l64 = ref.normal_ref(a, b)
    ga, gb = torch.autograd.grad(l64, [a, b])
    weight = 0.03
    normal_loss1 = weight * (((dn - n)).abs().sum(0)).mean()
    normal_loss2 = weight * (1 - ((dn * n).sum(0))).mean()
    assert abs(float(0.4 * normal_loss1 + 0.6 * normal_loss2) - float(l64.detach())) < 1e-7
    k = weight / (13 * 17)
    assert float((ga - k * (-0.4 * torch.sign(dn - n).double() - 0.6 * dn.double())).abs().max()) < 1e-12
    assert float((gb - k * (0.4 * torch.sign(dn - n).double() - 0.6 * n.double())).abs().max()) < 1e-12
    assert abs(float(ref.normal_ref(n, n, 0.03)) - 0.03 * 0.6 * float((1 - (n.double() ** 2).sum(0)).mean())) < 1e-15
