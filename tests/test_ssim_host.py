"""The SSIM unit on a CPU-only box: the restatement (tests/ssim_ref.py) at float64 against tests/metrics.ssim and the reference's own numbers, the C ABI
(include/ibgs_ssim.h <-> _lib.SSIM_EXPORTS <-> the built library), the build registration, the window weights compiled into the kernels, the entry
points' validation with null pointers, and the argument checks of ibgs_amd.losses / ibgs_amd.image_eval (which run before any GPU work)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ibgs_amd import _build, _lib, image_eval, losses
from tests import metrics
from tests import ssim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_at_float64_is_the_pinned_definition():
    d = np.load(os.path.join(G, "metrics.npz"))
    a, b = torch.from_numpy(d["a"]), torch.from_numpy(d["b"])
    maps = {form: ref.ssim_map_ref(a, b, torch.float64, form) for form in ref.FORMS}
    for form, m in maps.items():
        assert m.shape == a.shape and m.dtype == torch.float64
        # the reference's own float32 results, with the tolerance tests/test_oracle_golden.py grants the float64 restatement
        assert abs(float(m.mean()) - float(d["ssim"])) < 2e-6, form
        np.testing.assert_allclose(m.mean(dim=(1, 2, 3)).numpy(), d["ssim_per_image"], atol=2e-6)
        # tests/metrics.ssim: numpy float64, a float64 window
        assert abs(float(m.mean()) - metrics.ssim(d["a"], d["b"])) < 1e-6, form
    # the two applications of the same float32 2-D window agree to float64 rounding; the separable form differs by the window's rounding only
    assert float((maps["shift2d"] - maps["conv2d"]).abs().max()) < 1e-12
    assert 0 < float((maps["shift2d"] - maps["separable"]).abs().max()) < 1e-5
    # 3-D input, and differentiable in both images
    a3 = a[0].clone().double().requires_grad_(True)
    b3 = b[0].clone().double().requires_grad_(True)
    m3 = ref.ssim_map_ref(a3, b3)
    assert m3.shape == a3.shape and torch.equal(m3.detach(), maps["shift2d"][0])
    ga, gb = torch.autograd.grad(m3.mean(), [a3, b3])
    assert float(ga.abs().max()) > 0 and float(gb.abs().max()) > 0
    m64, l64, g64, d_map, d_grad = ref.arbiter_and_yardstick(a[:1], b[:1], lambda m: m.mean(), wrt=(0, 1))
    assert 0 < d_map < 1e-4 and len(d_grad) == 2 and all(0 < x < 1e-4 for x in d_grad) and torch.equal(m64, maps["shift2d"][:1])


def test_window_is_the_references_and_the_kernels_hold_it():
    g = ref.gaussian()
    assert g.dtype == torch.float32 and g.shape == (11,) and torch.equal(g, g.flip(0))
    w2 = ref.window_2d()
    assert w2.dtype == torch.float32 and torch.equal(w2, (g[:, None] * g[None, :]))
    src = open(os.path.join(ROOT, "ibgs_amd", "csrc", "shared", "ssim_window.h")).read()          # the one place the kernels of ssim.hip and geoloss.hip take it from
    taps = re.search(r"SSIMW_W\[6\]\s*=\s*\{([^}]*)\}", src).group(1)
    vals = [float.fromhex(t.strip().rstrip("f")) for t in taps.split(",")]
    assert vals == [float(x) for x in g[:6]]


# ---- the ABI and the build ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibgs_ssim.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ibgs_ssim_[a-z_0-9]+)\s*\(", text)))
    assert len(names) == 4
    for n in names:
        assert hasattr(built_lib, n), "libibgs_rast.so does not export %s" % n
    assert sorted(_lib.SSIM_EXPORTS) == names
    defines = re.findall(r"#define\s+IBGS_(SSIM_[A-Z_]+)\s+(\d+)", text)
    assert len(defines) == 2
    for name, val in defines:
        assert getattr(_lib, name) == int(val), name
    # the other export lists are untouched
    assert len(_lib.DTU_EXPORTS) == 8 and len(_lib.PCREG_EXPORTS) == 8 and len(_lib.MESH_EVAL_EXPORTS) == 9 and len(_lib.MESH_EXPORTS) == 5
    assert not any("ssim" in n for n in _lib.EXPORTS + _lib.DTU_EXPORTS + _lib.PCREG_EXPORTS + _lib.MESH_EVAL_EXPORTS + _lib.MESH_EXPORTS + _lib.TSDF_EXPORTS)
    th, tw = losses.ssim_tile()
    assert th >= 11 and tw >= 11 and (th, tw) == (32, 32)


def test_kernels_attributed_to_the_ssim_unit():
    src = open(os.path.join(ROOT, "ibgs_amd", "csrc", "ssim.hip")).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", src)
    assert sorted(kernels) == ["ssim_bwd_kernel", "ssim_final_kernel", "ssim_fwd_kernel"]
    for k in kernels:
        assert _build.tu_of(k) == "ssim", k
    assert _build.tu_of("ssim_fwd_kernel") == "ssim"
    assert "ssim" in _build.SOURCES and "ssim" in _build.UNIT_HEADERS and "ssim" in _build.tu_shas()
    assert "ssim" not in _build.EXTRA          # a tolerance contract: fma is welcome
    assert _build.compile_flags("ssim") == ["--offload-arch=gfx950"] + _build.BASE_FLAGS
    # the kernels of the other units still go where they went
    for k, tu in (("dtu_scan_kernel", "dtu"), ("meval_cell_count", "mesh_eval"), ("l1_rescale_kernel", "loss"), ("mesh_emit", "mesh"), ("scan_kernel", "scan_sort")):
        assert _build.tu_of(k) == tu, k
    assert not re.search(r"atomic", _build._code_only(src)), "the sums are per-workgroup partials and a fixed-order final pass"


def test_sizes_and_validation_before_any_gpu_work(built_lib):
    need = built_lib.ibgs_ssim_required_scratch
    assert need(3, 1080, 1920) >= 3 * 34 * 60 * 3 * 8 and need(1, 1, 1) > 0
    assert need(0, 8, 8) == 0 and need(1, 0, 8) == 0 and need(1, 8, 0) == 0 and need(-1, 8, 8) == 0 and need(1, 65537, 8) == 0 and need(1 << 31, 8, 8) == 0
    assert need(1 << 20, 65536, 65536) == 0          # planes x tiles < 2^31
    err = lambda: built_lib.ibgs_last_error()
    fwd, bwd = built_lib.ibgs_ssim_forward, built_lib.ibgs_ssim_backward
    big = 1 << 20
    assert fwd(None, 0, 3, 8, 8, 128, 128, None, None, 128, None, None, None, None, 128, big) < 0 and b"out of range" in err()
    assert fwd(None, 1, 0, 8, 8, 128, 128, None, None, 128, None, None, None, None, 128, big) < 0 and b"out of range" in err()
    assert fwd(None, 1, 3, 0, 8, 128, 128, None, None, 128, None, None, None, None, 128, big) < 0 and b"out of range" in err()
    assert fwd(None, 1, 3, 8, 65537, 128, 128, None, None, 128, None, None, None, None, 128, big) < 0 and b"out of range" in err()
    assert fwd(None, 1, 3, 8, 8, None, 128, None, None, 128, None, None, None, None, 128, big) < 0 and b"null image" in err()
    assert fwd(None, 1, 3, 8, 8, 128, None, None, None, 128, None, None, None, None, 128, big) < 0 and b"null image" in err()
    assert fwd(None, 1, 3, 8, 8, 128, 128, None, None, None, None, None, None, None, 128, big) < 0 and b"null outputs" in err()
    assert fwd(None, 1, 3, 8, 8, 128, 128, None, None, 128, None, None, None, None, None, big) < 0 and b"null scratch" in err()
    assert fwd(None, 1, 3, 8, 8, 128, 128, None, None, 128, None, None, None, None, 64, big) < 0 and b"aligned" in err()
    assert fwd(None, 1, 3, 8, 8, 128, 128, None, None, None, None, None, None, 128, 128, 16) < 0 and b"needed" in err()
    assert bwd(None, 0, 3, 8, 8, 128, 128, 128, 128, None, 128) < 0 and b"out of range" in err()
    assert bwd(None, 1, 3, 8, 0, 128, 128, 128, 128, None, 128) < 0 and b"out of range" in err()
    assert bwd(None, 1, 3, 8, 8, 128, 128, None, 128, None, 128) < 0 and b"null array" in err()
    assert bwd(None, 1, 3, 8, 8, 128, 128, 128, 128, None, None) < 0 and b"null array" in err()
    assert bwd(None, 1, 3, 8, 8, 128, 128, 128, None, None, 128) < 0 and b"exactly one" in err()
    assert bwd(None, 1, 3, 8, 8, 128, 128, 128, 128, 128, 128) < 0 and b"exactly one" in err()
    th, tw = ctypes.c_int32(-1), ctypes.c_int32(-1)
    built_lib.ibgs_ssim_tile(ctypes.byref(th), None)
    built_lib.ibgs_ssim_tile(None, ctypes.byref(tw))
    assert (th.value, tw.value) == losses.ssim_tile()


def test_cpu_tensors_and_bad_arguments_are_refused(built_lib):
    a, b = torch.rand(2, 3, 12, 14), torch.rand(2, 3, 12, 14)
    for fn in (lambda: losses.ssim(a, b), lambda: losses.ssim(a[0], b[0]), lambda: losses.ssim(a, b, size_average=False), lambda: losses.ssim_map(a, b),
               lambda: losses.ssim_map(a[0], b[0]), lambda: image_eval.image_metrics(a, b), lambda: image_eval.evaluate_images(a, b),
               lambda: image_eval.evaluate_images([a[0], a[1, :, :5]], [b[0], b[1, :, :5]])):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn()
    for fn in (lambda: losses.ssim(a, b, window_size=7), lambda: losses.ssim(a, b, 5), lambda: losses.ssim_map(a, b, window_size=9)):
        with pytest.raises(ValueError, match="window_size"):
            fn()
    for fn in (lambda: losses.ssim(a, b[:, :, :11]), lambda: losses.ssim(a, b[0]), lambda: losses.ssim_map(a, b[:1]), lambda: image_eval.image_metrics(a, b[:, :2])):
        with pytest.raises(ValueError, match="shapes differ"):
            fn()
    for shape in ((2, 3, 0, 14), (2, 3, 12, 0), (3, 0, 5), (0, 3, 4, 4)):
        z = torch.zeros(shape)
        for fn in (lambda: losses.ssim(z, z), lambda: losses.ssim_map(z, z)):
            with pytest.raises(ValueError, match="empty"):
                fn()
    with pytest.raises(ValueError, match="4-D"):
        losses.ssim(a[0], b[0], size_average=False)
    for bad in (torch.rand(12, 14), torch.rand(1, 2, 3, 12, 14)):
        for fn in (lambda: losses.ssim(bad, bad), lambda: losses.ssim_map(bad, bad)):
            with pytest.raises(ValueError, match="3-D or 4-D"):
                fn()
    with pytest.raises(TypeError):
        losses.ssim(a.numpy(), b)
    # evaluate_images: what it is given
    for fn in (lambda: image_eval.evaluate_images(a[0], b[0]), lambda: image_eval.evaluate_images([a], [b]), lambda: image_eval.evaluate_images([a[0]], [b[0], b[1]]),
               lambda: image_eval.evaluate_images([], []), lambda: image_eval.evaluate_images(a, b, names=["one"]), lambda: image_eval.evaluate_images(a, b, names=["x", "x"]),
               lambda: image_eval.evaluate_images([a[0]], [b[0, :, :5]])):
        with pytest.raises(ValueError):
            fn()
    # l1_loss is untouched
    with pytest.raises(RuntimeError, match="MI355X only"):
        losses.l1_loss(a, b)


def test_product_code_does_not_import_the_tests():
    for mod in ("losses.py", "image_eval.py"):
        src = open(os.path.join(ROOT, "ibgs_amd", mod)).read()
        assert not re.search(r"^(import|from)\s+(oracle|tests|lpips|scipy)\b", src, re.M)
    assert "LPIPS" in image_eval.__doc__ and "LPIPS" in image_eval.evaluate_images.__doc__
