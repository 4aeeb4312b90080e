"""The SH colours of a hinted forward ride in the depth sort's launches (sh_color.h: ShRide; scan_sort.hip: onesweep_hist_sh_kernel,
onesweep_pass_sh_kernel), the R note in the first of them.  Where they run must not show: records, clamp bits, the depth order, the tile
lists and the image are bit-identical to the standalone sh_color_kernel in front of the sort (ibgs_debug_set_sh_ride(0)) -- for every SH degree
and both coefficient layouts, on C1, C3 and a trained scene, with a hint that is large enough, one that is too small, and no hint at all (the
synchronous path, which never rides).  One scene spreads its depths over several float exponents, so that the sort's top-byte pass moves keys."""
import ctypes

import numpy as np
import pytest
import torch

from ibgs_amd import _lib, rasterizer, synthetic as syn
from ibgs_amd.rasterizer import GaussianRasterizer
from tests import hipref

pytestmark = pytest.mark.gpu


def _lib_hooks():
    lib = _lib.load()
    lib.ibgs_debug_set_sh_ride.restype = None
    lib.ibgs_debug_set_sh_ride.argtypes = [ctypes.c_int32]
    return lib


def _slice(buf, off, dtype, count):
    n = np.dtype(dtype).itemsize * int(count)
    return buf.view(torch.uint8)[off:off + n].cpu().numpy().view(dtype).copy()


def _front(inp, ride, hint, split=False):
    """One forward; hint: None = synchronous sizing, else the R the previous call is pretended to have returned."""
    lib = _lib_hooks()
    P, W, H = inp["means3D"].shape[0], int(inp["W"]), int(inp["H"])
    old = rasterizer.RENDERED_HINT
    rasterizer._last_rendered.clear()
    rasterizer.RENDERED_HINT = hint is not None
    if hint is not None:
        rasterizer._last_rendered[(torch.cuda.current_device(), P, W, H, False, False)] = hint
    lib.ibgs_debug_set_sh_ride(1 if ride else 0)
    try:
        st = hipref.settings_from(inp, "cuda")
        lv = hipref.leaf_inputs(inp, "cuda")
        kw = dict(means3D=lv["means3D"], means2D=lv["means2D"], means2D_abs=lv["means2D_abs"], opacities=lv["opacities"], scales=lv["scales"], rotations=lv["rotations"])
        if split:
            shs = lv["shs"].detach()
            outs = GaussianRasterizer(st)(shs=shs[:, :1].contiguous().requires_grad_(True), shs_rest=shs[:, 1:].contiguous().requires_grad_(True), **kw)
        else:
            outs = GaussianRasterizer(st)(shs=lv["shs"], **kw)
        torch.cuda.synchronize()
    finally:
        rasterizer.RENDERED_HINT = old
        lib.ibgs_debug_set_sh_ride(1)
    node = outs[0].grad_fn
    geom, binning, img = node.saved_tensors[-3:]
    R = int(node.num_rendered)
    go = lambda n: lib.ibgs_geom_offset(P, n.encode())
    offsets = _slice(geom, go("offsets"), np.uint32, P + 5)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    s = {
        "R": R,
        "rec": _slice(geom, go("rec"), np.uint32, P * 16).reshape(P, 16),
        "clamped": _slice(geom, go("clamped"), np.uint8, P),
        "depth_keys": _slice(geom, go("depths"), np.uint32, P),
        "tiles": _slice(geom, go("tiles"), np.uint32, P),
        "kept": int(offsets[P + 3]), "alt": int(offsets[P + 4]), "sort_err": int(offsets[P + 1]),
        "ranges": _slice(img, lib.ibgs_img_offset(W, H, b"ranges"), np.uint32, gx * gy * 2),
        "color": outs[0].detach().cpu().numpy().view(np.uint32).copy(),
    }
    s["order"] = _slice(geom, go("order_alt" if s["alt"] == 1 else "order"), np.uint32, s["kept"])
    s["point_list"] = _slice(binning, lib.ibgs_binning_offset(R, W, H, b"point_list"), np.uint32, R) if R > 0 else np.zeros(0, np.uint32)
    return s


def _same(a, b, what):
    assert a["R"] == b["R"], (what, a["R"], b["R"])
    for k in ("rec", "clamped", "order", "point_list", "ranges", "color", "kept"):
        assert np.array_equal(a[k], b[k]), (what, k)


def _check(inp, hints=("hit", "miss", None), split=False):
    base = _front(inp, ride=False, hint=None, split=split)          # the synchronous path: standalone SH kernel, exact arena
    R = base["R"]
    assert R > 0
    for h in hints:
        prev = {"hit": R, "miss": 1, None: None}[h]
        ride = _front(inp, ride=True, hint=prev, split=split)
        alone = _front(inp, ride=False, hint=prev, split=split)
        _same(ride, alone, ("ride vs standalone", h))
        _same(ride, base, ("ride vs synchronous", h))
    return base


def _spread(inp, lo=0.35, hi=3.5, seed=11):
    """Moves every Gaussian along its ray from the camera by a factor in [lo, hi]: view depths then span several float exponents."""
    inp = dict(inp)
    c = np.asarray(inp["campos"], np.float32)
    f = np.random.default_rng(seed).uniform(lo, hi, size=(inp["means3D"].shape[0], 1)).astype(np.float32)
    inp["means3D"] = np.ascontiguousarray(c + (inp["means3D"] - c) * f).astype(np.float32)
    return inp


@pytest.mark.parametrize("name", ["C1", "trained", "spread"])
def test_overlap_is_bit_identical_to_the_standalone_sh_pass(name):
    if name == "C1":
        inp = syn.make_scene(**syn.CONFIGS["C1"])
    elif name == "trained":
        inp = syn.make_scene(200_003, 960, 540, sh_degree=3, seed=5, opacity="trained", anisotropy="plane", scale_sigma=1.0, cluster=0.3)
    else:
        inp = _spread(syn.make_scene(150_001, 640, 480, sh_degree=3, seed=6, opacity="trained"))
    base = _check(inp)
    if name == "spread":          # the premise: the top byte of the depth keys of the Gaussians that are sorted is not one value, so the top-byte pass moves keys
        top = base["depth_keys"][base["tiles"] > 0] >> 24
        assert len(np.unique(top)) > 1 and base["alt"] == 0


def test_overlap_c3():
    c = syn.CONFIGS["C3"]
    inp = syn.make_scene(c["P"], c["W"], c["H"], sh_degree=c["sh_degree"], seed=c["seed"])
    base = _check(inp, hints=("hit", "miss"))
    top = base["depth_keys"][base["tiles"] > 0] >> 24
    assert len(np.unique(top)) == 1 and base["alt"] == 1          # C3's constant top byte: the last pass moves nothing


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("split", [False, True])
def test_overlap_every_degree_and_layout(deg, split):
    inp = syn.make_scene(50_003, 320, 240, sh_degree=3, seed=20 + deg, opacity="trained")          # P not a multiple of 64: a partial last wave
    inp["sh_degree"] = deg          # (16 coefficients per row, the degree reads the first (deg + 1)^2)
    _check(inp, hints=("hit",), split=split)


@pytest.mark.parametrize("P", [1, 100, 4097])
def test_overlap_tiny(P):
    """Fewer SH waves than launches: some launches carry none, the hist launch still carries the note (R)."""
    inp = syn.make_scene(P, 160, 120, sh_degree=3, seed=30 + P)
    base = _front(inp, ride=False, hint=None)
    for h in (max(base["R"], 1), 1):
        _same(_front(inp, ride=True, hint=h), base, ("tiny", P, h))
