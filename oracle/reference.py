"""The reference rasterizer's own CUDA sources, compiled for the CPU -- TEST INFRASTRUCTURE ONLY (``ibgs_amd`` never imports this).

ctypes front end over ``oracle/_ref/libibgs_ref_cpu.so`` (built by ``oracle/ref_cpu/build.py`` from the reference checkout; see
``oracle/ref_cpu/shim/refcpu.h`` for what the CPU execution model decides).  ``forward``, ``backward``, ``preprocess_backward`` and
``mark_visible`` take and return the dictionaries of the functions of the same names in ``oracle``, so a test calls either side with one
``inp``.  Options: ``tex_quant`` (linear-filter weights in the documented 1.8 fixed point), ``fma`` (the build in which the compiler may
contract a*b+c), ``reverse_blocks`` (every launch visits its blocks last to first: a second order of the float atomicAdd sums).
The stage functions (``stage_preprocess``, ``stage_render_forward``, ``stage_render_backward``, ``preprocess_backward``) run one stage of the
reference on state the caller supplies -- its own or the oracle's.
"""
import ctypes

import numpy as np

from .ref_cpu import build as _recipe

MAX_SRC = 5
_libs = {}
_F = np.float32


def available():
    """True where the library is there or can be built (a reference checkout is present)."""
    return _recipe.available() or _recipe.reference_root() is not None


def why_unavailable():
    return "oracle/_ref/libibgs_ref_cpu.so is absent and there is no reference checkout to build it from (oracle/ref_cpu/build.py)"


def lib(fma=False):
    if fma not in _libs:
        if _recipe.build() is None:
            raise RuntimeError(why_unavailable())
        L = ctypes.CDLL(_recipe.SO_FMA if fma else _recipe.SO)
        L.ref_forward.restype = ctypes.c_void_p
        _libs[fma] = L
    return _libs[fma]


def _p(a):
    if a is None:
        return ctypes.c_void_p(0)
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


def _f(a):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dtype=_F))
    return a if a.size else None


_ci = lambda x: ctypes.c_int(int(x))
_cf = lambda x: ctypes.c_float(float(x))


def mark_visible(means3D, viewmatrix, projmatrix=None, fma=False):
    means3D = np.ascontiguousarray(np.asarray(means3D, dtype=_F)).reshape(-1, 3); P = means3D.shape[0]
    out = np.zeros(P, np.uint8)
    if P == 0:
        return out.astype(bool)
    pm = _f(projmatrix) if projmatrix is not None else np.eye(4, dtype=_F)          # the test reads the view matrix alone; the projection must only be finite
    lib(fma).ref_mark_visible(_ci(P), _p(means3D), _p(_f(viewmatrix).reshape(-1)), _p(pm.reshape(-1)), _p(out))
    return out.astype(bool)


def _common(inp):
    c = {}
    c["means3D"] = np.ascontiguousarray(np.asarray(inp["means3D"], dtype=_F)).reshape(-1, 3); c["P"] = c["means3D"].shape[0]
    c["W"], c["H"] = int(inp["W"]), int(inp["H"])
    for k in ("shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "all_map"):
        c[k] = _f(inp.get(k))
    c["opac"] = np.ascontiguousarray(np.asarray(inp["opacities"], dtype=_F)).reshape(-1)
    c["vm"] = _f(inp["viewmatrix"]).reshape(-1); c["pm"] = _f(inp["projmatrix"]).reshape(-1)
    c["campos"] = _f(inp["campos"]).reshape(-1); c["bg"] = _f(inp["bg"]).reshape(-1)
    c["D"] = int(inp.get("sh_degree", 0)); c["M"] = 0 if c["shs"] is None else int(c["shs"].shape[1])
    c["mod"] = float(inp.get("scale_modifier", 1.0)); c["tanx"], c["tany"] = float(inp["tanfovx"]), float(inp["tanfovy"])
    c["geo"] = bool(inp.get("render_geo", False)); c["depth_only"] = bool(inp.get("render_depth_only", False))
    n = c["n_src"] = int(inp.get("n_src", 1)); c["L"] = int(inp.get("buffer_length", 4)); c["thr"] = float(inp.get("depth_thr", 0.01))
    H, W = c["H"], c["W"]
    c["r2s"] = _f(inp.get("ref_to_src")); c["scp"] = _f(inp.get("src_cam_pos")); c["img"] = _f(inp.get("src_images")); c["dep"] = _f(inp.get("src_depths"))
    if c["r2s"] is None: c["r2s"] = np.zeros((n, 16), _F)
    if c["scp"] is None: c["scp"] = np.zeros((n, 3), _F)
    if c["img"] is None: c["img"] = np.zeros((n, 3, H, W), _F)
    if c["dep"] is None: c["dep"] = np.zeros((n, 1, H, W), _F)
    if c["all_map"] is None: c["all_map"] = np.zeros((c["P"], 5), _F)          # the reference's front end always passes the tensor
    return c


def _outputs(H, W):
    return {"color": np.zeros((3, H, W), _F), "normal_map": np.zeros((3, H, W), _F), "median_depth": np.zeros((1, H, W), _F),
            "cam_feat": np.zeros((4 * MAX_SRC, H, W), _F), "warped_image": np.zeros((3 * MAX_SRC, H, W), _F),
            "min_depth_diff": np.zeros((1, H, W), _F), "camera_ray": np.zeros((3, H, W), _F),
            "use_first_src_frame_mask": np.zeros((1, H, W), np.int32)}


def _image_state(H, W):
    HW = H * W
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return {"ranges": np.zeros((gx * gy, 2), np.uint32), "final_T": np.zeros(HW, _F), "n_contrib": np.zeros(HW, np.uint32),
            "cache_sum_w": np.zeros(HW, _F), "cache_low": np.zeros(HW, np.uint32), "cache_high": np.zeros(HW, np.uint32),
            "valid_src_idx": np.zeros((MAX_SRC, HW), np.int32), "valid_src_w": np.zeros((MAX_SRC, HW), _F)}


def _geom_state(P):
    return {"radii": np.zeros(P, np.int32), "means2D": np.zeros((P, 2), _F), "depths": np.zeros(P, _F), "cov3D": np.zeros((P, 6), _F),
            "rgb": np.zeros((P, 3), _F), "conic_opacity": np.zeros((P, 4), _F), "tiles_touched": np.zeros(P, np.uint32),
            "clamped": np.zeros((P, 3), np.uint8)}


def forward(inp, tex_quant=False, fma=False, reverse_blocks=False):
    """The whole forward through CudaRasterizer::Rasterizer::forward.  Returns ``oracle.forward``'s dictionary (public outputs, every internal
    array, ``num_rendered``); ``keys`` / ``point_list`` are the sorted lists, ``keys_unsorted`` / ``point_list_unsorted`` the emitted ones."""
    c = _common(inp); P, H, W = c["P"], c["H"], c["W"]
    out = _outputs(H, W); st = _geom_state(P); st.update(_image_state(H, W))
    if c["geo"] is False:
        st["valid_src_idx"][:] = -1          # (never written on the colour path; oracle.forward's convention)
    if P == 0:   # the reference's front end does not call the rasterizer
        st["point_list"] = np.zeros(0, np.uint32); st["keys"] = np.zeros(0, np.uint64)
        st["valid_src_idx"][:] = -1
        out.update(st); out["num_rendered"] = 0
        return out
    L = lib(fma)
    R = ctypes.c_int(0)
    h = L.ref_forward(_ci(P), _ci(c["D"]), _ci(c["M"]), _p(c["bg"]), _ci(W), _ci(H), _p(c["means3D"]), _p(c["shs"]), _p(c["colors_precomp"]),
                      _p(c["opac"]), _p(c["scales"]), _cf(c["mod"]), _p(c["rotations"]), _p(c["cov3D_precomp"]), _p(c["all_map"]), _p(c["vm"]),
                      _p(c["pm"]), _p(c["r2s"]), _p(c["scp"]), _p(c["img"]), _p(c["dep"]), _ci(c["n_src"]), _ci(c["L"]), _cf(c["thr"]),
                      _p(c["campos"]), _cf(c["tanx"]), _cf(c["tany"]), _p(out["color"]), _p(st["radii"]), _p(out["normal_map"]),
                      _p(out["median_depth"]), _p(out["cam_feat"]), _p(out["warped_image"]), _p(out["min_depth_diff"]), _p(out["camera_ray"]),
                      _p(out["use_first_src_frame_mask"]), _ci(c["geo"]), _ci(c["depth_only"]), _ci(tex_quant), _ci(reverse_blocks), ctypes.byref(R))
    h = ctypes.c_void_p(h)
    try:
        R = R.value
        st["keys"] = np.zeros(R, np.uint64); st["point_list"] = np.zeros(R, np.uint32)
        st["keys_unsorted"] = np.zeros(R, np.uint64); st["point_list_unsorted"] = np.zeros(R, np.uint32)
        st["point_offsets"] = np.zeros(P, np.uint32)
        vi = st["valid_src_idx"] if c["geo"] else np.zeros_like(st["valid_src_idx"])
        L.ref_state(h, _p(st["means2D"]), _p(st["depths"]), _p(st["cov3D"]), _p(st["rgb"]), _p(st["conic_opacity"]), _p(st["tiles_touched"]),
                    _p(st["clamped"]), _p(st["point_offsets"]), _p(st["keys"]), _p(st["point_list"]), _p(st["keys_unsorted"]),
                    _p(st["point_list_unsorted"]), _p(st["ranges"]), _p(st["final_T"]), _p(st["n_contrib"]), _p(st["cache_sum_w"]),
                    _p(st["cache_low"]), _p(st["cache_high"]), _p(vi), _p(st["valid_src_w"]))
    finally:
        L.ref_free(h)
    out.update(st)
    out["num_rendered"] = R
    return out


def stage_preprocess(inp, fma=False):
    """FORWARD::preprocess alone: radii, means2D, depths, cov3D, rgb, conic_opacity, tiles_touched, clamped."""
    c = _common(inp); P = c["P"]
    st = _geom_state(P)
    if P:
        lib(fma).ref_stage_preprocess(_ci(P), _ci(c["D"]), _ci(c["M"]), _p(c["means3D"]), _p(c["scales"]), _cf(c["mod"]), _p(c["rotations"]), _p(c["opac"]),
                                      _p(c["shs"]), _p(c["cov3D_precomp"]), _p(c["colors_precomp"]), _p(c["vm"]), _p(c["pm"]), _p(c["campos"]),
                                      _ci(c["W"]), _ci(c["H"]), _cf(c["tanx"]), _cf(c["tany"]), _ci(c["depth_only"]), _p(st["radii"]), _p(st["means2D"]),
                                      _p(st["depths"]), _p(st["cov3D"]), _p(st["rgb"]), _p(st["conic_opacity"]), _p(st["tiles_touched"]), _p(st["clamped"]))
    return st


def stage_render_forward(inp, fwd, tex_quant=False, fma=False):
    """FORWARD::render on the lists and per-Gaussian state of ``fwd`` (a forward result of either side): the public outputs and the image state."""
    c = _common(inp); H, W = c["H"], c["W"]
    out = _outputs(H, W); st = _image_state(H, W)
    if not c["geo"]:
        st["valid_src_idx"][:] = -1
    vi = st["valid_src_idx"] if c["geo"] else np.zeros_like(st["valid_src_idx"])
    feats = c["colors_precomp"] if c["colors_precomp"] is not None else np.ascontiguousarray(fwd["rgb"], dtype=_F)
    ranges = np.ascontiguousarray(fwd["ranges"], dtype=np.uint32); pl = np.ascontiguousarray(fwd["point_list"], dtype=np.uint32)
    m2 = np.ascontiguousarray(fwd["means2D"], dtype=_F); co = np.ascontiguousarray(fwd["conic_opacity"], dtype=_F)
    lib(fma).ref_stage_render_forward(_ci(W), _ci(H), _p(ranges), _p(pl), _p(m2), _p(feats), _p(c["all_map"]), _p(co), _p(c["vm"]), _p(c["campos"]),
                                      _p(c["bg"]), _cf(c["tanx"]), _cf(c["tany"]), _ci(c["n_src"]), _p(c["r2s"]), _p(c["scp"]), _p(c["img"]), _p(c["dep"]),
                                      _ci(c["L"]), _cf(c["thr"]), _ci(c["geo"]), _ci(c["depth_only"]), _ci(tex_quant), _p(st["final_T"]),
                                      _p(st["n_contrib"]), _p(st["cache_sum_w"]), _p(st["cache_low"]), _p(st["cache_high"]), _p(vi),
                                      _p(st["valid_src_w"]), _p(out["color"]), _p(out["normal_map"]), _p(out["median_depth"]), _p(out["cam_feat"]),
                                      _p(out["warped_image"]), _p(out["min_depth_diff"]), _p(out["camera_ray"]), _p(out["use_first_src_frame_mask"]))
    st["ranges"] = ranges
    out.update(st)
    return out


def _upstream(H, W, dL_dcolor, dL_dnormal, dL_ddepth, dL_dwarped):
    z = lambda a, shape: np.zeros(shape, _F) if a is None or np.asarray(a).size == 0 else np.ascontiguousarray(np.asarray(a, dtype=_F))
    return z(dL_dcolor, (3, H, W)), z(dL_dnormal, (3, H, W)), z(dL_ddepth, (1, H, W)), z(dL_dwarped, (3 * MAX_SRC, H, W))


def stage_render_backward(inp, fwd, dL_dcolor, dL_dnormal=None, dL_ddepth=None, dL_dwarped=None, tex_quant=False, fma=False, reverse_blocks=False):
    """BACKWARD::render on the state and outputs of ``fwd`` (either side's forward): the six float-atomicAdd sums, in this run's block order."""
    c = _common(inp); P, H, W = c["P"], c["H"], c["W"]
    g_c, g_n, g_d, g_w = _upstream(H, W, dL_dcolor, dL_dnormal, dL_ddepth, dL_dwarped)
    res = {"dL_dmeans2D": np.zeros((P, 3), _F), "dL_dmeans2D_abs": np.zeros((P, 3), _F), "dL_dconic": np.zeros((P, 4), _F),
           "dL_dopacity": np.zeros((P, 1), _F), "dL_dcolors": np.zeros((P, 3), _F), "dL_dall_map": np.zeros((P, 5), _F)}
    if P == 0:
        return res
    a = lambda k, t: np.ascontiguousarray(np.asarray(fwd[k]), dtype=t)
    feats = c["colors_precomp"] if c["colors_precomp"] is not None else a("rgb", _F)
    keep = [a("ranges", np.uint32), a("point_list", np.uint32), a("means2D", _F), a("conic_opacity", _F), a("normal_map", _F), a("median_depth", _F),
            a("warped_image", _F), a("final_T", _F), a("n_contrib", np.uint32), a("cache_sum_w", _F).copy(), a("cache_low", np.uint32).copy(),
            a("cache_high", np.uint32).copy(), a("valid_src_idx", np.int32).copy(), a("valid_src_w", _F).copy()]
    lib(fma).ref_stage_render_backward(_ci(W), _ci(H), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), _p(feats), _p(c["all_map"]), _p(c["bg"]),
                                       _cf(c["tanx"]), _cf(c["tany"]), _ci(c["n_src"]), _p(c["r2s"]), _p(c["scp"]), _p(c["img"]), _p(c["dep"]),
                                       _p(keep[4]), _p(keep[5]), _p(keep[6]), _p(keep[7]), _p(keep[8]), _p(keep[9]), _p(keep[10]), _p(keep[11]),
                                       _p(keep[12]), _p(keep[13]), _p(g_c), _p(g_n), _p(g_d), _p(g_w), _ci(c["geo"]), _ci(tex_quant),
                                       _ci(reverse_blocks), _p(res["dL_dmeans2D"]), _p(res["dL_dmeans2D_abs"]), _p(res["dL_dconic"]),
                                       _p(res["dL_dopacity"]), _p(res["dL_dcolors"]), _p(res["dL_dall_map"]))
    return res


def preprocess_backward(inp, radii, clamped, cov3D, dL_dmean2D, dL_dconic, dL_dcolors, fma=False):
    """BACKWARD::preprocess alone on gradients the caller chooses (``oracle.preprocess_backward``'s arguments and result)."""
    c = _common(inp); P, M = c["P"], c["M"]
    res = {"dL_dmeans3D": np.zeros((P, 3), _F), "dL_dcov3D": np.zeros((P, 6), _F), "dL_dsh": np.zeros((P, M, 3), _F),
           "dL_dscales": np.zeros((P, 3), _F), "dL_drotations": np.zeros((P, 4), _F)}
    if P == 0:
        return res
    radii = np.ascontiguousarray(np.asarray(radii, np.int32)).reshape(P); clamped = np.ascontiguousarray(np.asarray(clamped, np.uint8)).reshape(P, 3)
    g2 = np.ascontiguousarray(np.asarray(dL_dmean2D, dtype=_F)).reshape(P, 3); gc = np.ascontiguousarray(np.asarray(dL_dconic, dtype=_F)).reshape(P, 4)
    gcol = np.ascontiguousarray(np.asarray(dL_dcolors, dtype=_F)).reshape(P, 3).copy(); cov = np.ascontiguousarray(np.asarray(cov3D, dtype=_F)).reshape(P, 6)
    lib(fma).ref_stage_preprocess_backward(_ci(P), _ci(c["D"]), _ci(M), _p(c["means3D"]), _p(radii), _p(c["shs"]), _p(clamped), _p(c["scales"]),
                                           _p(c["rotations"]), _cf(c["mod"]), _p(cov), _p(c["vm"]), _p(c["pm"]), _p(c["campos"]), _ci(c["W"]), _ci(c["H"]),
                                           _cf(c["tanx"]), _cf(c["tany"]), _p(g2), _p(gc), _p(gcol), _p(res["dL_dmeans3D"]), _p(res["dL_dcov3D"]),
                                           _p(res["dL_dsh"]), _p(res["dL_dscales"]), _p(res["dL_drotations"]))
    return res


def backward(inp, fwd, dL_dcolor, dL_dnormal=None, dL_ddepth=None, dL_dwarped=None, tex_quant=False, fma=False, reverse_blocks=False):
    """The whole backward through CudaRasterizer::Rasterizer::backward.  The reference keeps its forward state in the chunks of that call, so the
    forward is run again here (same options) and ``fwd`` supplies the outputs the backward reads.  Returns ``oracle.backward``'s dictionary."""
    c = _common(inp); P, H, W, M = c["P"], c["H"], c["W"], c["M"]
    g_c, g_n, g_d, g_w = _upstream(H, W, dL_dcolor, dL_dnormal, dL_ddepth, dL_dwarped)
    res = {"dL_dmeans3D": np.zeros((P, 3), _F), "dL_dmeans2D": np.zeros((P, 3), _F), "dL_dmeans2D_abs": np.zeros((P, 3), _F),
           "dL_dcolors": np.zeros((P, 3), _F), "dL_dall_map": np.zeros((P, 5), _F), "dL_dconic": np.zeros((P, 4), _F),
           "dL_dopacity": np.zeros((P, 1), _F), "dL_dcov3D": np.zeros((P, 6), _F), "dL_dsh": np.zeros((P, M, 3), _F),
           "dL_dscales": np.zeros((P, 3), _F), "dL_drotations": np.zeros((P, 4), _F)}
    if P == 0:
        return res
    L = lib(fma)
    out = _outputs(H, W); radii = np.zeros(P, np.int32); R = ctypes.c_int(0)
    h = L.ref_forward(_ci(P), _ci(c["D"]), _ci(M), _p(c["bg"]), _ci(W), _ci(H), _p(c["means3D"]), _p(c["shs"]), _p(c["colors_precomp"]),
                      _p(c["opac"]), _p(c["scales"]), _cf(c["mod"]), _p(c["rotations"]), _p(c["cov3D_precomp"]), _p(c["all_map"]), _p(c["vm"]),
                      _p(c["pm"]), _p(c["r2s"]), _p(c["scp"]), _p(c["img"]), _p(c["dep"]), _ci(c["n_src"]), _ci(c["L"]), _cf(c["thr"]),
                      _p(c["campos"]), _cf(c["tanx"]), _cf(c["tany"]), _p(out["color"]), _p(radii), _p(out["normal_map"]),
                      _p(out["median_depth"]), _p(out["cam_feat"]), _p(out["warped_image"]), _p(out["min_depth_diff"]), _p(out["camera_ray"]),
                      _p(out["use_first_src_frame_mask"]), _ci(c["geo"]), _ci(c["depth_only"]), _ci(tex_quant), _ci(0), ctypes.byref(R))
    h = ctypes.c_void_p(h)
    try:
        L.ref_backward(h, _ci(c["D"]), _ci(M), _p(c["bg"]), _p(out["normal_map"]), _p(out["median_depth"]), _p(out["warped_image"]), _p(c["means3D"]),
                       _p(c["shs"]), _p(c["colors_precomp"]), _p(c["all_map"]), _p(c["scales"]), _cf(c["mod"]), _p(c["rotations"]),
                       _p(c["cov3D_precomp"]), _p(c["vm"]), _p(c["pm"]), _p(c["r2s"]), _p(c["scp"]), _p(c["img"]), _p(c["dep"]), _ci(c["n_src"]),
                       _p(c["campos"]), _cf(c["tanx"]), _cf(c["tany"]), _p(radii), _p(g_c), _p(g_n), _p(g_d), _p(g_w), _p(res["dL_dmeans2D"]),
                       _p(res["dL_dmeans2D_abs"]), _p(res["dL_dconic"]), _p(res["dL_dopacity"]), _p(res["dL_dcolors"]), _p(res["dL_dmeans3D"]),
                       _p(res["dL_dcov3D"]), _p(res["dL_dsh"]), _p(res["dL_dscales"]), _p(res["dL_drotations"]), _p(res["dL_dall_map"]),
                       _ci(c["geo"]), _ci(tex_quant), _ci(reverse_blocks))
    finally:
        L.ref_free(h)
    return res
