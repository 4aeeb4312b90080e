#!/usr/bin/env python3
"""Records what the REFERENCE'S OWN CODE computes on the four cases of tests/reference_cases.FIXTURES into tests/golden/reference_<case>.npz: its CUDA sources
compiled for the CPU (oracle/ref_cpu, oracle/reference.py; needs the reference checkout).  tests/test_gpu_reference_pins.py holds the HIP kernels to these
numbers; it reads the committed files only.

Per file: the case's name, its scene and upstream-gradient seeds and the sha1 of its regenerated inputs and upstream gradients (tests/reference_cases.checksum), the upstream gradients (float16: the
values are drawn on that grid), every public output (live source planes only), the preprocess record and the internal integer state, the ten gradients of the
first-to-last run, `d_order` per gradient (relative L2 between the first-to-last and the last-to-first run), the float64 oracle's gradients (`f64_*`, the
arbiter's column for ill-conditioned arrays) and `flips_*`: on how many pixels the reference's plain and fma builds take different decisions.
Usage (repo root): python tests/golden/make_reference_fixtures.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from oracle import reference as ref  # noqa: E402
from tests import reference_cases as rc  # noqa: E402
from tests.metrics import rel_l2  # noqa: E402

TEN = ("dL_dmeans3D", "dL_dmeans2D", "dL_dmeans2D_abs", "dL_dcolors", "dL_dall_map", "dL_dopacity", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
F64 = ("dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")          # the outputs of the per-Gaussian chain: the ones that can be ill-conditioned


def terminated(v):
    v = np.asarray(v).reshape(5, -1).copy()
    v[np.cumsum(v == -1, axis=0) > 0] = -1
    return v


def record(name):
    inp, g, q = rc.fixture_case(name); ga = rc.grad_args(g)
    n = int(inp["n_src"]) if inp.get("render_geo") else 0
    f = ref.forward(inp, tex_quant=q); ff = ref.forward(inp, tex_quant=q, fma=True)
    b = ref.backward(inp, f, *ga, tex_quant=q); brev = ref.backward(inp, f, *ga, tex_quant=q, reverse_blocks=True)
    with oracle.variant("f64"):
        b64 = oracle.backward(inp, oracle.forward(inp, tex_quant=q, cull=False), *ga, tex_quant=q)
    out = {"case": np.asarray(name), "checksum": np.asarray(rc.checksum(inp, g)), "tex_quant": np.asarray(bool(q)), "num_rendered": np.int64(f["num_rendered"]),
           "scene_seed": np.int64(rc.FIXTURES[name]["scene_seed"]), "upstream_seed": np.int64(rc.FIXTURES[name]["upstream_seed"])}
    for k, v in g.items():
        v = v[:3 * n] if k == "warped_image" else v
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
        out["g_" + k] = v.astype(np.float16)
    out["color"] = f["color"]; out["final_T"] = f["final_T"]; out["n_contrib"] = f["n_contrib"]
    for k in ("radii", "tiles_touched", "clamped", "point_list", "ranges", "means2D", "depths", "cov3D", "conic_opacity"):
        out[k] = f[k]
    out["tile_keys"] = (f["keys"] >> np.uint64(32)).astype(np.uint32)
    if n:
        for k in ("normal_map", "median_depth", "min_depth_diff", "camera_ray", "cache_sum_w", "cache_low", "cache_high"):
            out[k] = f[k]
        out["cam_feat"] = f["cam_feat"][:4 * n]; out["warped_image"] = f["warped_image"][:3 * n]
        out["use_first_src_frame_mask"] = f["use_first_src_frame_mask"].astype(np.uint8)
        out["valid_src_idx"] = terminated(f["valid_src_idx"]).astype(np.int8); out["valid_src_w"] = f["valid_src_w"][:n]
    for k in TEN:
        a = np.asarray(b[k], np.float32)
        if a.size and np.abs(a).max() > 0:
            out[k] = a
            out["d_order_" + k] = np.float64(rel_l2(brev[k], a))
            if k in F64:
                out["f64_" + k] = np.asarray(b64[k], np.float64).reshape(a.shape).astype(np.float32)
                out["f64_dist_" + k] = np.float64(rel_l2(a, np.asarray(b64[k], np.float64).reshape(a.shape)))          # the reference's own distance, from the unrounded column
    same_lists = f["num_rendered"] == ff["num_rendered"] and np.array_equal(f["point_list"], ff["point_list"])
    out["flips_lists"] = np.int64(0 if same_lists else 1)
    out["flips_n_contrib"] = np.int64((f["n_contrib"] != ff["n_contrib"]).sum()) if same_lists else np.int64(-1)
    if n:
        out["flips_valid"] = np.int64((terminated(f["valid_src_idx"]) != terminated(ff["valid_src_idx"])).any(axis=0).sum())
        out["flips_median"] = np.int64(((f["cache_low"] != ff["cache_low"]) | (f["cache_high"] != ff["cache_high"])).sum())
    return out


if __name__ == "__main__":
    for name in rc.FIXTURES:
        path = os.path.join(ROOT, "tests", "golden", "reference_%s.npz" % name)
        r = record(name)
        np.savez_compressed(path, **r)
        print("wrote %s: %d bytes, R = %d, flips %s" % (os.path.relpath(path, ROOT), os.path.getsize(path), int(r["num_rendered"]),
                                                      {k: int(v) for k, v in r.items() if k.startswith("flips_")}))
        print("   d_order", {k[8:]: float("%.2e" % v) for k, v in r.items() if k.startswith("d_order_")})
        assert os.path.getsize(path) <= 634660, "fixture larger than the largest file under tests/golden/"
