"""The seeded cases on which the reference's own code (oracle/reference.py: its CUDA sources compiled for the CPU) is compared with the oracle
(tests/test_reference_pins_oracle.py) and, recorded under tests/golden/ by make_reference_fixtures.py, with the HIP kernels
(tests/test_gpu_reference_pins.py).  Frames of 72 x 56: 5 x 4 tiles with a partial tile column and a partial tile row."""
import hashlib

import numpy as np

import oracle
from ibgs_amd import synthetic as syn
from tests import scenes

W, H = 72, 56


def with_camera(inp, cam):
    inp = dict(inp)
    inp.update(tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"], _cam=cam)
    if inp.get("all_map") is not None:
        inp["all_map"] = syn.plane_all_map(inp["means3D"], inp["scales"], inp["rotations"], cam)
    return inp


def color_case(active_deg, seed, bg=(0.0, 0.0, 0.0), P=1500, scale_mul=2.0, opacity="trained", w=W, h=H):
    """make_scene's cloud with 16 stored SH coefficients and `active_deg` <= 3 of them active."""
    inp = scenes.scene(P=P, W=w, H=h, deg=3, seed=seed, opacity=opacity, scale_mul=scale_mul)
    inp["sh_degree"] = active_deg
    inp["bg"] = np.asarray(bg, np.float32)
    return inp


def precomp_case(seed=23, P=1500):
    """colors_precomp + cov3D_precomp (the covariances the oracle derives from the scales and rotations at scale_modifier 0.7), fx != fy."""
    inp = color_case(3, seed, bg=(0.3, 0.1, 0.6), P=P)
    inp = with_camera(inp, scenes.camera_at(W, H, (0.4, -3.6, 1.5), (0.0, 0.0, 0.0), 0.75, 0.48))
    inp["scale_modifier"] = 0.7
    cov = oracle.forward(inp)["cov3D"].copy()
    rng = np.random.default_rng(seed)
    inp["colors_precomp"] = rng.uniform(0, 1, (inp["means3D"].shape[0], 3)).astype(np.float32)
    inp["cov3D_precomp"] = cov
    for k in ("shs", "scales", "rotations"):
        inp[k] = None
    inp["sh_degree"] = 0
    return inp


def geo_case(n_src, L, seed, P=1500, depth_thr=0.01, close=False, w=W, h=H):
    """scenes.surface_scene: opaque discs on a sphere and a ground square, `n_src` source views, median buffer of `L`.  close: the reference camera
    0.5 above the sphere's surface, the sources around it."""
    if close:
        eye = (0.0, -1.25, 0.35)
        poses = [((0.12 * np.cos(a), -1.25 + 0.05 * np.sin(a), 0.35 + 0.12 * np.sin(a)), (0.0, 0.0, 0.0)) for a in np.linspace(0.0, 2 * np.pi, n_src, endpoint=False)]
        return scenes.surface_scene(P=P, W=w, H=h, seed=seed, L=L, deg=2, depth_thr=depth_thr, ref_pose=(eye, (0.0, 0.0, 0.0)), src_poses=poses, fovx=0.9, fovy=0.75)
    return scenes.surface_scene(P=P, W=w, H=h, seed=seed, n_src=n_src, L=L, deg=2, depth_thr=depth_thr)


def upstream(inp, seed):
    """Upstream gradients of every differentiable output the case produces: color, and on the geo path normal_map, median_depth, warped_image."""
    rng = np.random.default_rng(seed)
    h, w = int(inp["H"]), int(inp["W"])
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float16).astype(np.float32)          # float16 values: a fixture stores them in half the bytes, exactly
    g = {"color": draw(3, h, w)}
    if inp.get("render_geo"):
        g["normal_map"] = draw(3, h, w)
        g["median_depth"] = draw(1, h, w)
        g["warped_image"] = draw(15, h, w)
        g["warped_image"][3 * int(inp["n_src"]):] = 0.0          # slots beyond the sources are never written
    return g


def grad_args(g):
    return (g["color"], g.get("normal_map"), g.get("median_depth"), g.get("warped_image"))


def checksum(inp, g):
    """sha1 over every array of the inputs and the upstream gradients (sorted by name; shapes and dtypes included)."""
    h = hashlib.sha1()
    items = {k: v for k, v in inp.items() if not k.startswith("_")}
    items.update({"g_" + k: v for k, v in g.items()})
    for k in sorted(items):
        v = items[k]
        if v is None:
            h.update(("%s=None;" % k).encode())
            continue
        a = np.ascontiguousarray(np.asarray(v))
        h.update(("%s:%s:%s;" % (k, a.dtype.str, a.shape)).encode()); h.update(a.tobytes())
    return h.hexdigest()


# the four recorded cases of tests/golden/reference_<name>.npz: the builder, the scene seed it passes on, the seed of the upstream gradients, the texture mode
# (sizes chosen so that a fixture stays below the largest file already under tests/golden/: 1000 Gaussians at 72 x 56 on the colour path -- 20 tiles of ~500
# entries --, 600 discs at 56 x 40 on the geo path -- 4 x 3 tiles, again with a partial column and row)
FIXTURES = {
    "sh3_white": {"build": lambda: color_case(3, 31, bg=(1.0, 1.0, 1.0), P=1000), "scene_seed": 31, "upstream_seed": 7000, "tex_quant": False},
    "precomp": {"build": lambda: precomp_case(seed=23, P=1000), "scene_seed": 23, "upstream_seed": 7001, "tex_quant": False},
    "geo3_L4": {"build": lambda: geo_case(3, 4, 7, P=600, w=56, h=40), "scene_seed": 7, "upstream_seed": 7002, "tex_quant": False},
    "geo5_L3_close": {"build": lambda: geo_case(5, 3, 9, P=600, close=True, w=56, h=40), "scene_seed": 9, "upstream_seed": 7003, "tex_quant": True},
}


def fixture_case(name):
    """(inputs, upstream gradients, tex_quant) of a recorded case: the one place its seeds are turned into arrays."""
    f = FIXTURES[name]
    inp = f["build"]()
    return inp, upstream(inp, f["upstream_seed"]), f["tex_quant"]
