"""The tile-wave colour backward with its moments summed through LDS (render_bwd_color_kernel / _noabs_kernel on a black background in
float-atomic mode: render_bwd.hip `lds_red`, wave_reduce.h `wave_lds_reduce12`) against the oracle.

That path is taken by a wave when the background is black and the launch accumulates with float atomics; any other background, and the
deterministic mode, keep the float4 layout of the per-pixel constants and the butterfly.  Both sides of that wave-uniform choice are run here on
the same scenes, in atomic mode: black (the LDS reducer) and white (the butterfly beside it in the same kernel, with the background term), each
against the oracle's gradients for that background, with and without means2D_abs requiring a gradient (the two kernels).  Scenes: C1 with tile
waves forced (below 768 tiles the library would pick quadrant waves, whose kernel has no LDS reducer) and a 1080p frame (8 160 tiles: tile waves by
default, a ragged last tile row).  Bars and helpers are tests/test_gpu_parity.py's, unchanged."""
import functools

import numpy as np
import pytest

import oracle
from ibgs_amd import rasterizer, synthetic as syn
from tests.scenes import scene
from tests.test_gpu_background import BLACK, WHITE, hip_pass, library_flags, with_bg
from tests.test_gpu_hybrid import SPLIT
from tests.test_gpu_parity import GRAD_TOL, check_grads, rnd

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def get_scene(name):
    """(oracle-style inputs on black, upstream colour gradient, WAVE_SHAPE to force)."""
    if name == "C1":
        c = syn.CONFIGS["C1"]
        inp = syn.make_scene(c["P"], c["W"], c["H"], sh_degree=c["sh_degree"], seed=c["seed"])
        return inp, {"color": rnd((3, c["H"], c["W"]), 2)}, "tile"
    if name == "1080p":
        inp = scene(P=60000, W=1920, H=1080, deg=1, seed=81, opacity="trained", scale_mul=0.25)
        return inp, {"color": rnd((3, 1080, 1920), 6)}, None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_at(name, b):
    inp, g, _ = get_scene(name)
    inp = with_bg(inp, b)
    r = oracle.forward(inp, tex_quant=rasterizer.TEX_QUANT, cull=True)
    return r, oracle.backward(inp, r, g["color"], None, None, None, tex_quant=rasterizer.TEX_QUANT)


@pytest.mark.parametrize("abs_grad", [True, False], ids=["abs", "noabs"])
@pytest.mark.parametrize("b", [BLACK, WHITE], ids=["black", "white"])
@pytest.mark.parametrize("name", ["C1", "1080p"])
def test_tile_wave_colour_backward_in_atomic_mode(name, b, abs_grad):
    inp0, grads, shape = get_scene(name)
    inp = with_bg(inp0, b)
    ref, gb = oracle_at(name, b)
    with library_flags(shape, det=False):
        h = hip_pass(inp, grads, abs_grad)
    # the tile-wave kernels ran: one forward wave per tile, a launch order that holds every tile once, none of them split into quadrant waves
    assert h.meta[10] == 1, h.meta[10]
    tiles = h.order[h.order != 0xFFFFFFFF]
    assert np.array_equal(np.sort(tiles & ~np.uint32(SPLIT)), np.arange(h.nt, dtype=np.uint32)) and not (tiles & SPLIT).any()
    assert h.ist["R"] == ref["num_rendered"] and np.array_equal(h.o["radii"], ref["radii"])
    if name == "C1":
        assert (ref["ranges"][:, 1] - ref["ranges"][:, 0]).max() > 256          # lists of many 16-entry rounds
    if not abs_grad:
        assert "means2D_abs" not in h.g
    assert np.abs(gb["dL_dmeans2D"]).max() > 0 and np.abs(gb["dL_dsh"]).max() > 0
    check_grads(h.leaves, gb, tol=GRAD_TOL, skip=() if abs_grad else ("means2D_abs",))
    if b == WHITE:          # the two backgrounds are different problems: the white oracle is no stand-in for the black one
        gb0 = oracle_at(name, BLACK)[1]
        assert np.linalg.norm(gb["dL_dopacity"].astype(np.float64) - gb0["dL_dopacity"]) > 10 * GRAD_TOL * np.linalg.norm(gb["dL_dopacity"])
