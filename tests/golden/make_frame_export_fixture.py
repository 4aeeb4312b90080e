"""Generates tests/golden/frame_export.npz IN THE BUILD CONTAINER, where the reference is present (as make_coloragg_fixture.py does): six small depth maps go
through the reference's own `colorize` (/root/reference/utils/general_utils.py:153-184, imported read-only) with cmap='magma_r', as render.py:231 calls it.
matplotlib 3.9 removed `mpl.cm.get_cmap`, which that function calls: it is shimmed here to `mpl.colormaps[name]`, the same table.

Recorded: each map, the (H, W, 3) uint8 image the reference returned for it, the 256-entry table of the colour map, and the numpy and matplotlib versions.
The fixture is data only; nothing of the reference is copied.  Re-run:  python tests/golden/make_frame_export_fixture.py
"""
import os
import sys

import matplotlib as mpl
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

if not hasattr(mpl.cm, "get_cmap"):
    mpl.cm.get_cmap = lambda name: mpl.colormaps[name]

from utils.general_utils import colorize  # noqa: E402

rng = np.random.default_rng(20)


def depth(h, w):
    return rng.gamma(2.0, 1.5, (1, h, w)).astype(np.float32)


maps = {"m5x7": depth(5, 7), "m33x65": depth(33, 65), "m17x300_block": depth(17, 300), "m64x48_zero_rows": depth(64, 48), "m2x2": depth(2, 2),
        "m40x40_constant": np.full((1, 40, 40), 2.5, np.float32)}
maps["m17x300_block"][0, 4:10, 100:136] = -99.0
maps["m64x48_zero_rows"][0, 20:30, :] = 0.0          # 480 of 3072 values tie at 0: the 2nd percentile lies inside the run

out = {"names": np.array(sorted(maps)), "numpy_version": np.array(np.__version__), "matplotlib_version": np.array(mpl.__version__),
       "lut": (mpl.colormaps["magma_r"](np.arange(256))[:, :3] * 255).astype(np.uint8)}
for name, m in maps.items():
    img = colorize(m.copy(), cmap="magma_r")[:, :, :3]
    assert img.dtype == np.uint8 and img.shape == m.shape[1:] + (3,)
    out["in_" + name] = m
    out["out_" + name] = np.ascontiguousarray(img)
path = os.path.join(HERE, "frame_export.npz")
np.savez_compressed(path, **out)
print("frame_export.npz written:", {k: v.shape for k, v in maps.items()}, "bytes", os.path.getsize(path))
assert os.path.getsize(path) < 200 * 1024
