#!/usr/bin/env python3
"""Freezes the REFERENCE'S OWN answer for BASELINE config C1 into tests/golden/reference_c1.npz: the reference rasterizer's CUDA sources compiled
for the CPU (oracle/ref_cpu, oracle/reference.py; needs the reference checkout) run on the seeded inputs that make_oracle_snapshot.py freezes the
oracle on, with the same fields.  tests/test_oracle_snapshot.py::test_oracle_against_the_reference_snapshot compares the oracle with it.
Usage (repo root): python tests/golden/make_reference_snapshot.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference as ref  # noqa: E402
from tests.golden import make_oracle_snapshot as snap  # noqa: E402  (inputs + field list)


def snapshot(inp, g):
    f = ref.forward(inp)
    b = ref.backward(inp, f, g)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    out = {"num_rendered_aabb": np.int64(f["num_rendered"]), "color_crop": f["color"][(slice(None),) + snap.CROP],
           "n_contrib_crop": f["n_contrib"].reshape(H, W)[snap.CROP], "final_T_crop": f["final_T"].reshape(H, W)[snap.CROP],
           "radii_head": f["radii"][:snap.HEAD * 8], "color_sum": np.float64(f["color"].astype(np.float64).sum()),
           "color_abs_sum": np.float64(np.abs(f["color"]).astype(np.float64).sum())}
    for k in ("dL_dmeans3D", "dL_dsh", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D"):
        a = np.asarray(b[k], np.float32).reshape(P, -1)
        out[k + "_head"] = a[:snap.HEAD].copy()
        out[k + "_abs_sum"] = np.float64(np.abs(a).astype(np.float64).sum())
        out[k + "_sum"] = np.float64(a.astype(np.float64).sum())
    return out


if __name__ == "__main__":
    inp, g = snap.build()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "reference_c1.npz"), **snapshot(inp, g))
    print("wrote tests/golden/reference_c1.npz")
