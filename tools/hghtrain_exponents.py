"""The table behind IBGS_HGHT_E_TARGET (include/ibgs_hg_half_train.h; DESIGN.md section 15, "Half-precision training"): per pre-activation gradient of the
hourglass's backward, the exponents floor(log2 .) of its largest and of its smallest non-zero magnitude RELATIVE to the upstream's largest, over the test
networks -- both parameter sets of tests/test_gpu_hourglass.py and the recorded reference state dict (tests/golden/hourglass.npz) -- on every frame of
tests/test_hourglass_train_host.py.  Float64 on the CPU (tests/hghalf_bwd_ref.backward_decided with the float64 forward's decisions); no GPU.

    python tools/hghtrain_exponents.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import hghalf_bwd_ref as hbref  # noqa: E402
from tests import hourglass_ref as ref  # noqa: E402
from tests import test_gpu_hourglass as fwd  # noqa: E402
from tests import test_hourglass_train_host as host  # noqa: E402


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "hourglass.npz"))
    recorded = {name + s: z["sd/conv_decoder.%s.%s" % (theirs, t)] for name, theirs in ref.REFERENCE_NAMES.items() for s, t in (("_w", "weight"), ("_b", "bias"))}
    nets = [(kind, fwd._params(kind)) for kind in host.KINDS] + [("recorded", recorded)]
    frames = host.FRAMES + [f for f in host.wgrad_frames() if f not in host.FRAMES]
    order = ("gS", "f", "d1", "u1", "d2", "u2", "b", "e2", "e1")
    print("%-10s %s" % ("network", "  ".join("%-9s" % ("G_" + n if n != "gS" else n) for n in order)) + "   (hi / lo: floor(log2 max), floor(log2 min non-zero), relative to floor(log2 max |g|))")
    hi_all, lo_all = -999, 999
    for kind, p in nets:
        hi, lo = {n: -999 for n in order}, {n: 999 for n in order}
        for h, w in frames:
            x = ref.seeded_input(1000 * h + w, h, w)
            g = np.random.default_rng(1000 * h + w + 7)
            g_res, g_ip = g.standard_normal((3, h, w)).astype(np.float32), g.standard_normal((3, h, w)).astype(np.float32)
            stages = ref.forward_ref(x, p)
            G = hbref.backward_decided(x, p, stages, hbref.decisions_of(stages), stages, g_res, g_ip, 0.75)["_G"]
            e0 = int(np.floor(np.log2(np.abs(G["gS"]).max())))
            for n in order:
                a = np.abs(G[n])
                a = a[a > 0]
                if a.size:
                    hi[n], lo[n] = max(hi[n], int(np.floor(np.log2(a.max()))) - e0), min(lo[n], int(np.floor(np.log2(a.min()))) - e0)
        print("%-10s %s" % (kind, "  ".join("%+3d / %+3d" % (hi[n], lo[n]) for n in order)))
        hi_all, lo_all = max(hi_all, max(hi.values())), min(lo_all, min(lo.values()))
    e = hbref.E_TARGET
    print("with E_TARGET = %d the largest gradient sits at 2^%d (binary16 overflows at 2^16) and the smallest non-zero one at 2^%d (binary16's normals end at 2^-14, its subnormals at 2^-24)"
          % (e, e + hi_all, e + lo_all))


if __name__ == "__main__":
    main()
