"""Generates tests/golden/hghalf.npz IN THE BUILD CONTAINER, where the reference is present (as make_hourglass_fixture.py does): the reference's own
`ConvDecoderAE(38)` (color_aggregation_network.py, imported read-only through _ref_import's path) with the state dict recorded in hourglass.npz, run on the
CPU under torch.autocast(float16) -- how the reference's render.py runs it at test time -- on the two inputs of hourglass.npz (16 x 24 and 13 x 19).
Recorded: the two residuals as the network returns them (binary16), nothing else.

The fixture is data only; nothing of the reference is copied.  Re-run:  python tests/golden/make_hghalf_fixture.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import as ri  # noqa: E402

sys.path.insert(0, ri.REF)
from color_aggregation_network import ConvDecoderAE  # noqa: E402

z = np.load(os.path.join(HERE, "hourglass.npz"))
net = ConvDecoderAE(38)
net.load_state_dict({k[len("sd/conv_decoder."):]: torch.tensor(z[k]) for k in z.files if k.startswith("sd/conv_decoder.")})
out = {}
with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
    for tag, key in (("residual", "cnn_input"), ("odd_residual", "odd_cnn_input")):
        y = net(torch.tensor(z[key]))
        assert y.dtype == torch.float16 and tuple(y.shape) == (1, 3) + z[key].shape[-2:]
        out[tag] = y[0].numpy()

path = os.path.join(HERE, "hghalf.npz")
np.savez_compressed(path, **out)
print("hghalf.npz written:", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 16 << 10
