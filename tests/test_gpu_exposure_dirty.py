"""The exposure correction on dirty, guard-banded buffers (tests/dirty_alloc.py): every `torch.empty` / `torch.empty_like` of the
wrapper served from a block of 0x00, 0xFF and 0x40 bytes between two 4 KiB guards.  Every returned tensor and the gradient must have the same bits in all
runs, no NaN may appear, no guard byte may change, and at least as many allocations must have been intercepted as the wrapper makes for the call (counted
in its code: outputs + the arena; `_device.scratch` is one)."""
import pytest
import torch

from ibgs_amd import hourglass
from tests import dirty_alloc as da
from tests import test_gpu_exposure as expo

pytestmark = pytest.mark.gpu
DEV = "cuda"
CORRECT = 3 + 1          # corrected, affine, fit_ok; the partials' arena
CORRECT_BACKWARD = 1     # d render


@pytest.mark.parametrize("grey", [False, True], ids=["colourful", "near_grey"])
@pytest.mark.parametrize("frame", [(4, 4), (5, 7), (33, 65), (32, 48), "large"], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_exposure_correct_forward_and_backward(frame, grey):
    h, w = expo._large_frame() if frame == "large" else frame
    render, warped, mask, up = expo._case(h, w, 0.3, grey)["dev"]
    base = dict(da.check("exposure_correct %dx%d" % (h, w), lambda: expo._run(render, warped, mask, up), DEV, CORRECT + CORRECT_BACKWARD))
    assert sorted(base) == ["[0]", "[1]", "[2]", "[3]"] and int(base["[2]"]) == (1 if expo._case(h, w, 0.3, grey)["ok"] else 0)


def test_undetermined_fit():
    """The identity path writes every output too: the image is copied, the matrix and the status are stored."""
    render, warped, mask, up = expo._case(33, 65, 0.3, False)["dev"]
    base = dict(da.check("exposure_correct 33x65, empty mask", lambda: expo._run(render, warped, torch.zeros_like(mask), up), DEV, CORRECT + CORRECT_BACKWARD))
    assert int(base["[2]"]) == 0 and torch.equal(base["[0]"], render) and torch.equal(base["[3]"], up)


@pytest.mark.parametrize("precision", ["float32", "float16"])
def test_fuse_color_with_the_correction(precision):
    pkg, net = expo._package()
    assert tuple(pkg["render"].shape) == (3, 32, 48)

    def call():
        with torch.no_grad():
            out = hourglass.fuse_color(pkg, net, precision=precision, enable_exposure_correction=True)
        assert out.pop("burned_in_gauss") == 1.0          # (a float: the rest are tensors)
        return out
    # the correction; the front end: levels, its arena, cnn_input; the hourglass: residual, image_pred, its arena
    base = dict(da.check("fuse_color 32x48 %s, exposure correction" % precision, call, DEV, CORRECT + 3 + 3))
    assert int(base["['exposure_fit_ok']"]) == 1
