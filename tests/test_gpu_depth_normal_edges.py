"""The fused depth -> normal kernels (ibgs_amd/csrc/depth_normal.hip) region by region: at the seams of the backward's 64 x 8 LDS tile, in its last partial
tiles, on the image border, on the rim of zero-depth holes (the clamp branch of F.normalize, `len <= 1e-12` in `dn_grad_edges`) and deep inside them.

Per class of pixels (tests/glue_edges.py) and for the normal map as for dL/ddepth:

    rel L2 (fused vs float64) <= max(K * rel L2 (torch fp32 on the device vs float64), 1e-6),     K = glue_edges.K_CLASS = 2.0,

the whole-image factor of tests/test_gpu_depth_normal.py applied to each class on its own; the floor is torch's evaluation, never the kernel's.  What is
exact is asked exactly: no normal on the one-pixel border, nothing at all where every pixel within two is a hole, everything finite -- the 1e18 gradients
on a hole's rim included, which the reference produces too (its 1e-12 and 1e-8 in the denominators) and which are compared with the same relative bar.

Measured on the MI355X (docs/EXPERIMENTS.md section 14): fused / torch between 0.36 and 1.30 in every class whose bar is K * floor and not the 1e-6
floor, so K stayed at 2.0."""
import numpy as np
import pytest
import torch

from ibgs_amd.depthnormal import depth_normal
from tests import glue_edges as ge

pytestmark = pytest.mark.gpu


def _run(case, lattice=False):
    r = ge.reference(case, lattice)
    floor = ge.evaluate(ge.torch_glue, r.cam, r.depth, r.cot, torch.float32, "cuda")
    fused = ge.evaluate(depth_normal, r.cam, r.depth, r.cot, torch.float32, "cuda")
    return r, floor, fused


@pytest.mark.parametrize("case", list(ge.CASES))
def test_every_pixel_class_against_float64(case):
    r, floor, fused = _run(case)
    assert fused[0].shape == (3, r.H, r.W) and fused[1].shape == (r.H, r.W)
    assert ge.structural_zeros(*fused, r.masks) == []
    _, bad_n = ge.class_distances(case + " normal", fused[0], floor[0], r.n64, ge.normal_classes(r.masks))
    _, bad_g = ge.class_distances(case + " dL/ddepth", fused[1], floor[1], r.g64, ge.gradient_classes(r.masks, r.g64))
    assert bad_n == [] and bad_g == []


@pytest.mark.parametrize("case", ["197x29 holes", "197x29", "65x9"])
def test_gradient_support_of_a_lattice_cotangent(case):
    """A cotangent on the lattice v % 3 == 1, u % 3 == 1: each of its pixels feeds its four neighbours and nothing else, and no pixel hears from two."""
    r, floor, fused = _run(case, lattice=True)
    s = ge.lattice_support(r.W, r.H)
    assert np.isfinite(fused[1]).all()
    assert (fused[1][~s] == 0).all(), np.argwhere((fused[1] != 0) & ~s)[:8]
    _, bad = ge.class_distances(case + " lattice dL/ddepth", fused[1], floor[1], r.g64, ge.gradient_classes(r.masks, r.g64))
    assert bad == []


@pytest.mark.parametrize("case", ["197x29 holes", "65x9"])
def test_noncontiguous_cotangent_and_depth(case):
    r = ge.reference(case)
    dev = "cuda"
    d0 = r.depth.to(dev).requires_grad_(True)
    out0 = depth_normal(r.cam, d0)
    (out0 * r.cot.to(dev)).sum().backward()
    # the cotangent arrives as a permuted view: (H, W, 3) strides behind a (3, H, W) shape
    d1 = r.depth.to(dev).requires_grad_(True)
    out1 = depth_normal(r.cam, d1)
    (out1.permute(1, 2, 0) * r.cot.to(dev).permute(1, 2, 0).contiguous()).sum().backward()
    assert torch.equal(out1, out0) and torch.equal(d1.grad.view(torch.int32), d0.grad.view(torch.int32))
    # the depth is every other column of a wider map
    wide = torch.full((r.H, 2 * r.W), 123.0, device=dev)
    wide[:, ::2] = r.depth.to(dev)
    wide.requires_grad_(True)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    out2 = depth_normal(r.cam, view)
    (out2 * r.cot.to(dev)).sum().backward()
    assert torch.equal(out2.view(torch.int32), out0.view(torch.int32))
    assert torch.equal(wide.grad[:, ::2].contiguous().view(torch.int32), d0.grad.view(torch.int32)) and (wide.grad[:, 1::2] == 0).all()
