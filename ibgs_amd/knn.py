"""distCUDA2 replacement: mean squared distance to the 3 nearest neighbours,
used once by GaussianModel.create_from_pcd to initialise the scales (reference scene/gaussian_model.py:195,
submodules/simple-knn/spatial.cu:15-26)."""
import torch

from . import _device, _lib


def distCUDA2(points):
    lib = _lib.load()
    if points.ndimension() != 2 or points.size(1) != 3:
        raise RuntimeError("points must have dimensions (num_points, 3)")
    if not points.is_cuda:
        raise RuntimeError("points must live on a HIP device (libibgs_rast.so has no CPU path)")
    P = int(points.size(0))
    dev = points.device
    pts = points.detach().float().contiguous()
    out = torch.zeros(P, dtype=torch.float32, device=dev)
    if P:
        scratch = _device.scratch(dev, lib.ibgs_required_knn(P))
        _device.call(dev, "ibgs_knn_mean_dist2", P, pts.data_ptr(), out.data_ptr(), scratch.data_ptr(), scratch.numel())
    return out
