"""The image side of the reference's evaluation (metrics.py:75-98) on the device: SSIM, PSNR and LPIPS per test view, and their means.

`image_metrics` is one launch of the fused SSIM forward (csrc/ssim.hip, C ABI include/ibgs_ssim.h) with no per-pixel output: the same pass over the two
images that sums the SSIM map also sums (x - y)^2 and |x - y|, so SSIM, PSNR (utils/image_utils.py:18-20) and L1 of every image of a batch cost one read of
the batch.  `evaluate_images` stacks views of the same size into such launches and reads the numbers back once.

LPIPS, the third column of the reference's table, is computed when the caller hands over an `ibgs_amd.lpips.LPIPSNet` (the keyword `lpips_net`): the
network runs on this library's kernels (csrc/lpips.hip), but the library does not ship the VGG16 and `lpips` weights -- `LPIPSNet.from_files` loads them
from the two files of the caller's own LPIPS install, and nothing is downloaded.  Without the keyword both functions return exactly what they returned
before it existed.

HIP only: raises for CPU tensors (there is no CPU path)."""
import torch

from . import frame_export, losses
from . import lpips as _lpips


def image_metrics(renders, gts, lpips_net=None, quantize=False):
    """renders, gts: (N, C, H, W) (or (C, H, W): one image).  -> {"ssim": (N,), "psnr": (N,), "l1": (N,)} float32 on the device, nothing waits for it.
    ssim = `ssim(render, gt)` per image, psnr = 20 log10(1 / sqrt(mse)) per image, l1 = mean |render - gt| per image.
    With `lpips_net` (an `LPIPSNet`; C = 3, sides 16 .. 4096) also "lpips": (N,), `lpips.lpips(renders, gts, lpips_net)`.
    With `quantize=True` both images first go through `frame_export.quantize` -- save_image's rounding to a byte, then / 255 -- which is what the
    reference's metrics.py measures: it reads back the 8-bit PNGs render.py wrote (metrics.py:24-34).  Without the keyword every call keeps its bits."""
    dims = losses._ssim_check("image_metrics", renders, gts, 11, (3, 4))
    if quantize:
        renders, gts = frame_export.quantize(renders), frame_export.quantize(gts)
    x = renders.detach().float().contiguous()
    y = gts.detach().float().contiguous()
    n = dims[0]
    with torch.cuda.device(x.device):
        per, mse, l1 = (torch.empty(n, dtype=torch.float32, device=x.device) for _ in range(3))
    losses._ssim_forward(dims, x, y, per_image=per, mse=mse, l1_per_image=l1)
    psnr = 20.0 * torch.log10(1.0 / torch.sqrt(mse))
    out = {"ssim": per, "psnr": psnr, "l1": l1}
    if lpips_net is not None:
        out["lpips"] = _lpips.lpips(renders, gts, lpips_net)
    return out


def evaluate_images(renders, gts, names=None, lpips_net=None, quantize=False):
    """What metrics.py:75-98 computes for SSIM and PSNR, and with `lpips_net` (an `LPIPSNet`) for LPIPS too.  renders, gts: a 4-D tensor each, or lists of (3, H, W) / (1, 3, H, W) tensors whose sizes may differ
    from view to view (views of one size go into one launch).  names: one per view (default "00000", "00001", ..).
    -> {"SSIM": mean, "PSNR": mean, "per_view": {"SSIM": {name: value}, "PSNR": {name: value}}}, Python floats, after ONE device-to-host copy.
    With `lpips_net` the dictionary also holds "LPIPS": mean and per_view["LPIPS"]: {name: value} -- still after ONE copy; without it, neither.
    `quantize=True`: every view is measured as `image_metrics(..., quantize=True)` measures it (the reference's protocol on 8-bit images)."""
    def views(t, what):
        if torch.is_tensor(t):
            if t.dim() != 4:
                raise ValueError("evaluate_images: %s must be a 4-D tensor or a list of images, got %s" % (what, tuple(t.shape)))
            return list(t.unbind(0))
        out = []
        for v in t:
            if not torch.is_tensor(v) or v.dim() not in (3, 4) or (v.dim() == 4 and v.shape[0] != 1):
                raise ValueError("evaluate_images: every entry of %s must be a (C, H, W) or (1, C, H, W) tensor" % what)
            out.append(v[0] if v.dim() == 4 else v)
        return out

    r, g = views(renders, "renders"), views(gts, "gts")
    if len(r) != len(g) or not r:
        raise ValueError("evaluate_images: %d renders, %d ground-truth images" % (len(r), len(g)))
    names = ["%05d" % i for i in range(len(r))] if names is None else [str(n) for n in names]
    if len(names) != len(r) or len(set(names)) != len(names):
        raise ValueError("evaluate_images: %d distinct names for %d views" % (len(set(names)), len(r)))
    groups = {}
    for i, (a, b) in enumerate(zip(r, g)):
        if a.shape != b.shape:
            raise ValueError("evaluate_images: view %s: render %s, ground truth %s" % (names[i], tuple(a.shape), tuple(b.shape)))
        groups.setdefault((tuple(a.shape), a.device), []).append(i)
    order, parts = [], []
    for idx in groups.values():
        m = image_metrics(torch.stack([r[i] for i in idx]), torch.stack([g[i] for i in idx]), lpips_net, quantize)
        order += idx
        parts.append(torch.stack([m["ssim"], m["psnr"]] + ([m["lpips"]] if lpips_net is not None else [])).to(parts[0].device if parts else m["ssim"].device))
    table = torch.cat(parts, dim=1)
    rows = torch.cat([table, table.mean(dim=1, keepdim=True)], dim=1).tolist()          # the one copy to the host
    per = {"SSIM": {}, "PSNR": {}}
    pos = {view: k for k, view in enumerate(order)}
    for i, name in enumerate(names):
        per["SSIM"][name] = rows[0][pos[i]]
        per["PSNR"][name] = rows[1][pos[i]]
    out = {"SSIM": rows[0][-1], "PSNR": rows[1][-1], "per_view": per}
    if lpips_net is not None:
        out["LPIPS"] = rows[2][-1]
        per["LPIPS"] = {name: rows[2][pos[i]] for i, name in enumerate(names)}
    return out
