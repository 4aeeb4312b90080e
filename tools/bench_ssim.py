"""The fused SSIM (ibgs_amd/losses.py `ssim` / `ssim_map`, ibgs_amd/image_eval.py; csrc/ssim.hip) against the torch formulation -- the reference's
expression (utils/loss_utils.py:34-91) restated with F.conv2d(groups=C) -- in ONE process on one MI355X, at (3, 1080, 1920) and (3, 720, 1280).
Output: profiles/ssim.txt.

    python tools/bench_ssim.py [--out profiles/ssim.txt] [--iters 20] [--repeats 15]

Per size, both ways, alternating:
  loss forward            1 - ssim(image, gt) under no_grad
  loss forward + backward the same with the image requiring grad, and its backward (train.py:302, 355)
  photometric, 3 sources  train.py:327-331 on top of the map: masked = mask warped + (1 - mask) ref, 1 - map.mean(0) per source, the masked mean; forward +
                          backward into `warped`
  image_metrics           SSIM + PSNR + L1 of one view from one launch, against ssim + psnr + l1 in torch (metrics.py:79-81)
Timing: hipEvents around `iters` back-to-back calls on the current stream, after a warm-up of every shape; the median over `repeats` such windows, and their
minimum and maximum.  The byte floor quoted beside the fused forward + backward: 8 B read + 12 B written per plane-pixel forward (two images; three
derivative planes), 20 B read + 4 B written backward, at 8 TB/s.  A measurement needs the GPU: without one this script fails."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ibgs_amd import image_eval, losses  # noqa: E402
from tests import ssim_ref  # noqa: E402

HBM_BYTES_PER_S = 8e12
C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- the torch formulation ---------------------------------------------------------------------------------------------------------------------------
_windows = {}


def torch_window(c, dev):
    """(like the reference, which builds it on every call, the window is float32 and per channel; it is cached here, which only helps torch)"""
    key = (c, str(dev))
    if key not in _windows:
        _windows[key] = ssim_ref.window_2d().to(dev).expand(c, 1, 11, 11).contiguous()
    return _windows[key]


def torch_ssim_map(x, y):
    c = x.size(-3)
    w = torch_window(c, x.device)
    mu1, mu2 = F.conv2d(x, w, padding=5, groups=c), F.conv2d(y, w, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, w, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(y * y, w, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(x * y, w, padding=5, groups=c) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def torch_ssim(x, y):
    return torch_ssim_map(x, y).mean()


def torch_psnr(x, y):
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def photometric(mapfn, ref_image, warped, mask):
    masked = mask * warped + (1 - mask) * ref_image
    loss = 1 - torch.stack([mapfn(ref_image, masked[i]).mean(0) for i in range(len(masked))])
    return torch.sum(loss * mask[:, 0]) / torch.sum(mask[:, 0])


# ---- timing ------------------------------------------------------------------------------------------------------------------------------------------
def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def compare(fns, iters, repeats):
    """fns: {name: callable}.  Warm-up, then `repeats` windows of each, alternating.  -> {name: (median, min, max) ms per call}"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_ms(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    th, tw = losses.ssim_tile()
    say("# tools/bench_ssim.py on one %s: torch formulation (F.conv2d, groups=C, float32) against the fused kernels (tile %d x %d), one process," % (torch.cuda.get_device_name(0), th, tw))
    say("# hipEvents around %d back-to-back calls, median [min .. max] of %d windows, the two alternating" % (args.iters, args.repeats))
    for (c, h, w) in ((3, 1080, 1920), (3, 720, 1280)):
        g = torch.Generator().manual_seed(h)
        gt = torch.rand((c, h, w), generator=g).to(dev)
        image = (gt + 0.05 * torch.randn((c, h, w), generator=g).to(dev)).clamp(0, 1)
        warped = (gt[None] + 0.08 * torch.randn((3, c, h, w), generator=g).to(dev)).clamp(0, 1)
        mask = (torch.rand((3, 1, h, w), generator=g) < 0.4).to(dev).float()
        x = image.clone().requires_grad_(True)
        wl = warped.clone().requires_grad_(True)
        say()
        say("== (%d, %d, %d)" % (c, h, w))

        def fwd(f):
            with torch.no_grad():
                return 1.0 - f(image, gt)

        def fwd_bwd(f):
            x.grad = None
            (1.0 - f(x, gt)).backward()
            return x.grad

        def photo(mapfn):
            wl.grad = None
            photometric(mapfn, gt, wl, mask).backward()
            return wl.grad

        def metrics_torch():
            with torch.no_grad():
                a, b = image[None], gt[None]
                return torch_ssim(a, b), torch_psnr(a, b), torch.abs(a - b).mean()

        def metrics_fused():
            return image_eval.image_metrics(image[None], gt[None])

        # the two compute the same thing at this size
        v_t, v_f = float(fwd(torch_ssim)), float(fwd(losses.ssim))
        g_t, g_f = fwd_bwd(torch_ssim).clone(), fwd_bwd(losses.ssim).clone()
        p_t, p_f = photo(torch_ssim_map).clone(), photo(losses.ssim_map).clone()
        mt, mf = metrics_torch(), metrics_fused()
        say("same results: loss %.7f (torch) %.7f (fused); max |d grad| %.2e of max |grad| %.2e; photometric max |d grad| %.2e of %.2e; ssim %.7f / %.7f, psnr %.5f / %.5f"
            % (v_t, v_f, float((g_t - g_f).abs().max()), float(g_t.abs().max()), float((p_t - p_f).abs().max()), float(p_t.abs().max()),
               float(mt[0]), float(mf["ssim"][0]), float(mt[1]), float(mf["psnr"][0])))
        floor_us = 44.0 * c * h * w / HBM_BYTES_PER_S * 1e6
        rows = (("loss forward", {"torch": lambda: fwd(torch_ssim), "fused": lambda: fwd(losses.ssim)}),
                ("loss forward + backward", {"torch": lambda: fwd_bwd(torch_ssim), "fused": lambda: fwd_bwd(losses.ssim)}),
                ("photometric, 3 sources, fwd + bwd", {"torch": lambda: photo(torch_ssim_map), "fused": lambda: photo(losses.ssim_map)}),
                ("image_metrics (ssim + psnr + l1)", {"torch": metrics_torch, "fused": metrics_fused}))
        for name, fns in rows:
            r = compare(fns, args.iters, args.repeats)
            say("%-36s torch %8.3f ms [%7.3f .. %7.3f]   fused %8.3f ms [%7.3f .. %7.3f]   torch / fused %5.1f x"
                % (name, r["torch"][0], r["torch"][1], r["torch"][2], r["fused"][0], r["fused"][1], r["fused"][2], r["torch"][0] / r["fused"][0]))
            if name == "loss forward + backward":
                say("%-36s byte floor of the fused pair (44 B per plane-pixel at 8 TB/s): %.1f us = %.0f %% of its time; fused faster than torch: %s"
                    % ("", floor_us, 100.0 * floor_us / (r["fused"][0] * 1e3), r["fused"][0] < r["torch"][0]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
