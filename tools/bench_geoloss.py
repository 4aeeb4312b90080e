"""The fused geometry loss terms (ibgs_amd/losses.py `photometric_loss` / `normal_consistency`; csrc/geoloss.hip) against what a user composes without them
-- `losses.ssim_map` plus torch ops for the photometric term (with clamp(min=1) in place of the reference's host branch), the torch expression of
train.py:310-315 for the normal term -- in ONE process on one MI355X, at (3, 1080, 1920) and (3, 720, 1280), three sources, a 40 % mask.
Output: profiles/geoloss.txt.

    python tools/bench_geoloss.py [--out profiles/geoloss.txt] [--iters 20] [--repeats 15] [--no-train-iter]

Per size, both ways, alternating:
  photometric fwd + bwd      at the default weights (0.3, 1.0) and at photo_ssim_weight = 0.35, the gradient into `warped`
  photometric forward alone  fused only, with and without the derivative planes: what storing them costs the forward (the open choice)
  normal fwd + bwd           both gradients
For the record, no bar: bench.TrainIteration(full=True) (normal term + the L1 half of the photometric term, in torch) against the same iteration with the two
fused terms at the default photo_ssim_weight (i.e. the SSIM half).
Timing: hipEvents around `iters` back-to-back calls on the current stream, after a warm-up; the median over `repeats` such windows, and their minimum and
maximum.  The byte floor quoted beside the fused photometric pair, per source-pixel: forward 12 (gt) + 12 (warped) + 16 (features) read, 36 (three derivative
planes x three channels) written; backward 36 + 16 + 24 read, 12 written = 164 B, at 8 TB/s.  A measurement needs the GPU: without one this script fails."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ibgs_amd import losses  # noqa: E402

HBM_BYTES_PER_S = 8e12
PHOTO_BYTES = 164.0


def composed_photometric(gt, warped, cam_feat, nb, pw, ws):
    """train.py:320-338 over the fused map; clamp(min=1) instead of `if torch.sum(valid_mask) > 0`."""
    h, w = gt.shape[-2:]
    warped = warped.view(-1, 3, h, w)[:nb]
    mask = (torch.sum(cam_feat.view(-1, 4, h, w)[:nb], dim=1, keepdim=True) > 0).float()
    ref = gt.unsqueeze(0)
    masked = mask * warped + (1 - mask) * ref
    nv = torch.sum(mask[:, 0]).clamp(min=1.0)
    ssim_loss = 1 - torch.stack([losses.ssim_map(ref[0], masked[i]).mean(0) for i in range(len(masked))])
    ssim_loss = torch.sum(ssim_loss * mask[:, 0]) / nv
    l1 = torch.sum(torch.abs(ref - masked).mean(1) * mask[:, 0]) / nv
    return ((1 - ws) * l1 + ws * ssim_loss) * pw


def torch_normal(normal, dn, weight):
    return 0.4 * (weight * (dn - normal).abs().sum(0).mean()) + 0.6 * (weight * (1 - (dn * normal).sum(0)).mean())


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


def train_iteration_record(say, steps):
    import bench
    from ibgs_amd import synthetic as syn
    from ibgs_amd.optim import FusedAdam

    class FusedTerms(bench.TrainIteration):
        """TrainIteration(full=True) with its two torch-restated terms replaced by the fused ones (the photometric one at the default photo_ssim_weight)."""
        def __call__(self):
            k = self.it % 8
            self.it += 1
            out = self.renderer.render(self.cams[k], self.pc, self.scene, self.pipe, self.args, self.bg, True, 4, 4, render_geo=True, return_depth_normal=True)
            gt = self.scene.original_image_list[k]
            loss = (1.0 - 0.2) * torch.abs(out["render"] - gt).mean()
            loss = loss + losses.normal_consistency(out["rendered_normal"], out["median_intersected_depth_normal"], 0.03)
            loss = loss + losses.photometric_loss(gt, out["warped_image"], out["cam_feat"], 3, 0.3, 1.0)
            loss.backward()
            with torch.no_grad():
                self.scene.rendered_depth_list[k] = out["median_intersected_depth"].detach()
                self.densify.add_densification_stats(self.st, out["viewspace_points"], out["viewspace_points_abs"], out["radii"])
            self.opt.step()
            self.opt.zero_grad(set_to_none=True)

    dev = torch.device("cuda")
    c = syn.CONFIGS["C3"]
    res = {}
    for name, cls in (("torch terms (normal + photometric L1 half)", bench.TrainIteration), ("fused terms (normal + photometric SSIM half)", FusedTerms)):
        ti = cls(dev, c, FusedAdam, full=True)
        res[name] = bench.timed_wall_ms(ti, steps, warmup=10)
        del ti
        torch.cuda.empty_cache()
    say()
    say("== for the record: bench.TrainIteration(full=True) at C3, FusedAdam, wall ms per iteration over %d iterations (no bar: the two iterations do not compute the same loss)" % steps)
    for name, ms in res.items():
        say("%-48s %8.3f ms" % (name, ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geoloss.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--no-train-iter", action="store_true")
    ap.add_argument("--train-steps", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geoloss.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    th, tw = losses.geoloss_tile()
    say("# tools/bench_geoloss.py on one %s: the fused terms (tile %d x %d) against their composition (losses.ssim_map + torch ops; the torch expression of the normal term)," % (torch.cuda.get_device_name(0), th, tw))
    say("# one process, hipEvents around %d back-to-back calls, median [min .. max] of %d windows, the two alternating" % (args.iters, args.repeats))
    verdict = []
    for (h, w) in ((1080, 1920), (720, 1280)):
        g = torch.Generator().manual_seed(h)
        st = 4          # the rasterizer's output, taken whole: four sources, three visible
        gt = torch.rand((3, h, w), generator=g).to(dev)
        warped = (gt[None] + 0.08 * torch.randn((st, 3, h, w), generator=g).to(dev)).clamp(0, 1).reshape(3 * st, h, w).contiguous()
        mask = (torch.rand((st, 1, h, w), generator=g) < 0.4).to(dev)
        feat = ((torch.rand((st, 4, h, w), generator=g).to(dev) + 0.1) * mask).reshape(4 * st, h, w).contiguous()
        n = torch.nn.functional.normalize(torch.randn((3, h, w), generator=g), dim=0).to(dev)
        dn = torch.nn.functional.normalize(n + 0.2 * torch.randn((3, h, w), generator=g).to(dev), dim=0)
        wl = warped.clone().requires_grad_(True)
        nl, dnl = n.clone().requires_grad_(True), dn.clone().requires_grad_(True)
        say()
        say("== (3, %d, %d), 3 of 4 sources, %.1f %% of their pixels valid" % (h, w, 100.0 * float(mask[:3].float().mean())))

        def photo(fn, ws):
            wl.grad = None
            fn(gt, wl, feat, 3, 0.3, ws).backward()
            return wl.grad

        def photo_fwd(grad):
            if grad:
                return losses.photometric_loss(gt, wl, feat, 3, 0.3, 1.0)
            with torch.no_grad():
                return losses.photometric_loss(gt, wl, feat, 3, 0.3, 1.0)

        def normal(fn):
            nl.grad = dnl.grad = None
            fn(nl, dnl, 0.03).backward()
            return nl.grad

        for ws in (1.0, 0.35):
            a, b = photo(composed_photometric, ws).clone(), photo(losses.photometric_loss, ws).clone()
            say("same results, w_s %.2f: loss %.7f (composed) %.7f (fused); max |d grad| %.2e of max |grad| %.2e"
                % (ws, float(composed_photometric(gt, warped, feat, 3, 0.3, ws)), float(losses.photometric_loss(gt, warped, feat, 3, 0.3, ws)),
                   float((a - b).abs().max()), float(a.abs().max())))
        a, b = normal(torch_normal).clone(), normal(losses.normal_consistency).clone()
        say("same results, normal: loss %.7f (torch) %.7f (fused); max |d grad| %.2e of max |grad| %.2e"
            % (float(torch_normal(n, dn, 0.03)), float(losses.normal_consistency(n, dn, 0.03)), float((a - b).abs().max()), float(a.abs().max())))
        floor_us = PHOTO_BYTES * 3 * h * w / HBM_BYTES_PER_S * 1e6
        rows = (("photometric fwd + bwd, w_s 1.0", {"composed": lambda: photo(composed_photometric, 1.0), "fused": lambda: photo(losses.photometric_loss, 1.0)}),
                ("photometric fwd + bwd, w_s 0.35", {"composed": lambda: photo(composed_photometric, 0.35), "fused": lambda: photo(losses.photometric_loss, 0.35)}),
                ("normal consistency fwd + bwd", {"composed": lambda: normal(torch_normal), "fused": lambda: normal(losses.normal_consistency)}))
        for name, fns in rows:
            r = compare(fns, args.iters, args.repeats)
            faster = r["fused"][0] < r["composed"][0]
            verdict.append(faster)
            say("%-34s composed %8.3f ms [%7.3f .. %7.3f]   fused %8.3f ms [%7.3f .. %7.3f]   composed / fused %5.1f x   fused faster: %s"
                % (name, r["composed"][0], r["composed"][1], r["composed"][2], r["fused"][0], r["fused"][1], r["fused"][2], r["composed"][0] / r["fused"][0], faster))
            if name.endswith("w_s 1.0"):
                say("%-34s byte floor of the fused pair (164 B per source-pixel at 8 TB/s): %.1f us = %.0f %% of its time" % ("", floor_us, 100.0 * floor_us / (r["fused"][0] * 1e3)))
        r = compare({"plain": lambda: photo_fwd(False), "planes": lambda: photo_fwd(True)}, args.iters, args.repeats)
        say("%-34s without derivative planes %8.3f ms [%7.3f .. %7.3f]   with %8.3f ms [%7.3f .. %7.3f]   storing them costs the forward %.3f ms"
            % ("photometric forward alone, fused", r["plain"][0], r["plain"][1], r["plain"][2], r["planes"][0], r["planes"][1], r["planes"][2], r["planes"][0] - r["plain"][0]))
    say()
    say("every fused term faster than its composition at both sizes: %s" % all(verdict))
    if not args.no_train_iter:
        train_iteration_record(say, args.train_steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
