"""The fused colour aggregation front end (ibgs_amd/coloragg.py `per_view_features`; csrc/coloragg.hip) against its torch composition -- the assembly that
tests/scenes.fuse_color_inputs restates, written in torch from the definition, then nn.Sequential(Linear, ReLU, Linear, ReLU) over the (HW levels, 7) rows, the
mean over the views and the concatenation into (1, 38, H, W), with one `.item()` for the level count -- in ONE process on one MI355X, at (3, 1080, 1920) and
(3, 720, 1280), three sources, 60 % of the slots valid.  Output: profiles/coloragg.txt.

    python tools/bench_coloragg.py [--out profiles/coloragg.txt] [--iters 10] [--repeats 11]

Per size, both ways, alternating:
  forward                    under no_grad (a test frame)
  forward + backward, all    gradients of render, warped_image and the four parameters (a steady-state iteration)
  forward + backward, params render and warped_image detached (the reference's burn-in)
and, fused only, the aggregation mode "max"; and once per size what STORING h1 and h2 for the backward would move instead of recomputing them: a device
copy of 64 floats per pixel and source, i.e. one write and one read of that array.
Timing: hipEvents around `iters` back-to-back calls on the current stream, after a warm-up; the median over `repeats` such windows, and their minimum and
maximum.  The byte floor quoted beside the fused forward: 27 floats read and 38 written per pixel at 3 sources, at 8 TB/s; the arithmetic floor: 1 248
multiply-adds per pixel and source at 157 TFLOP/s.  A measurement needs the GPU: without one this script fails."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ibgs_amd import coloragg  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP32_FLOPS = 157.3e12


def composed(render, warped, cam_feat, camera_ray, mlp, nb):
    """The front end from its definition in torch ops, as tests/coloragg_ref.torch_composition states it, with the network as an
    nn.Sequential and the level count read on the host: per slot the mask from the four feature planes, the masked colour difference and the features as seven
    planes, those as (pixels x levels, 7) rows through the two layers, the mean over the levels, and the 38 planes."""
    _, h, w = render.shape
    colours, feats = warped.reshape(-1, 3, h, w), cam_feat.reshape(-1, 4, h, w)
    levels = min(int((colours != 0).flatten(1).any(dim=1).sum().item()), nb, colours.shape[0])          # the one host sync
    colours, feats = colours[:levels], feats[:levels]
    valid = (feats.sum(dim=1, keepdim=True) > 0).to(render.dtype)                        # (levels, 1, H, W)
    planes = torch.cat([(colours - render[None]) * valid, feats], dim=1)                # (levels, 7, H, W)
    rows = planes.permute(2, 3, 0, 1).reshape(h * w * levels, 7)
    agg = mlp(rows).reshape(h * w, levels, -1).mean(dim=1)                               # (HW, 32)
    return torch.cat([agg.t().reshape(-1, h, w), camera_ray, render], dim=0).unsqueeze(0)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coloragg.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=11)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coloragg.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/bench_coloragg.py on one %s: the fused front end against its torch composition (assembly + nn.Sequential(Linear, ReLU, Linear, ReLU) + mean + cat)," % torch.cuda.get_device_name(0))
    say("# one process, hipEvents around %d back-to-back calls, median [min .. max] of %d windows, the two alternating" % (args.iters, args.repeats))
    torch.manual_seed(0)
    front = coloragg.PerViewFrontEnd().to(dev)
    mlp = nn.Sequential(nn.Linear(7, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU()).to(dev)
    with torch.no_grad():
        mlp[0].weight.copy_(front.w1); mlp[0].bias.copy_(front.b1); mlp[2].weight.copy_(front.w2); mlp[2].bias.copy_(front.b2)
    params_f, params_c = list(front.parameters()), list(mlp.parameters())
    verdict = []
    for (h, w) in ((1080, 1920), (720, 1280)):
        g = torch.Generator().manual_seed(h)
        s = 3
        render = torch.rand((3, h, w), generator=g).to(dev)
        warped = (render[None] + 0.1 * torch.randn((s, 3, h, w), generator=g).to(dev)).clamp(0, 1).reshape(3 * s, h, w).contiguous()
        mask = (torch.rand((s, 1, h, w), generator=g) < 0.6).to(dev)
        feat = ((torch.rand((s, 4, h, w), generator=g).to(dev) + 0.1) * mask).reshape(4 * s, h, w).contiguous()
        ray = torch.nn.functional.normalize(torch.randn((3, h, w), generator=g), dim=0).to(dev)
        up = torch.randn((1, 38, h, w), generator=g).to(dev)
        rl, wl = render.clone().requires_grad_(True), warped.clone().requires_grad_(True)
        say()
        say("== (3, %d, %d), 3 sources, %.1f %% of the slots valid" % (h, w, 100.0 * float(mask.float().mean())))

        def run(fused, grads, mode="mean"):
            """grads: None (forward under no_grad), "all" or "params"."""
            r, x = (rl, wl) if grads == "all" else (render, warped)
            if fused:
                call = lambda: coloragg.per_view_features(r, x, feat, ray, front.w1, front.b1, front.w2, front.b2, 3, mode)[0]
            else:
                call = lambda: composed(r, x, feat, ray, mlp, 3)
            if grads is None:
                with torch.no_grad():
                    return call(), ()
            leaves = ([rl, wl] if grads == "all" else []) + (params_f if fused else params_c)
            out = call()
            return out, torch.autograd.grad((out * up).sum(), leaves)

        oc, gc = run(False, "all")
        of, gf = run(True, "all")
        oc, of = oc.detach(), of.detach()
        say("same results: max |d out| %.2e of max |out| %.2e; gradients max |d| / max |.|: %s"
            % (float((oc - of).abs().max()), float(oc.abs().max()), "  ".join("%.1e" % (float((a - b).abs().max()) / float(a.abs().max())) for a, b in zip(gc, gf))))
        del oc, of, gc, gf
        byte_us = (27 + 38) * 4 * h * w / HBM_BYTES_PER_S * 1e6
        flop_us = 2 * 1248 * 3 * h * w / FP32_FLOPS * 1e6
        for name, grads in (("forward (no_grad)", None), ("forward + backward, all gradients", "all"), ("forward + backward, parameters only", "params")):
            r = compare({"composed": lambda: run(False, grads), "fused": lambda: run(True, grads), "fused max": lambda: run(True, grads, "max")}, args.iters, args.repeats)
            faster = r["fused"][0] < r["composed"][0]
            verdict.append(faster)
            say("%-38s composed %8.3f ms [%7.3f .. %7.3f]   fused %8.3f ms [%7.3f .. %7.3f]   composed / fused %5.1f x   fused faster: %s   (fused, max mode %8.3f ms)"
                % (name, r["composed"][0], r["composed"][1], r["composed"][2], r["fused"][0], r["fused"][1], r["fused"][2], r["composed"][0] / r["fused"][0], faster, r["fused max"][0]))
            if grads is None:
                say("%-38s floors of the fused forward: bytes (65 floats per pixel at 8 TB/s) %.1f us, arithmetic (1 248 fma per pixel and source at 157 TFLOP/s) %.1f us = %.0f %% and %.0f %% of its time"
                    % ("", byte_us, flop_us, 100.0 * byte_us / (r["fused"][0] * 1e3), 100.0 * flop_us / (r["fused"][0] * 1e3)))
        stored = torch.empty((64 * s, h, w), dtype=torch.float32, device=dev)
        other = torch.empty_like(stored)
        r = compare({"copy": lambda: other.copy_(stored)}, args.iters, args.repeats)
        say("%-38s a device copy of 64 floats per pixel and source (%.2f GB written and as much read): %8.3f ms [%7.3f .. %7.3f]"
            % ("storing h1 and h2 instead", stored.numel() * 4 / 1e9, r["copy"][0], r["copy"][1], r["copy"][2]))
        del stored, other
        torch.cuda.empty_cache()
    say()
    say("the fused front end faster than its composition in every mode at both sizes: %s" % all(verdict))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
