"""LPIPS on the matrix cores (ibgs_amd/lpips.py `lpips`; csrc/lpips.hip) against its torch composition ON THE DEVICE -- 13 F.conv2d, ReLUs, 4 max_pool2d and
the head in torch ops, float32, written from the definition (include/ibgs_lpips.h) -- in ONE process on one MI355X, for one pair at (3, 1080, 1920) and
(3, 720, 1280), under no_grad, with seeded He-normal weights (the library ships none; the time does not depend on the values).  Output: profiles/lpips.txt.

    python tools/bench_lpips.py [--out profiles/lpips.txt] [--iters 3] [--repeats 7] [--warmup 6] [--sizes 1080x1920,720x1280]

Per size: `lpips()` and the composition, alternating, after `warmup` calls of each (MIOpen compiles and chooses its kernels on the first uses of a shape):
hipEvents around `iters` back-to-back calls, the median over `repeats` such windows, their minimum and maximum.  Then every convolution launch alone
(ibgs_lpips_conv3 on the arena's stages, both images), the head and final sum as the remainder, the multiply-adds of a pair counted from the shapes, the f32
matrix floor 2 x MACs / 157.3 TFLOP/s and the fraction of it reached, the max-abs difference of the two device results (no float64 arbiter is affordable
at these sizes: tests/test_gpu_lpips.py holds the bar at small ones), and hipcc's resource report per instantiation.  A measurement needs the GPU."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ibgs_amd import _build, _device, _lib, lpips as lp  # noqa: E402

FP32_FLOPS = 157.3e12
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)


def composed(x, y, net, return_maps=False):
    """x, y: (3, H, W).  -> lpips (0-d), and with return_maps the five maps."""
    t = torch.stack([x, y])
    t = (t - t.new_tensor(MEAN)[None, :, None, None]) / t.new_tensor(STD)[None, :, None, None]
    total, maps, tap = 0.0, [], 0
    for i, name in enumerate(lp.CONV_NAMES):
        if i > 0 and lp.LEVEL[i] != lp.LEVEL[i - 1]:
            t = F.max_pool2d(t, 2, 2)
        t = F.relu(F.conv2d(t, getattr(net, name + "_w"), getattr(net, name + "_b"), padding=1))
        if i == lp.TAP_CONV[tap]:
            n = t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + 1e-10)
            m = F.conv2d((n[0:1] - n[1:2]) ** 2, getattr(net, lp.LIN_NAMES[tap] + "_w").reshape(1, -1, 1, 1))
            total = total + m.mean()
            maps.append(m[0, 0])
            tap += 1
    return (total, maps) if return_maps else total


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def compare(fns, iters, repeats, warmup):
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        print("  (warmed up: %s)" % k, flush=True)
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_ms(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def layer_macs(h, w):
    """multiply-adds of every convolution for a PAIR (both images), from the shapes"""
    sides = lp.level_sides(h, w)
    return [2 * lp.CHANNELS[i] * lp.CHANNELS[i + 1] * 9 * sides[lp.LEVEL[i]][0] * sides[lp.LEVEL[i]][1] for i in range(13)]


def per_layer(x, y, net, h, w, iters, repeats):
    """-> [ms] of the thirteen convolution launches alone, on the stages a forward left in a scratch arena"""
    dev = x.device
    arena = _device.scratch(dev, _lib.load().ibgs_lpips_required_scratch(h, w))
    words = arena.view(torch.float32)
    stage, _ = lp._stage_offsets(h, w)
    sides = lp.level_sides(h, w)
    out = []
    for i, name in enumerate(lp.CONV_NAMES):
        k, cin, cout = lp.LEVEL[i], lp.CHANNELS[i], lp.CHANNELS[i + 1]
        pool = i > 0 and lp.LEVEL[i - 1] != k
        hs, ws = sides[k - 1] if pool else sides[k]
        if i == 0:
            in_x, in_y = x.data_ptr(), y.data_ptr()
        else:
            in_x = words[stage[i - 1]:].data_ptr()
            in_y = in_x + 4 * cin * hs * ws
        wt, bt = getattr(net, name + "_w"), getattr(net, name + "_b")
        fn = lambda: _device.call(dev, "ibgs_lpips_conv3", hs, ws, cin, cout, int(pool), int(i == 0), in_x, in_y, wt.data_ptr(), bt.data_ptr(), words[stage[i]:].data_ptr())
        fn()
        torch.cuda.synchronize()
        out.append(statistics.median(window_ms(fn, iters) for _ in range(repeats)))
    return out


def resource_report(say):
    src = os.path.join(_build.CSRC, "lpips.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([_build._hipcc()] + _build.compile_flags("lpips") + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "lpips.o")],
                           capture_output=True, text=True)
    if r.returncode != 0:
        say("hipcc's resource report could not be produced (exit %d)" % r.returncode)
        return
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            k = re.search(r"(lpips_[a-z0-9_]+?_kernel)", m.group(1))
            t = re.search(r"ILb([01])ELb([01])E", m.group(1))
            cur = {"name": (k.group(1) if k else m.group(1)) + ("<%s, %s>" % ("pool" if t.group(1) == "1" else "plain", "first" if t.group(2) == "1" else "-") if t else "")}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    say("hipcc's report for lpips.hip per instantiation (lpips_conv3_kernel<read mode of the input, first layer with the z-score>):")
    for c in rows:
        say("  %-36s VGPRs %3d  AGPRs %3d  spilled VGPRs %d  SGPRs %d  scratch %d B/lane  LDS %5d B  occupancy %d waves/SIMD"
            % (c["name"], c.get("VGPRs", -1), c.get("AGPRs", -1), c.get("VGPRs Spill", -1), c.get("SGPRs Spill", -1), c.get("ScratchSize", -1), c.get("LDS Size", -1), c.get("Occupancy", -1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips.txt"))
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--sizes", default="1080x1920,720x1280")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/bench_lpips.py on one %s: LPIPS (VGG16) of one pair on the matrix cores (13 convolution launches over both images, 5 head launches, 1 sum) against its torch" % torch.cuda.get_device_name(0))
    say("# composition on the device (13 conv2d, ReLUs, 4 max_pool2d, the head in torch ops; float32, MIOpen), one process, no_grad, seeded He-normal weights,")
    say("# hipEvents around %d back-to-back calls, median [min .. max] of %d windows after %d warm-up calls each, the candidates alternating" % (args.iters, args.repeats, args.warmup))
    torch.manual_seed(0)
    net = lp.LPIPSNet().to(dev)
    verdict = {}
    with torch.no_grad():
        for size in args.sizes.split(","):
            h, w = (int(v) for v in size.split("x"))
            g = torch.Generator().manual_seed(h)
            x = torch.rand((3, h, w), generator=g).to(dev)
            y = (x + 0.1 * torch.randn((3, h, w), generator=g).to(dev)).clamp(0, 1)
            say()
            say("== (3, %d, %d)" % (h, w))
            mine, maps = lp.lpips(x, y, net, return_maps=True)
            theirs, their_maps = composed(x, y, net, True)
            say("same results: lpips hip %.9f torch %.9f (|d| %.2e); max |d map_k| %s of max |map_k| %s"
                % (float(mine[0]), float(theirs), abs(float(mine[0]) - float(theirs)), " ".join("%.2e" % float((a[0] - b).abs().max()) for a, b in zip(maps, their_maps)),
                   " ".join("%.2e" % float(b.abs().max()) for b in their_maps)))
            del maps, their_maps
            torch.cuda.empty_cache()
            r = compare({"hip": lambda: lp.lpips(x, y, net), "torch float32": lambda: composed(x, y, net)}, args.iters, args.repeats, args.warmup)
            for k in r:
                say("%-16s %8.3f ms [%7.3f .. %7.3f]" % (k, r[k][0], r[k][1], r[k][2]))
            faster = r["hip"][0] < r["torch float32"][0]
            verdict[size] = faster
            say("torch float32 / hip %5.2f x   hip faster than torch float32: %s" % (r["torch float32"][0] / r["hip"][0], faster))
            macs = layer_macs(h, w)
            floor_ms = 2 * sum(macs) / FP32_FLOPS * 1e3
            say("arithmetic: %.4g multiply-adds per pair; f32 matrix floor (2 x MACs / 157.3 TFLOP/s) %.3f ms = %.0f %% of the hip time reached; arena %.2f GB"
                % (sum(macs), floor_ms, 100.0 * floor_ms / r["hip"][0], _lib.load().ibgs_lpips_required_scratch(h, w) / 1e9))
            ms = per_layer(x, y, net, h, w, args.iters, args.repeats)
            sides = lp.level_sides(h, w)
            for i, name in enumerate(lp.CONV_NAMES):
                fl = 2 * macs[i] / FP32_FLOPS * 1e3
                say("  %-8s %3d -> %3d at %4d x %4d%s  %8.3f ms   floor %7.3f ms = %3.0f %%"
                    % (name, lp.CHANNELS[i], lp.CHANNELS[i + 1], sides[lp.LEVEL[i]][0], sides[lp.LEVEL[i]][1], " (pooled in)" if i > 0 and lp.LEVEL[i] != lp.LEVEL[i - 1] else "            ",
                       ms[i], fl, 100.0 * fl / ms[i]))
            say("  the thirteen convolutions %8.3f ms; five head launches, the final sum and the host's part (the remainder) %8.3f ms" % (sum(ms), r["hip"][0] - sum(ms)))
            del x, y
            torch.cuda.empty_cache()
    say()
    say("lpips() faster than the torch float32 composition on the device: %s" % ", ".join("%s %s" % kv for kv in verdict.items()))
    say()
    resource_report(say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
