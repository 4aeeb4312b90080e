"""The hourglass CNN on the matrix cores (ibgs_amd/hourglass.py `hourglass_forward`; csrc/hourglass.hip) against its torch composition -- nine
F.conv2d, two max_pool2d, two nearest interpolate, three cat, ReLUs and the image_pred expression, written from the definition --
in ONE process on one MI355X, at (38, 1080, 1920) and (38, 720, 1280), under no_grad.  Output: profiles/hourglass.txt.

    python tools/bench_hourglass.py [--out profiles/hourglass.txt] [--iters 5] [--repeats 9] [--warmup 12] [--append]

Per size, alternating:
  hip                the seven launches
  hip float16        `hourglass_forward(..., precision="float16")` (csrc/hghalf.hip): the packing launch and seven launches on the f16 matrix-core instruction;
                     its yardsticks are BOTH hip (the float32 kernel) and torch autocast (the precision the reference renders with)
  torch float32      the composition in float32 (MIOpen's convolutions): THE YARDSTICK
  torch autocast     the same under torch.autocast(float16), for the record: another precision, not a competitor on equal terms
and then the whole test-time tail from the rasterizer's planes: coloragg.fuse_color_inputs + hourglass (`hourglass.fuse_color`) against the fused front end
followed by the torch float32 CNN and the image_pred expression, and `hourglass.fuse_color(..., precision="float16")` beside them.  With --append the report
is written after the forward reports --out already holds (in front of the "# --train" part) instead of replacing them.
Timing: hipEvents around `iters` back-to-back calls on the current stream, after `warmup` calls of each (MIOpen chooses its kernels on the first uses of
a shape); the median over `repeats` such windows, and their minimum and maximum.  Floors quoted beside the hip forward: 52 218 multiply-adds per pixel at the
157.3 TFLOP/s f32 matrix peak, and the minimum traffic of the seven-launch split (x, e1 and u1 written once and read once or twice, the half- and
quarter-resolution stages, the outputs) at 8 TB/s.  Also printed: the padding efficiency of the 16-wide matrix instruction per layer and hipcc's register
and spill report per instantiation of the kernel.  A measurement needs the GPU: without one this script fails.

    python tools/bench_hourglass.py --train [--out profiles/hourglass.txt] ...

measures TRAINING by the same method, grad mode on: `hourglass_train` + backward (csrc/hgtrain.hip) against the torch float32 composition + autograd
(MIOpen) in the same process, with all nineteen gradients, with the parameter gradients only (a detached input) and with the input gradient only (a frozen
CNN); then the whole training tail, `fuse_color_train` + backward against front end + torch CNN + backward.  Beside them, alternating in the same windows, the
HALF-PRECISION rows (`hourglass_train(..., precision="float16")` and the two tails inside `hourglass.train_precision("float16")`; csrc/hghtrain.hip): `hourglass_train` with all gradients, parameters only and input only, `fuse_color_train`, and
`fuse_color_train_scaled` at 0.5; their yardsticks are the float32 rows and torch autocast(float16) + autograd on the device with the loss scaled by 2^10 and
the gradients divided by it.  Its report REPLACES the part of --out from the line "# --train" on and leaves the forward's report above it as it is."""
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

from ibgs_amd import _build, coloragg, hourglass, resample_train  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP32_FLOPS = 157.3e12
FP16_FLOPS = 2.5e15
# (layer, Cout, Cin, taps, resolution level): the multiply-adds per full-resolution pixel
MACS = sum(cout * cin * k * k / 4 ** level for (_, cout, cin, k), level in zip(hourglass.LAYERS, (0, 1, 2, 1, 1, 0, 0, 0, 0)))


def composed(x, p, burned):
    """x: (1, 38, H, W); p: the HourglassCNN.  -> (residual (3, H, W), image_pred)"""
    conv = lambda t, name, pad: F.conv2d(t, getattr(p, name + "_w"), getattr(p, name + "_b"), padding=pad)
    e1 = F.relu(conv(x, "enc1", 1))
    e2 = F.relu(conv(F.max_pool2d(e1, 2), "enc2", 1))
    b = F.relu(conv(F.max_pool2d(e2, 2), "enc3", 1))
    u2 = F.relu(conv(F.interpolate(b, size=e2.shape[-2:], mode="nearest"), "up2_conv", 1))
    d2 = F.relu(conv(torch.cat([u2, e2], 1), "dec2", 1))
    u1 = F.relu(conv(F.interpolate(d2, size=e1.shape[-2:], mode="nearest"), "up1_conv", 1))
    d1 = F.relu(conv(torch.cat([u1, e1], 1), "dec1", 1))
    f = F.relu(conv(torch.cat([d1, x], 1), "fuse_input", 0))
    residual = conv(f, "final", 0)[0]
    return residual, burned * x[0, 35:38] + residual


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def compare(fns, iters, repeats, warmup):
    """fns: {name: callable}.  Warm-up, then `repeats` windows of each, alternating.  -> {name: (median, min, max) ms per call}"""
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


def min_bytes(h, w):
    p1, p2, p4 = h * w, (h // 2) * (w // 2), (h // 4) * (w // 4)
    # x: read by enc1 and by the last launch; e1: written, read by enc2 (pooled) and the last launch; e2: written, read by enc3 and dec2; b, u2, d2: written and read
    # once; u1: written and read; the six output planes and the three colour planes read again
    return 4 * (2 * 38 * p1 + 3 * 38 * p1 + 3 * 19 * p2 + 2 * 9 * p4 + 2 * 19 * p2 + 2 * 19 * p2 + 2 * 38 * p1 + 9 * p1)


def min_bytes_half(h, w):
    p1, p2, p4 = h * w, (h // 2) * (w // 2), (h // 4) * (w // 4)
    # x (float32) read by the packing launch and h(x) (40 binary16 per pixel) written, then read by enc1 and by the last launch; the stages as in min_bytes at
    # 40 / 24 / 16 binary16 per pixel; the six output planes and the three colour planes read again
    return 4 * 38 * p1 + 2 * (3 * 40 * p1 + 3 * 40 * p1 + 3 * 24 * p2 + 2 * 16 * p4 + 2 * 24 * p2 + 2 * 24 * p2 + 2 * 40 * p1) + 4 * 9 * p1


# unit: (the legend above its rows, the width of a row's name, whether its template arguments are printed as the forward's <.., read mode, last launch>)
REPORTS = {"hourglass": ("hipcc's report for hourglass.hip per instantiation (<channels of A, channels of B, Cout, read mode of A, last launch>):", 48, True),
           "hghalf": ("hipcc's report for hghalf.hip per instantiation (<channels of A, channels of B, Cout, read mode of A, last launch>):", 48, True),
           "hgtrain": ("hipcc's report per instantiation of hgtrain.hip (hgb_conv_kernel<channels of A, of B, Cout, taps, transposed>; hgb_wgrad_kernel<channels of A, of B, Cout, read mode of A, taps>):", 44, False),
           "hghtrain": ("hipcc's report per instantiation of hghtrain.hip (hght_conv3_kernel<channels of A, of B, rows, epilogue: 0 float32, 1 masked binary16, 2 grad_x, 3 head>; "
                        "hght_wgrad_kernel<channels of A, of B, Cout, read mode of A, taps>):", 44, False)}


def resource_report(say, unit):
    """hipcc's own report for one of the four hourglass units with the build's flags (compiled to a scratch file): a row per kernel and instantiation."""
    legend, width, forward = REPORTS[unit]
    src = os.path.join(_build.CSRC, unit + ".hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([_build._hipcc()] + _build.compile_flags(unit) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "hg.o")],
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
            k = re.search(r"(hg[a-z]*_[a-z0-9_]+?)(?:I|E)", m.group(1))
            t = re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)(?:EL[ib]([0-9]+))?E", m.group(1))
            name = k.group(1) if k else m.group(1)
            if t and forward:
                name += "<%s, %s, %s, %s, %s>" % (t.group(1), t.group(2), t.group(3), ("plain", "pool", "up")[int(t.group(4))], "fused" if t.group(5) == "1" else "-")
            elif t:
                name += "<%s>" % ", ".join(v for v in t.groups() if v is not None)
            cur = {"name": name}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    say(legend)
    for c in rows:
        say("  %-*s VGPRs %3d  AGPRs %3d  spilled VGPRs %d  SGPRs %d  scratch %d B/lane  LDS %5d B  occupancy %d waves/SIMD"
            % (width, c["name"], c.get("VGPRs", -1), c.get("AGPRs", -1), c.get("VGPRs Spill", -1), c.get("SGPRs Spill", -1), c.get("ScratchSize", -1), c.get("LDS Size", -1), c.get("Occupancy", -1)))


TRAIN_MARK = "# --train"
# the backward's products per pixel: two per forward product of the 3 x 3 layers and of the 1 x 1 head (input and weight gradient), the recomputed dec1 and
# fuse_input, less enc1's input gradient when the input is detached
BWD_MACS = 2 * MACS + (38 * 76 * 9 + 38 * 76)


def min_bytes_half_train(h, w):
    """The minimum traffic of the half-precision backward's launches, from the shapes (bytes per pixel of each level: what every launch must read and write
    once, binary16 stages and G_* at 80 / 48 / 32 bytes per pixel, float32 input gradients at 160 / 96 / 64): without and with the weight gradients' reads."""
    p1, p2, p4 = h * w, (h // 2) * (w // 2), (h // 4) * (w // 4)
    routing = 2208 * p1 + 1120 * p2 + 320 * p4          # the head, the nine input gradients, the four gathers, grad_x
    wgrad = 816 * p1 + 656 * p2 + 256 * p4             # G and the layer's input, once per layer
    return routing, routing + wgrad


def main_train(args):
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(TRAIN_MARK + ": tools/bench_hourglass.py --train on one %s: forward + backward of the hourglass (hourglass_train; csrc/hgtrain.hip) against the torch float32 composition + autograd (MIOpen)," % torch.cuda.get_device_name(0))
    say("# one process, grad mode on, hipEvents around %d back-to-back calls, median [min .. max] of %d windows after %d warm-up calls each, the candidates alternating" % (args.iters, args.repeats, args.warmup))
    say("# arithmetic: %d multiply-adds per pixel forward, %d backward (two per forward product, and the recomputed dec1 and fuse_input)" % (round(MACS), round(BWD_MACS)))
    torch.manual_seed(0)
    net = hourglass.ColorAggregationNet().to(dev)
    cnn = net.cnn
    params = list(cnn.parameters())
    verdict, verdict16 = {}, {}
    for size in args.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(h)
        s = 3
        render = torch.rand((3, h, w), generator=g).to(dev)
        warped = (render[None] + 0.1 * torch.randn((s, 3, h, w), generator=g).to(dev)).clamp(0, 1).reshape(3 * s, h, w).contiguous()
        mask = (torch.rand((s, 1, h, w), generator=g) < 0.6).to(dev)
        feat = ((torch.rand((s, 4, h, w), generator=g).to(dev) + 0.1) * mask).reshape(4 * s, h, w).contiguous()
        ray = F.normalize(torch.randn((3, h, w), generator=g), dim=0).to(dev)
        pkg = {"render": render.requires_grad_(True), "warped_image": warped.requires_grad_(True), "cam_feat": feat, "camera_ray": ray,
               "min_depth_diff": torch.rand((1, h, w), generator=g).to(dev)}
        with torch.no_grad():
            x0, _ = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
        up = torch.randn((3, h, w), generator=g).to(dev)
        say()
        say("== (38, %d, %d)" % (h, w))

        def step(forward, x_grad, p_grad, scale=None):
            def run():
                x = x0.detach().requires_grad_(x_grad)
                for q in params:
                    q.requires_grad_(p_grad)
                    q.grad = None
                _, ip = forward(x)
                if scale is None:
                    (ip * up).sum().backward()
                    return x.grad, [q.grad for q in params]
                ((ip.float() * up).sum() * scale).backward()          # torch autocast: the loss scaled, the gradients divided in float32
                return (None if x.grad is None else x.grad / scale), [None if q.grad is None else q.grad.div_(scale) for q in params]
            return run
        hip = lambda x: hourglass.hourglass_train(x, cnn, render_scale=1.0)
        half = lambda x: hourglass.hourglass_train(x, cnn, render_scale=1.0, precision="float16")
        tor = lambda x: composed(x, cnn, 1.0)

        def auto(x):
            with torch.autocast("cuda", dtype=torch.float16):
                return composed(x, cnn, 1.0)
        LOSS_SCALE = 2.0 ** 10
        gx_h, gp_h = step(hip, True, True)()
        gx_t, gp_t = step(tor, True, True)()
        say("same gradients: max |d grad_x| %.2e of max %.2e; worst parameter gradient %.2e of its max"
            % (float((gx_h - gx_t).abs().max()), float(gx_t.abs().max()), max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gp_h, gp_t))))
        gx_f, gp_f = step(half, True, True)()
        gx_a, gp_a = step(auto, True, True, LOSS_SCALE)()
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
        names = [n for n, _ in cnn.named_parameters()]
        worst = max(zip(names, gp_f, gp_t), key=lambda t: rel(t[1], t[2]))[0]
        say("hip float16 against the torch float32 gradients: grad_x %.2e of its max, worst parameter gradient %.2e of its max (%s) (torch autocast with the loss scaled by 2^10: %.2e, %.2e)"
            % (rel(gx_f, gx_t), max(rel(a, b) for a, b in zip(gp_f, gp_t)), worst, rel(gx_a, gx_t), max(rel(a, b) for a, b in zip(gp_a, gp_t))))
        # the same ReLU and pool decisions in the six stages: the float32 unit on the half forward's stages.  What is left is the roundings and the d1 / f decisions;
        # a weight-gradient workgroup of the half unit walks a strip of (tiles of 8 x 16) / 128 tiles here, two in the test frames
        with torch.no_grad():
            _, st16 = hourglass.hourglass_forward(x0, cnn, return_stages=True, precision="float16")
            st16 = {k: v.clone() for k, v in st16.items()}
        hx, hp = hourglass.hourglass_backward(x0, cnn, st16, None, up, precision="float16")
        fx, fp = hourglass.hourglass_backward(x0, cnn, {k: v.float().contiguous() for k, v in st16.items()}, None, up)
        per = {k: rel(hp[k], fp[k]) for k in hp}
        say("hip float16 against the float32 unit on the half forward's stages (strips of %d tiles): grad_x %.2e of its max; parameter gradients %.2e (%s) .. %.2e (%s) of their maxima"
            % (-(-(-(-h // 8) * -(-w // 16)) // 128), rel(hx, fx), min(per.values()), min(per, key=per.get), max(per.values()), max(per, key=per.get)))
        del st16, hx, hp, fx, fp
        del gx_h, gp_h, gx_t, gp_t, gx_f, gp_f, gx_a, gp_a
        r = compare({"hip all": step(hip, True, True), "hip float16 all": step(half, True, True), "torch all": step(tor, True, True), "torch autocast all": step(auto, True, True, LOSS_SCALE),
                     "hip params only": step(hip, False, True), "hip float16 params only": step(half, False, True), "torch params only": step(tor, False, True),
                     "hip input only": step(hip, True, False), "hip float16 input only": step(half, True, False), "torch input only": step(tor, True, False)},
                    args.iters, args.repeats, args.warmup)
        for k in r:
            say("%-26s %8.3f ms [%7.3f .. %7.3f]" % (k, r[k][0], r[k][1], r[k][2]))
        for what in ("all", "params only", "input only"):
            f16, f32 = r["hip float16 " + what], r["hip " + what]
            faster = f16[0] < f32[0]
            verdict16["%s %s" % (size, what)] = faster
            say("forward + backward, %-11s hip float32 / hip float16 %5.2f x (float32 range [%7.3f .. %7.3f])   hip float16 faster: %s%s"
                % (what + ":", f32[0] / f16[0], f32[1], f32[2], faster, "   torch autocast / hip float16 %5.2f x" % (r["torch autocast all"][0] / f16[0]) if what == "all" else ""))
        for what in ("all", "params only", "input only"):
            faster = r["hip " + what][0] < r["torch " + what][0]
            verdict["%s %s" % (size, what)] = faster
            say("forward + backward, %-11s torch float32 / hip %5.2f x   hip faster: %s" % (what + ":", r["torch " + what][0] / r["hip " + what][0], faster))
        lib = hourglass._lib.load()
        flop16_ms = 2 * (MACS + BWD_MACS) * h * w / FP16_FLOPS * 1e3
        route_b, all_b = min_bytes_half_train(h, w)
        byte16_ms = (min_bytes_half(h, w) + all_b) / HBM_BYTES_PER_S * 1e3
        say("floors of hip float16, forward + backward with all gradients: arithmetic (at 2.5 PFLOP/s) %.3f ms = %.0f %% of its time reached; bytes (%.2f GB at 8 TB/s: the forward's "
            "%.2f, the backward's %.2f of which %.2f without the weight gradients' reads) %.3f ms = %.0f %%; kept activations (the half forward's arena) %.2f GB, the backward's arena %.2f GB"
            % (flop16_ms, 100.0 * flop16_ms / r["hip float16 all"][0], (min_bytes_half(h, w) + all_b) / 1e9, min_bytes_half(h, w) / 1e9, all_b / 1e9, route_b / 1e9, byte16_ms,
               100.0 * byte16_ms / r["hip float16 all"][0], lib.ibgs_hgh_required_scratch(h, w) / 1e9, lib.ibgs_hgh_train_required_scratch(h, w) / 1e9))
        floor_ms = 2 * (MACS + BWD_MACS) * h * w / FP32_FLOPS * 1e3
        say("arithmetic floor, forward + backward (%d fma per pixel at 157.3 TFLOP/s) %.3f ms = %.0f %% of the hip time reached; kept activations (the forward's arena) %.2f GB, "
            "the backward's arena %.2f GB" % (round(MACS + BWD_MACS), floor_ms, 100.0 * floor_ms / r["hip all"][0], lib.ibgs_hg_required_scratch(h, w) / 1e9,
                                               lib.ibgs_hgb_required_scratch(h, w) / 1e9))

        def tail(cnn_forward):
            def run():
                for q in net.parameters():
                    q.requires_grad_(True)
                    q.grad = None
                render.grad = warped.grad = None
                if cnn_forward is None:
                    ip = hourglass.fuse_color_train(pkg, net, 3)["image_pred"]
                elif cnn_forward == "float16":
                    with hourglass.train_precision("float16"):
                        ip = hourglass.fuse_color_train(pkg, net, 3)["image_pred"]
                elif cnn_forward in ("scaled", "scaled float16"):
                    with hourglass.train_precision("float16" if cnn_forward == "scaled float16" else "float32"):
                        ip = resample_train.fuse_color_train_scaled(pkg, net, 0.5, 3)["image_pred"]
                else:
                    xi, _ = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
                    ip = cnn_forward(xi)[1]
                (ip * up).sum().backward()
            return run
        r = compare({"fuse_color_train": tail(None), "fuse_color_train float16": tail("float16"), "front end + torch CNN": tail(tor), "scaled 0.5": tail("scaled"),
                     "scaled 0.5 float16": tail("scaled float16")}, args.iters, args.repeats, 3)
        say("the training tail from the rasterizer's planes, forward + backward: fuse_color_train %8.3f ms [%7.3f .. %7.3f]   front end + torch float32 CNN %8.3f ms [%7.3f .. %7.3f]   ratio %5.2f x"
            % (r["fuse_color_train"] + r["front end + torch CNN"] + (r["front end + torch CNN"][0] / r["fuse_color_train"][0],)))
        say("the same tail inside train_precision(\"float16\") %8.3f ms [%7.3f .. %7.3f]   fuse_color_train / float16 %5.2f x"
            % (r["fuse_color_train float16"] + (r["fuse_color_train"][0] / r["fuse_color_train float16"][0],)))
        say("fuse_color_train_scaled at 0.5: float32 %8.3f ms [%7.3f .. %7.3f]   inside train_precision(\"float16\") %8.3f ms [%7.3f .. %7.3f]   float32 / float16 %5.2f x"
            % (r["scaled 0.5"] + r["scaled 0.5 float16"] + (r["scaled 0.5"][0] / r["scaled 0.5 float16"][0],)))
        verdict16["%s fuse_color_train" % size] = r["fuse_color_train float16"][0] < r["fuse_color_train"][0]
        verdict16["%s scaled 0.5" % size] = r["scaled 0.5 float16"][0] < r["scaled 0.5"][0]
        del x0, pkg, render, warped, feat, ray, mask, up
        for q in net.parameters():
            q.grad = None
        torch.cuda.empty_cache()
    say()
    say("hourglass_train + backward faster than the torch float32 composition + autograd: %s" % ", ".join("%s %s" % kv for kv in verdict.items()))
    say("precision=\"float16\" faster than the float32 unit: %s" % ", ".join("%s %s" % kv for kv in verdict16.items()))
    say()
    resource_report(say, "hgtrain")
    resource_report(say, "hghtrain")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    kept = []
    if os.path.exists(args.out):
        for line in open(args.out).read().split("\n"):
            if line.startswith(TRAIN_MARK):
                break
            kept.append(line)
        while kept and not kept[-1].strip():
            kept.pop()
    with open(args.out, "w") as f:
        f.write("\n".join(kept + [""] + lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hourglass.txt"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--sizes", default="1080x1920,720x1280")
    ap.add_argument("--append", action="store_true", help="write the forward's report after the forward reports --out holds instead of replacing them")
    ap.add_argument("--train", action="store_true", help="measure forward + backward (training) instead; replaces the '# --train' part of --out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hourglass.py measures on the GPU; there is none here")
    if args.train:
        return main_train(args)
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/bench_hourglass.py on one %s: the hourglass CNN on the matrix cores (seven launches) against its torch composition (9 conv2d, 2 max_pool2d, 2 interpolate, 3 cat)," % torch.cuda.get_device_name(0))
    say("# one process, no_grad, hipEvents around %d back-to-back calls, median [min .. max] of %d windows after %d warm-up calls each, the candidates alternating" % (args.iters, args.repeats, args.warmup))
    torch.manual_seed(0)
    net = hourglass.ColorAggregationNet().to(dev).requires_grad_(False)
    cnn = net.cnn
    useful = sum(cout * cin * k * k / 4 ** level for (_, cout, cin, k), level in zip(hourglass.LAYERS[:7], (0, 1, 2, 1, 1, 0, 0)))
    issued = sum((cout + 15) // 16 * 16 * ((cin * k * k + 3) // 4 * 4) / 4 ** level for (_, cout, cin, k), level in zip(hourglass.LAYERS[:7], (0, 1, 2, 1, 1, 0, 0)))
    say("# %d multiply-adds per pixel; padding of the 16-wide instruction (Cout 38 -> 48, 19 -> 32, 9 -> 16; K to a multiple of 4): %.1f %% of the 3 x 3 layers' issued products are useful"
        % (round(MACS), 100.0 * useful / issued) + " (the 32-wide form, 38 -> 64: %.1f %%)"
        % (100.0 * useful / sum((cout + 31) // 32 * 32 * ((cin * k * k + 1) // 2 * 2) / 4 ** level for (_, cout, cin, k), level in zip(hourglass.LAYERS[:7], (0, 1, 2, 1, 1, 0, 0)))))
    # the half-precision kernel: the same M padding; K is 9 taps x the input's octets (channels padded to 8 per input of a concatenation) in chunks of four
    octets = lambda name, cin: 2 * ((cin // 2 + 7) // 8) if name in ("dec2", "dec1") else (cin + 7) // 8
    issued16 = sum((cout + 15) // 16 * 16 * 9 * 32 * ((octets(name, cin) + 3) // 4) / 4 ** level for (name, cout, cin, k), level in zip(hourglass.LAYERS[:7], (0, 1, 2, 1, 1, 0, 0)))
    say("# hip float16 (v_mfma_f32_16x16x32_f16; K in chunks of 32 channels, one tap per instruction: 38 channels run as 64, [38 | 38] as 96, 19 and 9 as 32): %.1f %% of the 3 x 3 layers' issued products are useful"
        % (100.0 * useful / issued16))
    verdict, verdict16 = {}, {}
    with torch.no_grad():
        for size in args.sizes.split(","):
            h, w = (int(v) for v in size.split("x"))
            g = torch.Generator().manual_seed(h)
            s = 3
            render = torch.rand((3, h, w), generator=g).to(dev)
            warped = (render[None] + 0.1 * torch.randn((s, 3, h, w), generator=g).to(dev)).clamp(0, 1).reshape(3 * s, h, w).contiguous()
            mask = (torch.rand((s, 1, h, w), generator=g) < 0.6).to(dev)
            feat = ((torch.rand((s, 4, h, w), generator=g).to(dev) + 0.1) * mask).reshape(4 * s, h, w).contiguous()
            ray = F.normalize(torch.randn((3, h, w), generator=g), dim=0).to(dev)
            pkg = {"render": render, "warped_image": warped, "cam_feat": feat, "camera_ray": ray, "min_depth_diff": torch.rand((1, h, w), generator=g).to(dev)}
            x, _ = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
            say()
            say("== (38, %d, %d)" % (h, w))
            r_hip, ip_hip = hourglass.hourglass_forward(x, cnn, render_scale=1.0)
            r_t, ip_t = composed(x, cnn, 1.0)
            say("same results: max |d residual| %.2e of max |residual| %.2e; image_pred is torch's expression on the hip residual bit for bit: %s"
                % (float((r_hip - r_t).abs().max()), float(r_t.abs().max()), bool(torch.equal(ip_hip, 1.0 * x[0, 35:38] + r_hip))))
            del r_hip, ip_hip, r_t, ip_t

            def autocast():
                with torch.autocast("cuda", dtype=torch.float16):
                    return composed(x, cnn, 1.0)
            r_h, ip_h = hourglass.hourglass_forward(x, cnn, render_scale=1.0, precision="float16")
            with torch.autocast("cuda", dtype=torch.float16):
                r_a, _ = composed(x, cnn, 1.0)
            r_t, _ = composed(x, cnn, 1.0)
            say("hip float16: max |residual - torch float32's| %.2e (torch autocast's: %.2e); image_pred is torch's expression on its residual bit for bit: %s"
                % (float((r_h - r_t).abs().max()), float((r_a.float() - r_t).abs().max()), bool(torch.equal(ip_h, 1.0 * x[0, 35:38] + r_h))))
            del r_h, ip_h, r_a, r_t
            r = compare({"hip": lambda: hourglass.hourglass_forward(x, cnn, render_scale=1.0),
                         "hip float16": lambda: hourglass.hourglass_forward(x, cnn, render_scale=1.0, precision="float16"),
                         "torch float32": lambda: composed(x, cnn, 1.0), "torch autocast": autocast}, args.iters, args.repeats, args.warmup)
            flop_ms = 2 * MACS * h * w / FP32_FLOPS * 1e3
            byte_ms = min_bytes(h, w) / HBM_BYTES_PER_S * 1e3
            for k in ("hip", "hip float16", "torch float32", "torch autocast"):
                say("%-16s %8.3f ms [%7.3f .. %7.3f]" % (k, r[k][0], r[k][1], r[k][2]))
            faster = r["hip"][0] < r["torch float32"][0]
            verdict[size] = faster
            say("torch float32 / hip %5.2f x   hip faster than torch float32: %s   (torch autocast / hip %5.2f x)" % (r["torch float32"][0] / r["hip"][0], faster, r["torch autocast"][0] / r["hip"][0]))
            say("floors of the hip forward: arithmetic (%d fma per pixel at 157.3 TFLOP/s) %.3f ms = %.0f %% of its time reached; bytes (%.2f GB at 8 TB/s) %.3f ms = %.0f %%; arena %.2f GB"
                % (round(MACS), flop_ms, 100.0 * flop_ms / r["hip"][0], min_bytes(h, w) / 1e9, byte_ms, 100.0 * byte_ms / r["hip"][0], hourglass._lib.load().ibgs_hg_required_scratch(h, w) / 1e9))

            half = r["hip float16"][0]
            flop16_ms, byte16_ms = 2 * MACS * h * w / FP16_FLOPS * 1e3, min_bytes_half(h, w) / HBM_BYTES_PER_S * 1e3
            ok = half < 0.95 * r["hip"][0] and half < 0.95 * r["torch autocast"][0]
            verdict16[size] = ok
            say("hip / hip float16 %5.2f x   torch autocast / hip float16 %5.2f x   hip float16 faster than both by more than 5 %%: %s" % (r["hip"][0] / half, r["torch autocast"][0] / half, ok))
            say("floors of hip float16: arithmetic (at 2.5 PFLOP/s) %.3f ms = %.0f %% of its time reached; bytes (%.2f GB at 8 TB/s) %.3f ms = %.0f %%; the float32 split's byte floor %.3f ms = %.0f %%; arena %.2f GB"
                % (flop16_ms, 100.0 * flop16_ms / half, min_bytes_half(h, w) / 1e9, byte16_ms, 100.0 * byte16_ms / half, byte_ms, 100.0 * byte_ms / half,
                   hourglass._lib.load().ibgs_hgh_required_scratch(h, w) / 1e9))

            def tail_torch():
                xi, m = coloragg.fuse_color_inputs(pkg, net.front_end, 3)
                return composed(xi, cnn, 1.0)
            r = compare({"fuse_color": lambda: hourglass.fuse_color(pkg, net, 3), "fuse_color float16": lambda: hourglass.fuse_color(pkg, net, 3, precision="float16"),
                         "front end + torch CNN": tail_torch}, args.iters, args.repeats, 3)
            say("the test-time tail from the rasterizer's planes: fuse_color (front end + hip hourglass) %8.3f ms [%7.3f .. %7.3f]   front end + torch float32 CNN %8.3f ms [%7.3f .. %7.3f]   ratio %5.2f x"
                % (r["fuse_color"] + r["front end + torch CNN"] + (r["front end + torch CNN"][0] / r["fuse_color"][0],)))
            say("the same tail with fuse_color(..., precision=\"float16\") %8.3f ms [%7.3f .. %7.3f]   fuse_color / fuse_color float16 %5.2f x"
                % (r["fuse_color float16"] + (r["fuse_color"][0] / r["fuse_color float16"][0],)))
            del x, pkg, render, warped, feat, ray, mask
            torch.cuda.empty_cache()
    say()
    say("the hip hourglass faster than the torch float32 composition: %s" % ", ".join("%s %s" % kv for kv in verdict.items()))
    say("hip float16 faster than both the float32 kernel and torch autocast by more than 5 %%: %s" % ", ".join("%s %s" % kv for kv in verdict16.items()))
    say()
    resource_report(say, "hourglass")
    resource_report(say, "hghalf")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head, rest = [], []
    if args.append and os.path.exists(args.out):          # after the forward reports the file holds, in front of the training report
        head = open(args.out).read().split("\n")
        at = next((i for i, line in enumerate(head) if line.startswith(TRAIN_MARK)), len(head))
        head, rest = head[:at], head[at:]
        while head and not head[-1].strip():
            head.pop()
        while rest and not rest[-1].strip():
            rest.pop()
        head.append("")
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines + ([""] + rest if rest else [])) + "\n")


if __name__ == "__main__":
    main()
