"""The colour tail at a reduced residual resolution (`hourglass.fuse_color(..., residual_resolution_scale=0.5)`: csrc/resample.hip around the hourglass)
against the reference's torch composition on the device -- the masked feature assembly, three `F.interpolate` over 21 + 3 + 3 planes, the per-view MLP as
two `F.linear`, the CNN as `F.conv2d`, `F.interpolate` back and the image_pred expression -- and against this library's own tail at scale 1, in ONE
process on one MI355X, at (3, 1080, 1920) and (3, 720, 1280) with 3 sources, in float32 and float16 (the torch side under `torch.autocast`, as the
reference renders).  Output: profiles/resample.txt.

    python tools/bench_resample.py [--out profiles/resample.txt] [--iters 5] [--repeats 7]
    python tools/bench_resample.py --train [--out profiles/resample.txt]

`--train` measures TRAINING at the reduced resolution instead (`resample_train.fuse_color_train_scaled`, forward + backward of `(image_pred g).sum()` with render,
warped_image and all 22 parameters requiring grad) against the same torch composition with autograd and against `hourglass.fuse_color_train` at scale 1, then
the two entry points of csrc/rsztrain.hip alone beside their byte floors, and that unit's resource report; it replaces the training section at the end of the
output file and leaves the rest of it alone.

Then each of the two kernels alone through the Python wrappers, beside its byte floor from the shapes at 8 TB/s, the hourglass alone at both resolutions
(the expectation that its time falls with s^2 is only an expectation: the output says what was found), and hipcc's register / spill / LDS report of the unit.
Timing: hipEvents around `iters` back-to-back calls on the current stream, after a warm-up of every shape; the median over `repeats` such windows, their
minimum and maximum, the candidates alternating.  Slower-than-torch cases are printed like the others.  A measurement needs the GPU: without one this script fails."""
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

from ibgs_amd import _build, _device, _lib, hourglass, resample, resample_train  # noqa: E402

HBM_BYTES_PER_S = 8e12
ENQUEUE_BOUND_US = 12.0          # below this a back-to-back window measures the host's enqueue rate


def torch_cnn(x, p):
    """x: (1, 38, h, w); p: the HourglassCNN.  -> residual (3, h, w)"""
    conv = lambda t, name, pad: F.conv2d(t, getattr(p, name + "_w"), getattr(p, name + "_b"), padding=pad)
    e1 = F.relu(conv(x, "enc1", 1))
    e2 = F.relu(conv(F.max_pool2d(e1, 2), "enc2", 1))
    b = F.relu(conv(F.max_pool2d(e2, 2), "enc3", 1))
    u2 = F.relu(conv(F.interpolate(b, size=e2.shape[-2:], mode="nearest"), "up2_conv", 1))
    d2 = F.relu(conv(torch.cat([u2, e2], 1), "dec2", 1))
    u1 = F.relu(conv(F.interpolate(d2, size=e1.shape[-2:], mode="nearest"), "up1_conv", 1))
    d1 = F.relu(conv(torch.cat([u1, e1], 1), "dec1", 1))
    f = F.relu(conv(torch.cat([d1, x], 1), "fuse_input", 0))
    return conv(f, "final", 0)[0]


def composed(pkg, net, s, levels, burned=1.0):
    """The reference's lines (color_aggregation_network.py:187-241) in torch ops on the device, the level count given (the reference reads it back)."""
    render = pkg["render"]
    _, h, w = render.shape
    feat = pkg["cam_feat"].view(-1, 4, h, w).permute(2, 3, 0, 1)[:, :, :levels]
    warped = pkg["warped_image"].view(-1, 3, h, w).permute(2, 3, 0, 1)[:, :, :levels]
    valid = (torch.sum(feat, dim=-1, keepdim=True) > 0.0).float()
    x = torch.cat([(warped - render.permute(1, 2, 0).unsqueeze(2)) * valid, feat], dim=-1)
    resize = lambda t: F.interpolate(t, scale_factor=s, mode="bilinear", align_corners=True)
    x = resize(x.permute(2, 3, 0, 1)).permute(2, 3, 0, 1)
    colour = resize(render.unsqueeze(0)).squeeze(0)
    ray = resize(pkg["camera_ray"].view(3, h, w).unsqueeze(0)).squeeze(0)
    ray = ray / (torch.norm(ray, dim=0, keepdim=True) + 1e-10)
    hr, wr = ray.shape[1:]
    front = net.front_end
    feats = F.relu(F.linear(F.relu(F.linear(x.reshape(-1, 7), front.w1, front.b1)), front.w2, front.b2)).view(hr * wr, levels, -1)
    agg = feats.mean(dim=1) if front.mode == "mean" else feats.max(dim=1).values
    cnn_input = torch.cat([agg.T.view(1, -1, hr, wr), ray.unsqueeze(0).to(agg.dtype), colour.unsqueeze(0).to(agg.dtype)], dim=1)
    residual = torch_cnn(cnn_input, net.cnn).float()
    residual = F.interpolate(residual.unsqueeze(0), size=(h, w), mode="bilinear", align_corners=True).squeeze(0)
    return residual, burned * render + residual


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
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        print("  (warmed up: %s)" % k, flush=True)
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_ms(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def resource_report(unit="resample"):
    """hipcc's kernel-resource-usage remarks of the unit's .hip with the unit's own flags -> lines."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build._hipcc()] + _build.compile_flags(unit) + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, unit + ".hip"), "-o", os.path.join(tmp, unit + ".o")]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    out, cur = [], None
    for line in text.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip() or m.group(1)
            cur = {"name": re.sub(r"\(.*", "", name).replace("void ", "").replace("ibgs::", "")}
            out.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return ["  %-44s VGPRs %3d  AGPRs %2d  SGPRs %3d  spills %d / %d  scratch %d B/lane  LDS %5d B  occupancy %d waves/SIMD"
            % (k["name"], k.get("vgpr", -1), k.get("agpr", 0), k.get("sgpr", -1), k.get("vspill", -1), k.get("sspill", -1), k.get("scratch", -1), k.get("lds", -1), k.get("occ", -1)) for k in out]


TRAIN_MARK = "# ---- training at the reduced resolution (--train)"


def scene(h, w, dev):
    g = torch.Generator().manual_seed(h)
    render = torch.rand((3, h, w), generator=g).to(dev)
    feat = torch.rand((12, h, w), generator=g) * 0.5
    feat = torch.where(torch.rand((3, 1, h, w), generator=g).expand(3, 4, h, w).reshape(12, h, w) < 0.7, feat, torch.zeros(())).to(dev)          # 30 % of the slots invalid
    return {"render": render, "warped_image": (render[None] + 0.1 * torch.randn((3, 3, h, w), generator=g).to(dev)).clamp(0.01, 1).reshape(9, h, w).contiguous(),
            "cam_feat": feat, "camera_ray": F.normalize(torch.randn((3, h, w), generator=g), dim=0).to(dev), "min_depth_diff": torch.rand((1, h, w), generator=g).to(dev)}


def main_train(args):
    dev = torch.device("cuda")
    s = args.scale
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(TRAIN_MARK)
    say("# tools/bench_resample.py --train on one %s: fuse_color_train_scaled(..., %g), forward + backward of (image_pred g).sum() with render, warped_image and the 22" % (torch.cuda.get_device_name(0), s))
    say("# parameters requiring grad, against the torch composition with autograd and against fuse_color_train at scale 1; 3 sources; float32; one process, hipEvents")
    say("# around %d back-to-back steps, median [min .. max] of %d windows, the candidates alternating" % (args.iters, args.repeats))
    torch.manual_seed(7)
    net = hourglass.ColorAggregationNet().to(dev)
    verdict = []
    for (h, w) in ((1080, 1920), (720, 1280)):
        pkg = scene(h, w, dev)
        for k in ("render", "warped_image"):
            pkg[k].requires_grad_(True)
        leaves = [pkg["render"], pkg["warped_image"]] + list(net.parameters())
        up = torch.randn((3, h, w), generator=torch.Generator().manual_seed(w)).to(dev)
        hr, wr = resample.scaled_size(h, w, s)
        plane, plane_r = h * w, hr * wr

        def step(forward):
            def run():
                for t in leaves:
                    t.grad = None
                (forward() * up).sum().backward()
            return run
        fns = {"torch": step(lambda: composed(pkg, net, s, 3)[1]), "scaled": step(lambda: resample_train.fuse_color_train_scaled(pkg, net, s)["image_pred"]),
               "full": step(lambda: hourglass.fuse_color_train(pkg, net)["image_pred"])}
        say()
        say("== (3, %d, %d), 3 sources; the CNN at %d x %d" % (h, w, hr, wr))
        fns["scaled"]()
        mine = [t.grad.clone() for t in leaves]
        fns["torch"]()
        names = ["render", "warped_image"] + [k for k, _ in net.named_parameters()]
        l2 = max((float((a - t.grad).norm() / t.grad.norm()), k) for a, t, k in zip(mine, leaves, names))
        top = max((float((a - t.grad).abs().max() / t.grad.abs().max()), k) for a, t, k in zip(mine, leaves, names))
        # (a ReLU or pool decision that float32 rounding takes the other way changes single pixels of an image gradient by its own size: the max-abs figure of the images counts those)
        say("same gradients (float32) over the 24 tensors: the largest |d grad|_2 / |grad|_2 %.2e (%s); the largest max |d grad| / max |grad| %.2e (%s)" % (l2 + top))
        del mine
        r = compare(fns, args.iters, args.repeats)
        cheaper, faster = r["scaled"][0] < r["full"][0], r["scaled"][0] < r["torch"][0]
        verdict.append(cheaper)
        say("torch composition + autograd at s = %g %8.3f ms [%7.3f .. %7.3f]   fuse_color_train_scaled at s = %g %8.3f ms [%7.3f .. %7.3f]   torch / scaled %6.2f x   scaled faster: %s"
            % ((s,) + r["torch"] + (s,) + r["scaled"] + (r["torch"][0] / r["scaled"][0], faster)))
        say("fuse_color_train at s = 1             %8.3f ms [%7.3f .. %7.3f]   s = 1 / s = %g %6.2f x (pixels: %.2f x)   scaled faster than s = 1: %s"
            % (r["full"] + (s, r["full"][0] / r["scaled"][0], plane / plane_r, cheaper)))
        # the two entry points alone, on buffers made once
        with torch.no_grad():
            front = net.front_end
            levels = resample.count_levels(pkg["warped_image"], 3)
            imgs = [pkg[k].detach() for k in ("render", "warped_image", "cam_feat")]
            pars = [t.detach().contiguous() for t in (front.w1, front.b1, front.w2, front.b2)]
            go = torch.randn((38, hr, wr), device=dev)
            grads = [torch.empty_like(t) for t in imgs[:2] + pars]
            sc = _device.scratch(dev, _lib.load().ibgs_rzt_required_scratch(3, h, w, hr, wr))
            g_res = torch.empty((3, hr, wr), device=dev)
            ptrs = lambda ts: [None if t is None else t.data_ptr() for t in ts]
            features = lambda outs: _device.call(dev, "ibgs_rzt_features_backward", 3, h, w, hr, wr, _lib.RSZ_MEAN, *ptrs(imgs + pars), levels.data_ptr(), go.data_ptr(), *ptrs(outs),
                                                 sc.data_ptr(), sc.numel())
            parts = {"rzt_features_backward, every gradient (3 kernels)": lambda: features(grads),
                     "rzt_features_backward, parameters only (2 kernels)": lambda: features([None, None] + grads[2:]),
                     "rzt_features_backward, images only (2 kernels)": lambda: features(grads[:2] + [None] * 4),
                     "rzt_upsample_backward, one upstream": lambda: _device.call(dev, "ibgs_rzt_upsample_backward", h, w, hr, wr, None, up.data_ptr(), g_res.data_ptr()),
                     "rzt_upsample_backward, both upstreams": lambda: _device.call(dev, "ibgs_rzt_upsample_backward", h, w, hr, wr, up.data_ptr(), up.data_ptr(), g_res.data_ptr())}
            r = compare(parts, 2 * args.iters, args.repeats)
            # reduced kernel: render, warped and cam_feat read about once (24 full planes), grad_out's 32 planes read, 9 planes of gx written; gather: cam_feat (12),
            # gx (9 reduced) and grad_out's 3 colour planes read, 3 + 9 full planes written
            reduced_kernel = 24 * 4 * plane + 32 * 4 * plane_r
            gather = (12 + 12) * 4 * plane + (9 + 3) * 4 * plane_r
            floors = {"rzt_features_backward, every gradient (3 kernels)": reduced_kernel + 9 * 4 * plane_r + gather, "rzt_features_backward, parameters only (2 kernels)": reduced_kernel,
                      "rzt_features_backward, images only (2 kernels)": reduced_kernel + 9 * 4 * plane_r + gather,
                      "rzt_upsample_backward, one upstream": 3 * 4 * (plane + plane_r), "rzt_upsample_backward, both upstreams": 3 * 4 * (2 * plane + plane_r)}
            for name, (med, lo, hi) in r.items():
                floor_us = floors[name] / HBM_BYTES_PER_S * 1e6
                say("  %-52s %8.1f us [%7.1f .. %7.1f]%s   floor %6.1f MB at 8 TB/s = %5.1f us = %3.0f %% reached"
                    % (name, med * 1e3, lo * 1e3, hi * 1e3, "  (the host's enqueue rate)" if med * 1e3 < ENQUEUE_BOUND_US else "", floors[name] / 1e6, floor_us, 100.0 * floor_us / (med * 1e3)))
        del pkg, leaves, up, grads, sc, go, parts, fns
        torch.cuda.empty_cache()
    say()
    if all(verdict):
        say("fuse_color_train_scaled at s = %g faster than fuse_color_train at s = 1 at both sizes: True" % s)
    else:
        say("**fuse_color_train_scaled at s = %g is NOT faster than fuse_color_train at s = 1 at every size: the option misses its purpose there**" % s)
    say()
    say("hipcc -Rpass-analysis=kernel-resource-usage, %s:" % " ".join(_build.compile_flags("rsztrain")))
    for line in resource_report("rsztrain"):
        say(line)
    kept = []
    if os.path.exists(args.out):
        kept = open(args.out).read().split("\n")
        if TRAIN_MARK in kept:
            kept = kept[:kept.index(TRAIN_MARK)]
        while kept and not kept[-1].strip():
            kept.pop()
        kept.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(kept + lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.txt"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--train", action="store_true", help="measure training at the reduced resolution; replaces the training section at the end of --out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU; there is none here")
    if args.train:
        return main_train(args)
    dev = torch.device("cuda")
    s = args.scale
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("# tools/bench_resample.py on one %s: fuse_color(..., residual_resolution_scale=%g) against the reference's torch composition on the device (assembly," % (torch.cuda.get_device_name(0), s))
    say("# three F.interpolate, two F.linear, the CNN as F.conv2d, F.interpolate back) and against fuse_color at scale 1; 3 sources; one process, hipEvents around %d" % args.iters)
    say("# back-to-back calls, median [min .. max] of %d windows, the candidates alternating; float16 = precision=\"float16\" here, torch.autocast(float16) there" % args.repeats)
    torch.manual_seed(7)
    net = hourglass.ColorAggregationNet().to(dev).requires_grad_(False)
    verdict = []
    for (h, w) in ((1080, 1920), (720, 1280)):
        g = torch.Generator().manual_seed(h)
        render = torch.rand((3, h, w), generator=g).to(dev)
        feat = torch.rand((12, h, w), generator=g) * 0.5
        feat = torch.where(torch.rand((3, 1, h, w), generator=g).expand(3, 4, h, w).reshape(12, h, w) < 0.7, feat, torch.zeros(())).to(dev)          # 30 % of the slots invalid
        pkg = {"render": render, "warped_image": (render[None] + 0.1 * torch.randn((3, 3, h, w), generator=g).to(dev)).clamp(0.01, 1).reshape(9, h, w).contiguous(),
               "cam_feat": feat, "camera_ray": F.normalize(torch.randn((3, h, w), generator=g), dim=0).to(dev), "min_depth_diff": torch.rand((1, h, w), generator=g).to(dev)}
        hr, wr = resample.scaled_size(h, w, s)
        plane, plane_r = h * w, hr * wr
        say()
        say("== (3, %d, %d), 3 sources; the CNN at %d x %d" % (h, w, hr, wr))
        with torch.no_grad():
            ours = hourglass.fuse_color(pkg, net, residual_resolution_scale=s)
            theirs = composed(pkg, net, s, 3)
            say("same results (float32): max |d residual| %.2e of max %.2e; max |d image_pred| %.2e" % (float((ours["residual"] - theirs[0]).abs().max()), float(theirs[0].abs().max()),
                                                                                                      float((ours["image_pred"] - theirs[1]).abs().max())))
            del ours, theirs
            for precision in ("float32", "float16"):
                def torch_tail():
                    with torch.autocast("cuda", dtype=torch.float16, enabled=precision == "float16"):
                        return composed(pkg, net, s, 3)
                r = compare({"torch": torch_tail, "scaled": lambda: hourglass.fuse_color(pkg, net, precision=precision, residual_resolution_scale=s),
                             "full": lambda: hourglass.fuse_color(pkg, net, precision=precision)}, args.iters, args.repeats)
                faster = r["scaled"][0] < r["torch"][0]
                verdict.append(faster)
                say("%-8s torch composition at s = %g %8.3f ms [%7.3f .. %7.3f]   fuse_color at s = %g %8.3f ms [%7.3f .. %7.3f]   torch / fuse_color %6.2f x   fuse_color faster: %s"
                    % ((precision, s) + r["torch"] + (s,) + r["scaled"] + (r["torch"][0] / r["scaled"][0], faster)))
                say("%-8s fuse_color at s = 1      %8.3f ms [%7.3f .. %7.3f]   s = 1 / s = %g %6.2f x (pixels: %.2f x)" % (("",) + r["full"] + (s, r["full"][0] / r["scaled"][0], plane / plane_r)))
            # the parts of the scaled tail, each alone
            front = net.front_end
            levels = resample.count_levels(pkg["warped_image"], 3)
            x = resample.resized_features(render, pkg["warped_image"], pkg["cam_feat"], pkg["camera_ray"], front.w1, front.b1, front.w2, front.b2, (hr, wr), levels)
            x_full = front(render, pkg["warped_image"], pkg["cam_feat"], pkg["camera_ray"], 3)[0]
            res = hourglass.hourglass_forward(x, net.cnn)
            parts = {"count_levels (cagg_levels_kernel)": lambda: resample.count_levels(pkg["warped_image"], 3),
                     "resized_features (rsz_features_kernel)": lambda: resample.resized_features(render, pkg["warped_image"], pkg["cam_feat"], pkg["camera_ray"], front.w1, front.b1, front.w2,
                                                                                                 front.b2, (hr, wr), levels),
                     "per_view_features at s = 1 (cagg_fwd_kernel)": lambda: front(render, pkg["warped_image"], pkg["cam_feat"], pkg["camera_ray"], levels=levels),
                     "hourglass float32 at %d x %d" % (hr, wr): lambda: hourglass.hourglass_forward(x, net.cnn),
                     "hourglass float32 at %d x %d" % (h, w): lambda: hourglass.hourglass_forward(x_full, net.cnn),
                     "hourglass float16 at %d x %d" % (hr, wr): lambda: hourglass.hourglass_forward(x, net.cnn, precision="float16"),
                     "hourglass float16 at %d x %d" % (h, w): lambda: hourglass.hourglass_forward(x_full, net.cnn, precision="float16"),
                     "upsample_residual (rsz_upsample_kernel)": lambda: resample.upsample_residual(res, render, 1.0)}
            r = compare(parts, 2 * args.iters, args.repeats)
            # features: 27 full-resolution planes read (about once each at s <= 1: the taps of neighbouring reduced pixels tile the frame), 38 reduced planes written
            floors = {"resized_features (rsz_features_kernel)": (3 + 3 * 7 + 3) * 4 * (plane if s <= 1 else 4 * plane_r) + 38 * 4 * plane_r,
                      "per_view_features at s = 1 (cagg_fwd_kernel)": (3 + 3 * 7 + 3 + 38) * 4 * plane,
                      "upsample_residual (rsz_upsample_kernel)": 3 * 4 * plane_r + (3 + 6) * 4 * plane, "count_levels (cagg_levels_kernel)": 9 * 4 * plane}
            for name, (med, lo, hi) in r.items():
                head = "  %-48s %8.1f us [%7.1f .. %7.1f]%s" % (name, med * 1e3, lo * 1e3, hi * 1e3, "  (the host's enqueue rate)" if med * 1e3 < ENQUEUE_BOUND_US else "")
                if name in floors:
                    floor_us = floors[name] / HBM_BYTES_PER_S * 1e6
                    head += "   floor %6.1f MB at 8 TB/s = %5.1f us = %3.0f %% reached" % (floors[name] / 1e6, floor_us, 100.0 * floor_us / (med * 1e3))
                say(head)
            for precision in ("float32", "float16"):
                a, b = r["hourglass %s at %d x %d" % (precision, h, w)][0], r["hourglass %s at %d x %d" % (precision, hr, wr)][0]
                say("  hourglass %s: full / reduced %5.2f x for %.2f x the pixels" % (precision, a / b, plane / plane_r))
            del x, x_full, res, parts
        torch.cuda.empty_cache()
    say()
    say("fuse_color at s = %g faster than the torch composition in both precisions at both sizes: %s" % (s, all(verdict)))
    say()
    say("hipcc -Rpass-analysis=kernel-resource-usage, %s:" % " ".join(_build.compile_flags("resample")))
    for line in resource_report():
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
