"""The exposure correction (ibgs_amd/exposure.py `exposure_correct`; csrc/exposure.hip) against the reference's torch composition on the device -- the
boolean-mask gather (which waits for the host on the pixel count), `cat`, `torch.linalg.lstsq` on the N x 4 matrix, `einsum`, autograd: the lines of
compute_exposure_affine_matrix as tests/exposure_ref.torch_composition states them -- in ONE process on one MI355X, at (3, 1080, 1920) and (3, 720, 1280),
with about 30 % and with all of the pixels under the mask.  Output: profiles/exposure.txt.

    python tools/bench_exposure.py [--out profiles/exposure.txt] [--iters 10] [--repeats 11]

Per size and density, both ways, alternating:
  forward                    under no_grad (a test frame)
  forward + backward         the gradient of a seeded sum with respect to render (a training iteration's share)
then each kernel alone through the C ABI (the moments, the solve, the apply, the transposed apply) -- its time from `rocprofv3 --kernel-trace --stats` around
a fresh child process that launches nothing else (`--kernels-only`; tracing slows the host, so it is a run of its own), beside the event window -- with its
byte floor from the shapes -- the moments read 7 planes, an apply reads 3 and writes 3: 28 + 24 = 52 B per pixel for the forward -- at 8 TB/s and the
fraction of it reached; `fuse_color` at 1080p with
and without the keyword; and hipcc's register / spill report of the unit.  If `torch.linalg.lstsq` does not run on the device build the composition's solve
is torch's normal equations instead (`torch.linalg.solve` of X^T X), and the output says so.
Timing: hipEvents around `iters` back-to-back calls on the current stream, after a warm-up; the median over `repeats` such windows, and their minimum and
maximum.  A kernel of a few microseconds timed this way is bounded by the host's enqueue rate, not by the device: the output marks those.  A measurement
needs the GPU: without one this script fails."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ibgs_amd import _build, _device, _lib, exposure, hourglass  # noqa: E402

HBM_BYTES_PER_S = 8e12
ENQUEUE_BOUND_US = 12.0          # below this a back-to-back window measures the host's enqueue rate


def composed(render, warped, mask, solver):
    """The reference's lines (color_aggregation_network.py:136-153, 182-185) in float32 torch on the device."""
    _, h, w = render.shape
    valid = mask.reshape(1, h, w)
    first = warped.reshape(-1, 3, h, w)[0] * valid
    with torch.no_grad():
        sel = (valid == 1)[0]
        r_valid, s_valid = render[:, sel], first[:, sel]          # the boolean gather: one host synchronisation on the count
        x = torch.cat([r_valid, torch.ones((1, r_valid.shape[1]), device=render.device, dtype=render.dtype)], 0).T
        affine = solver(x, s_valid.T).T
    aug = torch.cat([render, torch.ones((1, h, w), device=render.device, dtype=render.dtype)], 0)
    return torch.einsum("ij,jhw->ihw", affine, aug), affine


def lstsq_solver(x, y):
    return torch.linalg.lstsq(x, y).solution


def normal_solver(x, y):
    return torch.linalg.solve(x.T @ x, x.T @ y)


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


def resource_report():
    """hipcc's kernel-resource-usage remarks of exposure.hip with the unit's own flags -> lines."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build._hipcc()] + _build.compile_flags("exposure") + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "exposure.hip"), "-o", os.path.join(tmp, "exposure.o")]
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
    return ["  %-44s VGPRs %3d  AGPRs %d  SGPRs %3d  spills %d / %d  scratch %d B/lane  LDS %5d B  occupancy %d waves/SIMD"
            % (k["name"], k.get("vgpr", -1), k.get("agpr", 0), k.get("sgpr", -1), k.get("vspill", -1), k.get("sspill", -1), k.get("scratch", -1), k.get("lds", -1), k.get("occ", -1)) for k in out]


def kernel_calls(dev, h, w, density):
    """-> ({name: callable} of the four launches through the C ABI on seeded inputs, (affine, status))."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(h + int(10 * density))
    render, warped, up = torch.rand((3, h, w), generator=g).to(dev), torch.rand((3, h, w), generator=g).to(dev), torch.randn((3, h, w), generator=g).to(dev)
    u = torch.rand((1, h, w), generator=g)
    mask = torch.where(u < density, 1, torch.where(u < density + (1 - density) / 2, 0, 2)).int().to(dev)
    with torch.cuda.device(dev):
        out, affine, status = torch.empty_like(render), torch.empty((3, 4), device=dev), torch.empty((), dtype=torch.int32, device=dev)
    sc = _device.scratch(dev, lib.ibgs_expo_required_scratch(h, w))
    keep = (render, warped, up, mask, out, sc)
    fit = lambda phases: _device.call(dev, "ibgs_expo_fit", h, w, render.data_ptr(), warped.data_ptr(), mask.data_ptr(), affine.data_ptr(), status.data_ptr(), sc.data_ptr(), sc.numel(), phases)
    fit(_lib.EXPO_FIT)
    return {"expo_moments_kernel": lambda: fit(_lib.EXPO_MOMENTS), "expo_solve_kernel": lambda: fit(_lib.EXPO_SOLVE),
            "expo_apply_kernel": lambda: _device.call(dev, "ibgs_expo_apply", h, w, affine.data_ptr(), status.data_ptr(), render.data_ptr(), out.data_ptr()),
            "expo_apply_kernel (transposed)": lambda: _device.call(dev, "ibgs_expo_apply_backward", h, w, affine.data_ptr(), status.data_ptr(), up.data_ptr(), out.data_ptr())}, (affine, status, keep)


TRACED_CALLS = 40


def kernels_only(h, w, density):
    """The child under rocprofv3: TRACED_CALLS launches of each kernel, nothing else of this unit."""
    calls, (affine, status, _) = kernel_calls(torch.device("cuda"), h, w, density)
    for _ in range(TRACED_CALLS):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    assert int(status) == 1


def traced_kernel_us(h, w, density):
    """Kernel times from `rocprofv3 --kernel-trace --stats` around a fresh child process that only launches the four kernels (a run of its own: tracing
    slows the host, so nothing else is timed under it).  -> {name: average us} with the names of `kernel_calls`, or a string saying why there is none."""
    import csv
    import glob
    import shutil
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "rocprofv3 is not installed"
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--kernels-only", str(h), str(w), str(density)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, cwd=ROOT)
        if done.returncode != 0:
            return "the traced child failed (%d): %s" % (done.returncode, done.stdout.strip().split("\n")[-1][:160])
        rows = [r for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
    out = {}
    for r in rows:
        n = r["Name"]
        for key, pats in (("expo_moments_kernel", ("expo_moments_kernel",)), ("expo_solve_kernel", ("expo_solve_kernel",)), ("expo_apply_kernel", ("expo_apply_kernel<false", "expo_apply_kernelILb0")),
                          ("expo_apply_kernel (transposed)", ("expo_apply_kernel<true", "expo_apply_kernelILb1"))):          # (demangled or not)
            if any(pat in n for pat in pats) and int(r["Calls"]) >= TRACED_CALLS:
                out[key] = float(r["AverageNs"]) / 1e3
    return out if len(out) == 4 else "the trace holds %d of the four kernels (%s)" % (len(out), sorted(r["Name"][:40] for r in rows if "expo_" in r["Name"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", nargs=3, metavar=("H", "W", "DENSITY"), help="launch the four kernels and exit (the child of the traced run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=11)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_exposure.py measures on the GPU; there is none here")
    if args.kernels_only:
        return kernels_only(int(args.kernels_only[0]), int(args.kernels_only[1]), float(args.kernels_only[2]))
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/bench_exposure.py on one %s: exposure_correct (moments, solve, apply) against the reference's torch composition on the device (boolean gather, cat," % torch.cuda.get_device_name(0))
    say("# torch.linalg.lstsq, einsum, autograd), one process, hipEvents around %d back-to-back calls, median [min .. max] of %d windows, the two alternating" % (args.iters, args.repeats))
    solver, solver_name = lstsq_solver, "torch.linalg.lstsq"
    try:
        lstsq_solver(torch.rand(64, 4, device=dev), torch.rand(64, 3, device=dev))
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- whatever the device build raises for a missing solver
        solver, solver_name = normal_solver, "torch.linalg.solve of the normal equations"
        say("# torch.linalg.lstsq is NOT available on this device build (%s: %s): the composition solves the normal equations (X^T X) with torch.linalg.solve instead"
            % (type(e).__name__, str(e).split("\n")[0][:120]))
    say("# the composition's solve: %s" % solver_name)
    verdict = []
    for (h, w) in ((1080, 1920), (720, 1280)):
        for density in (0.3, 1.0):
            g = torch.Generator().manual_seed(h + int(10 * density))
            render = torch.rand((3, h, w), generator=g).to(dev)
            true = torch.tensor([[0.9, 0.06, -0.03], [0.04, 1.1, 0.05], [-0.02, 0.03, 0.8]]).to(dev)
            warped = torch.rand((3, 3, h, w), generator=g).to(dev)
            warped[0] = torch.einsum("ij,jhw->ihw", true, render) + 0.02 + 0.02 * torch.randn((3, h, w), generator=g).to(dev)
            warped = warped.reshape(9, h, w).contiguous()
            u = torch.rand((1, h, w), generator=g)
            mask = torch.where(u < density, 1, torch.where(u < density + (1 - density) / 2, 0, 2)).int().to(dev)
            up = torch.randn((3, h, w), generator=g).to(dev)
            leaf = render.clone().requires_grad_(True)
            say()
            say("== (3, %d, %d), %.1f %% of the pixels under the mask" % (h, w, 100.0 * float((mask == 1).float().mean())))

            def run(fused, grad):
                r = leaf if grad else render
                call = (lambda: exposure.exposure_correct(r, warped, mask)[:2]) if fused else (lambda: composed(r, warped, mask, solver))
                if not grad:
                    with torch.no_grad():
                        return call() + (None,)
                out, a = call()
                return out, a, torch.autograd.grad((out * up).sum(), leaf)[0]

            oc, ac, gc = run(False, True)
            of, af, gf = run(True, True)
            oc, of = oc.detach(), of.detach()
            say("same results: max |d affine| %.2e; max |d corrected| %.2e of max %.2e; max |d grad| %.2e of max %.2e"
                % (float((ac - af).abs().max()), float((oc - of).abs().max()), float(oc.abs().max()), float((gc - gf).abs().max()), float(gc.abs().max())))
            del oc, ac, gc, of, af, gf
            plane = h * w
            for name, grad, nbytes in (("forward (no_grad)", False, (7 + 6) * 4 * plane), ("forward + backward", True, (7 + 6 + 6) * 4 * plane)):
                r = compare({"composed": lambda: run(False, grad), "fused": lambda: run(True, grad)}, args.iters, args.repeats)
                faster = r["fused"][0] < r["composed"][0]
                verdict.append(faster)
                floor_us = nbytes / HBM_BYTES_PER_S * 1e6
                say("%-20s composed %8.3f ms [%7.3f .. %7.3f]   fused %8.3f ms [%7.3f .. %7.3f]   composed / fused %6.1f x   fused faster: %s" % ((name,) + r["composed"] + r["fused"] + (r["composed"][0] / r["fused"][0], faster)))
                say("%-20s byte floor of the fused call: %.1f MB at 8 TB/s = %.1f us = %.0f %% of its time" % ("", nbytes / 1e6, floor_us, 100.0 * floor_us / (r["fused"][0] * 1e3)))
            # each kernel alone, through the C ABI: events here, and the trace of a child process
            calls, (affine, status, keep) = kernel_calls(dev, h, w, density)
            r = compare(calls, 5 * args.iters, args.repeats)
            assert int(status) == 1
            traced = traced_kernel_us(h, w, density)
            if isinstance(traced, str):
                say("  no kernel trace: %s; the times below are event windows over back-to-back launches" % traced)
            partials = (keep[-1].numel() - 128) // (8 * _lib.EXPO_SUMS)
            for name, nbytes in (("expo_moments_kernel", 7 * 4 * plane), ("expo_solve_kernel", 0), ("expo_apply_kernel", 6 * 4 * plane), ("expo_apply_kernel (transposed)", 6 * 4 * plane)):
                window = r[name][0] * 1e3
                us = window if isinstance(traced, str) else traced[name]
                head = "  %-32s %s %7.1f us   (event window over back-to-back launches %6.1f us%s)" % (name, "window" if isinstance(traced, str) else "traced", us, window,
                                                                                                  ": the host's enqueue rate" if window < ENQUEUE_BOUND_US else "")
                if nbytes:
                    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
                    say("%s   floor %5.1f MB at 8 TB/s = %5.1f us = %3.0f %% reached (%.2f TB/s)" % (head, nbytes / 1e6, floor_us, 100.0 * floor_us / us, nbytes / us / 1e6))
                else:
                    say("%s   one workgroup: %d partials of 22 f64, a 4 x 4 solve" % (head, partials))
            if not isinstance(traced, str):
                fwd_floor = 52 * plane / HBM_BYTES_PER_S * 1e6
                total = sum(traced[k] for k in ("expo_moments_kernel", "expo_solve_kernel", "expo_apply_kernel"))
                say("  the three forward kernels %8.1f us traced; the forward's floor 52 B per pixel = %.1f MB = %.1f us = %.0f %% reached" % (total, 52 * plane / 1e6, fwd_floor, 100.0 * fwd_floor / total))
            del calls, keep
            torch.cuda.empty_cache()
    # fuse_color with and without the keyword
    h, w = 1080, 1920
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    net = hourglass.ColorAggregationNet().to(dev)
    render = torch.rand((3, h, w), generator=g).to(dev)
    pkg = {"render": render, "warped_image": (render[None] + 0.1 * torch.randn((3, 3, h, w), generator=g).to(dev)).clamp(0, 1).reshape(9, h, w).contiguous(),
           "cam_feat": (torch.rand((12, h, w), generator=g).to(dev) + 0.1), "camera_ray": torch.nn.functional.normalize(torch.randn((3, h, w), generator=g), dim=0).to(dev),
           "min_depth_diff": torch.rand((1, h, w), generator=g).to(dev), "use_first_src_frame_mask": (torch.rand((1, h, w), generator=g) < 0.3).int().to(dev)}
    say()
    say("== fuse_color at (3, %d, %d), 3 sources, under no_grad" % (h, w))
    for precision in ("float32", "float16"):
        def call(on):
            with torch.no_grad():
                return hourglass.fuse_color(pkg, net, precision=precision, enable_exposure_correction=on)
        r = compare({"off": lambda: call(False), "on": lambda: call(True)}, args.iters, args.repeats)
        say("%-8s without the correction %8.3f ms [%7.3f .. %7.3f]   with it %8.3f ms [%7.3f .. %7.3f]   the correction adds %6.1f us = %.1f %%"
            % ((precision,) + r["off"] + r["on"] + ((r["on"][0] - r["off"][0]) * 1e3, 100.0 * (r["on"][0] / r["off"][0] - 1))))
    say()
    say("exposure_correct faster than the torch composition in every mode at both sizes and densities: %s" % all(verdict))
    say()
    say("hipcc -Rpass-analysis=kernel-resource-usage, %s:" % " ".join(_build.compile_flags("exposure")))
    for line in resource_report():
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
