"""The frame export (ibgs_amd/frame_export.py `export_frame` + `to_host`; csrc/export.hip) against the reference's host composition -- every plane copied to
the host, save_image's arithmetic, the residual's normalisation, the normal map, and colorize with np.percentile and matplotlib's lookup, as the second loop
of render.py writes them -- in ONE process on one MI355X, at 1080p and 720p.  Output: profiles/export.txt.

    python tools/bench_export.py [--out profiles/export.txt] [--iters 10] [--repeats 11]

Per size:
  the frame            export_frame + to_host (six images, one copy of 6 H W 3 bytes) against the host composition (13 float planes copied, about a dozen host passes,
                       a full sort inside np.percentile); wall clock, both end with the bytes on the host
  the device part      export_frame alone, hipEvents; then the select chain (`percentile`) and the writer (a frame whose depth bounds are given and which has no
                       residual: one launch) alone, each beside its byte floor from the shapes at 8 TB/s
  each kernel          from `rocprofv3 --kernel-trace --stats` around a fresh child process that only runs export_frame (`--kernels-only`)
  select or sort       the select chain against a full sort of the same H W keys with the project's radix sort (api.hip's tests-only entry) and with torch.sort
and hipcc's register / spill report of the unit.
Timing: after a warm-up, the median over `repeats` windows of `iters` back-to-back calls (hipEvents for device work, perf_counter around calls that end on the
host), and their minimum and maximum; the sides of a comparison alternate.  A measurement needs the GPU: without one this script fails."""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ibgs_amd import _build, _lib  # noqa: E402
from ibgs_amd import frame_export as fe  # noqa: E402

HBM_BYTES_PER_S = 8e12
TRACED_CALLS = 30
KERNELS = ("fexp_hist_kernel<0>", "fexp_narrow_kernel<0>", "fexp_hist_kernel<1>", "fexp_narrow_kernel<1>", "fexp_hist_kernel<2>", "fexp_narrow_kernel<2>", "fexp_write_kernel")


def package(h, w, dev):
    g = torch.Generator().manual_seed(h)
    depth = torch.from_numpy(np.random.default_rng(h).gamma(2.0, 1.5, (1, h, w)).astype(np.float32))
    depth[0, ::3, :] = 0          # a third of the pixels at 0
    depth[0, :8, :64] = -99
    t = dict(render=torch.rand((3, h, w), generator=g), gt=torch.rand((3, h, w), generator=g), image_pred=torch.rand((3, h, w), generator=g),
             residual=0.1 * torch.randn((3, h, w), generator=g), normal=torch.nn.functional.normalize(torch.randn((3, h, w), generator=g), dim=0), depth=depth)
    return {k: v.to(dev) for k, v in t.items()}


def export(d, lut):
    return fe.export_frame(dict(render=d["render"], median_intersected_depth=d["depth"], rendered_normal=d["normal"]), dict(image_pred=d["image_pred"], residual=d["residual"]), d["gt"], lut)


def host_composition(d, cmap):
    """render.py:221-249 for a test view, with the file writes left out: what reaches the encoders."""
    save = lambda t: t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()          # torchvision.utils.save_image
    vis = torch.abs(d["residual"])
    vis = vis / torch.max(vis)
    out = {"gt": save(d["gt"]), "render": save(d["render"]), "aggregate": save(d["image_pred"]), "residual": save(vis)}
    value = d["depth"].detach().cpu().numpy().squeeze()          # colorize
    invalid = value == -99
    mask = np.logical_not(invalid)
    vmin, vmax = np.percentile(value[mask], 2), np.percentile(value[mask], 85)
    value = (value - vmin) / (vmax - vmin) if vmin != vmax else value * 0.0
    value[invalid] = np.nan
    img = cmap(value, bytes=True)
    img[invalid] = (128, 128, 128, 255)
    out["depth"] = img[:, :, :3]
    normal = (d["normal"].permute(1, 2, 0).detach().cpu() + 1) / 2
    out["normal"] = (normal.numpy() * 255).clip(0, 255).astype(np.uint8)
    return out


def window_ms(fn, iters, events):
    if events:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def compare(fns, iters, repeats, events=True):
    """fns: {name: callable}.  Warm-up, then `repeats` windows of each, alternating.  -> {name: (median, min, max) ms per call}"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_ms(fn, iters, events))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def resource_report():
    """hipcc's kernel-resource-usage remarks of export.hip with the unit's own flags -> lines."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build._hipcc()] + _build.compile_flags("export") + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "export.hip"), "-o", os.path.join(tmp, "export.o")]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    out, cur = [], None
    for line in text.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip() or m.group(1)
            cur = {"name": re.sub(r"\(.*", "", name).replace("void ", "").replace("ibgs::", "")}
            out.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return ["  %-28s VGPRs %3d  SGPRs %3d  spills %d / %d  scratch %d B/lane  LDS %5d B  occupancy %d waves/SIMD"
            % (k["name"], k.get("vgpr", -1), k.get("sgpr", -1), k.get("vspill", -1), k.get("sspill", -1), k.get("scratch", -1), k.get("lds", -1), k.get("occ", -1)) for k in out]


def kernels_only(h, w):
    """The child under rocprofv3: TRACED_CALLS frames, nothing else of this unit."""
    dev = torch.device("cuda")
    d, lut = package(h, w, dev), fe.colormap_lut("magma_r", dev)
    for _ in range(TRACED_CALLS):
        frame = export(d, lut)
    torch.cuda.synchronize()
    assert int(frame["status"]) == 0


def traced_kernel_us(h, w):
    """-> {kernel: average us} from `rocprofv3 --kernel-trace --stats` around a fresh child (tracing slows the host: a run of its own), or a string saying why not."""
    import csv
    import glob
    import shutil
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "rocprofv3 is not installed"
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--kernels-only", str(h), str(w)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, cwd=ROOT)
        if done.returncode != 0:
            return "the traced child failed (%d): %s" % (done.returncode, done.stdout.strip().split("\n")[-1][:160])
        rows = [r for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
    out = {}
    for r in rows:
        n = r["Name"]
        for key in KERNELS:
            base, _, arg = key.partition("<")
            pats = (key, "%sILi%sE" % (base, arg.rstrip(">"))) if arg else (key,)          # (demangled or not)
            if any(p in n for p in pats) and int(r["Calls"]) >= TRACED_CALLS:
                out[key] = float(r["AverageNs"]) / 1e3
    return out if len(out) == len(KERNELS) else "the trace holds %d of the %d kernels (%s)" % (len(out), len(KERNELS), sorted(r["Name"][:40] for r in rows if "fexp_" in r["Name"]))


def sort_calls(depth):
    """-> {name: callable}: the H W keys of the depth map through the project's radix sort and through torch.sort (values sorted as floats)."""
    lib = _lib.load()
    sz, vp, i32 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int32
    lib.ibgs_debug_sort_scratch_elems.restype, lib.ibgs_debug_sort_scratch_elems.argtypes = sz, [sz]
    lib.ibgs_debug_sort_pairs.restype, lib.ibgs_debug_sort_pairs.argtypes = i32, [vp, vp, vp, vp, vp, sz, i32, vp, sz, vp, vp]
    flat = depth.reshape(-1)
    n = flat.numel()
    bits = flat.view(torch.int32)
    keys = torch.where(bits < 0, ~bits, bits | -2 ** 31)          # the select's order-preserving key (as int32 bit patterns)
    k0, k1, v0, v1 = keys.clone(), torch.empty_like(keys), torch.arange(n, dtype=torch.int32, device=depth.device), torch.empty_like(keys)
    elems = lib.ibgs_debug_sort_scratch_elems(n)
    scratch = torch.empty(elems, dtype=torch.int32, device=depth.device)

    def radix():
        k0.copy_(keys)
        rc = lib.ibgs_debug_sort_pairs(torch.cuda.current_stream().cuda_stream, k0.data_ptr(), k1.data_ptr(), v0.data_ptr(), v1.data_ptr(), n, 32, scratch.data_ptr(), elems, None, None)
        assert rc >= 0, _lib.last_error()
    return {"the project's radix sort (32-bit keys, with the copy of the keys in front and its own wait for the look-back flag)": radix, "torch.sort": lambda: torch.sort(flat)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", nargs=2, metavar=("H", "W"), help="run export_frame and exit (the child of the traced run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=11)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_export.py measures on the GPU; there is none here")
    if args.kernels_only:
        return kernels_only(int(args.kernels_only[0]), int(args.kernels_only[1]))
    import matplotlib
    dev = torch.device("cuda")
    lut, cmap = fe.colormap_lut("magma_r", dev), matplotlib.colormaps["magma_r"]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/bench_export.py on one %s: export_frame + to_host against the reference's host composition (render.py:221-249: .cpu() of every plane, save_image's" % torch.cuda.get_device_name(0))
    say("# arithmetic, np.percentile, matplotlib's lookup, the casts), one process, numpy %s, matplotlib %s; median [min .. max] of %d windows of %d calls, the sides alternating"
        % (np.__version__, matplotlib.__version__, args.repeats, args.iters))
    for (h, w) in ((1080, 1920), (720, 1280)):
        plane = h * w
        d = package(h, w, dev)
        say()
        say("== %d x %d: render, gt, aggregate, residual, depth, normal" % (h, w))
        frame = export(d, lut)
        pinned = torch.empty(frame["packed"].numel(), dtype=torch.uint8, pin_memory=True)
        mine, theirs = fe.to_host(frame, pinned), host_composition(d, cmap)
        say("same images: " + ", ".join("%s %d of %d bytes differ" % (k, int((mine[k] != theirs[k]).sum()), theirs[k].size) for k in sorted(theirs)) + "; status %d" % mine["status"])
        r = compare({"host": lambda: host_composition(d, cmap), "device": lambda: fe.to_host(export(d, lut), pinned)}, max(args.iters // 5, 2), args.repeats, events=False)
        say("the frame on the host (wall clock)    host composition %9.3f ms [%8.3f .. %8.3f]   export_frame + to_host %8.3f ms [%7.3f .. %7.3f]   %6.1f x"
            % (r["host"] + r["device"] + (r["host"][0] / r["device"][0],)))
        say("                                      copied to the host: 13 float planes = %.1f MB against %.1f MB of bytes" % (13 * 4 * plane / 1e6, frame["packed"].numel() / 1e6))
        full_bytes = (3 * 4 * 4 + 4 + 3 * 4) * plane + 3 * 4 * plane + 3 * 4 * plane + 6 * 3 * plane          # writer: 16 planes in, 18 bytes out; pass 0: depth + residual; passes 1, 2: depth
        writer_bytes = (3 * 4 * 4 + 4) * plane + 5 * 3 * plane
        select_bytes = 3 * 4 * plane

        def writer_only():          # five images, no residual, the depth's bounds given: the status memset and ONE launch
            st = torch.empty(1, dtype=torch.int32, device=dev)
            imgs = [(d[k], out_w[i], mode, False) for i, (k, mode) in enumerate((("render", _lib.FEXP_ROUND), ("gt", _lib.FEXP_ROUND), ("image_pred", _lib.FEXP_ROUND), ("normal", _lib.FEXP_NORMAL),
                                                                                   ("depth", _lib.FEXP_COLORIZE)))]
            fe._run(dev, h, w, imgs, st, dict(lut=lut, mask=None, invalid_val=-99.0, vmin=0.1, vmax=5.0, background=(128, 128, 128)))
        out_w = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(5)]
        r = compare({"frame": lambda: export(d, lut), "select": lambda: fe.percentile(d["depth"], (2, 85), invalid_val=-99.0), "writer": writer_only,
                     "quantize": lambda: fe.quantize(d["render"])}, args.iters, args.repeats)
        for name, what, nbytes in (("frame", "export_frame (memset, 3 histogram + 3 narrow launches, writer)", full_bytes), ("select", "percentile: the select chain alone (7 launches)", select_bytes),
                                   ("writer", "the writer alone: 5 images, bounds given (1 launch)", writer_bytes), ("quantize", "quantize (3 planes, float to float)", 2 * 3 * 4 * plane)):
            floor_us = nbytes / HBM_BYTES_PER_S * 1e6
            say("  %-72s %8.1f us [%7.1f .. %7.1f]   floor %6.1f MB at 8 TB/s = %5.1f us = %3.0f %% reached" % ((what,) + tuple(1e3 * v for v in r[name]) + (nbytes / 1e6, floor_us, 100.0 * floor_us / (1e3 * r[name][0]))))
        traced = traced_kernel_us(h, w)
        if isinstance(traced, str):
            say("  no kernel trace: %s" % traced)
        else:
            floors = {"fexp_hist_kernel<0>": (4 + 12) * plane, "fexp_hist_kernel<1>": 4 * plane, "fexp_hist_kernel<2>": 4 * plane, "fexp_write_kernel": (3 * 4 * 4 + 4 + 3 * 4) * plane + 6 * 3 * plane}
            for k in KERNELS:
                if k in floors:
                    fl = floors[k] / HBM_BYTES_PER_S * 1e6
                    say("    traced %-24s %7.1f us   floor %6.1f MB = %5.1f us = %3.0f %% reached (%.2f TB/s)" % (k, traced[k], floors[k] / 1e6, fl, 100.0 * fl / traced[k], floors[k] / traced[k] / 1e6))
                else:
                    say("    traced %-24s %7.1f us   one workgroup: a scan of %d bins per rank" % (k, traced[k], 1024 if k.endswith("<2>") else 2048))
            say("    traced kernels of a frame, summed: %.1f us" % sum(traced.values()))
        # select or sort
        sorts = sort_calls(d["depth"])
        r2 = compare(dict(sorts, select=lambda: fe.percentile(d["depth"], (2, 85), invalid_val=-99.0)), args.iters, args.repeats)
        say("  two percentiles of %d keys:" % plane)
        for k in r2:
            say("    %-118s %8.1f us [%7.1f .. %7.1f]%s" % ((("the select chain" if k == "select" else k),) + tuple(1e3 * v for v in r2[k]) + ("" if k == "select" else "   %5.1f x the select" % (r2[k][0] / r2["select"][0]),)))
        del d, frame, out_w
        torch.cuda.empty_cache()
    say()
    say("hipcc -Rpass-analysis=kernel-resource-usage, %s:" % " ".join(_build.compile_flags("export")))
    for line in resource_report():
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
