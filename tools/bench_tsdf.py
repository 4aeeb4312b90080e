"""TSDF fusion + marching cubes on the MI355X (ibgs_amd/tsdf.py): the surface scene (tests/scenes.surface_discs) rendered at 1080p from N views,
fused at voxel sizes where the ground square spans ~1024 and ~2048 voxels, then meshed.  Output: profiles/tsdf.txt.

    python tools/bench_tsdf.py [--views 16] [--gaussians 400000] [--kstats DIR]

Per voxel size: ms per view of integrate (hipEvents around the call: allocation + update), with and without the allocation's LDS dedup;
active blocks per view; the update's bytes (20 B read + 20 B written per voxel of an active block) over its time against 8 TB/s; extract_mesh ms, V, F;
then, on the extracted mesh, mesh.cluster_connected_triangles and mesh.post_process_mesh (ibgs_amd/mesh.py): ms, C, V', F'.
`--kstats DIR --kstats-only [--active N]`: the per-kernel times of a `rocprofv3 --kernel-trace -d DIR -- python tools/bench_tsdf.py --spans S
--no-ab --no-restatement` run of this script, which split the call into allocation and update (and the update's bytes per second at N active blocks; with `--faces F`
the edge kernel's edges per second).  Last, the numpy restatement (tests/tsdf_ref.py) at 160 x 120, 24 views, and, with `--mesh-restatement`, the
numpy + scipy restatement of the post-processing (tests/mesh_ref.py) on the first span's mesh, for context (host time).
`--mesh-eval`: every stage of ibgs_amd/mesh_eval.py on each span's post-processed mesh (density = a third of the voxel, so that the triangles are sampled,
not only their vertices; max_dist = 100 densities, DTU's ratio; the
ground truth is the thinned sampling of the raw mesh at 1.5 densities), and sklearn's kd-tree (the reference's engine, n_jobs = 16) on `--mesh-eval-host`
points of the same clouds, a size the host finishes.
`--tnt`: ibgs_amd/registration.py on each span's post-processed mesh: its vertices, moved by the inverse of a planted similarity, against the thinned
sampling of the raw mesh inside a polygon volume that cuts off one corner (tau = two thirds of the voxel): every stage's time, the time of one ICP
iteration, the whole evaluate_tnt, and the numpy restatement (tests/registration_ref.py) on `--mesh-eval-host` points of the same clouds.
`--dtu`: ibgs_amd/dtu.py on each span's meshes: dilate_masks for 49 object masks of 1600 x 1200 at radius 24 (an ellipse each), cull_vertices and cull_mesh of the
raw mesh against them (49 cameras on two rings around the mesh), the two point filters on the sampled cloud, the whole evaluate_dtu on the post-processed mesh
(density = a third of the voxel, max_dist = 100 densities, gt = the thinned sampling of the raw mesh), and the numpy restatement (tests/dtu_ref.py) of the
dilation on one mask and of the vertex rule on `--mesh-eval-host` vertices, for information."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ibgs_amd import _lib, dtu, mesh as meshpp, mesh_eval, registration, renderer, simple_scene, synthetic as syn, tsdf  # noqa: E402
from tests import scenes  # noqa: E402

HBM_BYTES_PER_S = 8e12
KERNEL_FILTER = ("tsdf_", "mesh_", "meval_", "pcreg_", "dtu_", "scan_chunk_kernel", "scan_add_kernel")


def render_views(n, W, H, P, dev):
    g = scenes.surface_discs(P, seed=3)
    pc = simple_scene.SimpleGaussians(g, sh_degree=2, device=dev)
    cams = []
    for i in range(n):
        el = 25.0 if i % 2 == 0 else 55.0
        cams.append(simple_scene.SimpleCamera(syn.make_camera(W, H, azimuth_deg=360.0 * i / n, elevation_deg=el, radius=4.0), uid=i, device=dev))
    for c in cams:
        c.nearest_id = []
    scene = simple_scene.SimpleScene(cams, device=dev)
    pipe, args = simple_scene.default_pipe(), simple_scene.default_args()
    views = []
    with torch.no_grad():
        for c in cams:
            out = renderer.render(c, pc, scene, pipe, args, torch.zeros(3, device=dev), learnt_normal=True, nb_src_frames=3, buffer_length=4,
                                  render_geo=True, return_depth_normal=False)
            views.append((c, tsdf.depth_for_fusion(out, c, max_depth=8.0), out["render"].detach().contiguous()))
    torch.cuda.synchronize()
    return views


def kernel_split(kdir):
    """{kernel: (calls, median us)} of the tsdf_ and mesh_ kernels (and the scans the mesh unit launches) from a rocprofv3 --kernel-trace output directory
    (rocpd database or CSV)."""
    durs = {}
    mine = lambda name: any(k in name for k in KERNEL_FILTER)
    for f in glob.glob(os.path.join(kdir, "**", "*.db"), recursive=True):
        import sqlite3
        for name, ns in sqlite3.connect(f).execute("select name, duration from kernels"):
            if mine(name):
                durs.setdefault(name.split("(")[0].split("::")[-1].split(" ")[-1], []).append(ns / 1e3)
    for f in glob.glob(os.path.join(kdir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if mine(row.get("Kernel_Name", "")):
                name = row["Kernel_Name"].split("(")[0].split("::")[-1].split(" ")[-1]
                durs.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: (len(v), float(np.median(v))) for k, v in durs.items()}


def print_split(kdir, active=None, faces=None):
    ks = kernel_split(kdir)
    print("\nkernel times from %s (rocprofv3 --kernel-trace; calls, median us):" % kdir)
    for k, (n, us) in sorted(ks.items()):
        print("  %-26s %6d calls  %9.2f us" % (k, n, us))
    if active and "tsdf_integrate_kernel" in ks:
        us = ks["tsdf_integrate_kernel"][1]
        b = active * 512 * 40
        print("  update at %d active blocks: %.1f MB in %.1f us = %.2f TB/s = %.0f %% of 8 TB/s" % (active, b / 1e6, us, b / (us * 1e-6) / 1e12,
                                                                                                  100 * b / (us * 1e-6) / HBM_BYTES_PER_S))
    if faces and "mesh_edge_union_kernel" in ks:
        us = ks["mesh_edge_union_kernel"][1]
        print("  edge table at %d faces: %.1f M edges (a load, a CAS for an edge's first arrival, an atomicMin, a union for the later ones) = %.2f G edges/s; each a random"
              " 16-byte slot, one 64-byte line in and out = %.2f TB/s = %.0f %% of 8 TB/s" % (faces, 3 * faces / 1e6, 3 * faces / (us * 1e-6) / 1e9, 3 * faces * 128 / (us * 1e-6) / 1e12,
                                                                                             100 * 3 * faces * 128 / (us * 1e-6) / HBM_BYTES_PER_S))


def bench_mesh_eval(raw, post, voxel, host_points):
    """Stage times (hipEvents around the Python calls, median of 3 after a warm-up, read-backs included) and the host engine's on a subsample."""
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, reps=3):
        out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = ev(), ev()
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), out

    density = voxel / 3
    max_dist = 100 * density
    gt_cloud = mesh_eval.sample_surface(raw, 1.5 * density)
    gt = gt_cloud[mesh_eval.downsample(gt_cloud, 1.5 * density)]
    del gt_cloud
    r = {"density": density, "F": int(post.faces.shape[0]), "gt": int(gt.shape[0])}
    r["sample_ms"], cloud = timed(lambda: mesh_eval.sample_surface(post, density))
    order = torch.randperm(cloud.shape[0], device=cloud.device)
    r["thin_ms"], keep = timed(lambda: mesh_eval.downsample(cloud, density, order=order))
    thinned = cloud[keep]
    r["sampled"], r["thinned"] = int(cloud.shape[0]), int(thinned.shape[0])
    state = torch.zeros(_lib.MEVAL_STATE_WORDS, dtype=torch.int32, device=cloud.device)
    r["build_ms"], index = timed(lambda: mesh_eval._Index(gt, state))
    r["d2s_ms"], _ = timed(lambda: index.query(thinned, max_dist))
    r["nearest_s2d_ms"], _ = timed(lambda: mesh_eval.nearest(gt, thinned, max_dist))
    r["chamfer_ms"], c = timed(lambda: mesh_eval.chamfer(thinned, gt, max_dist))
    r["fscore_ms"], f = timed(lambda: mesh_eval.fscore(thinned, gt, 2 * density))
    r["evaluate_ms"], e = timed(lambda: mesh_eval.evaluate_mesh(post, gt, density=density, max_dist=max_dist))
    r["chamfer"], r["fscore"], r["evaluate"] = c, f, e
    if host_points:
        import sklearn.neighbors as skln
        n = min(host_points, cloud.shape[0], gt.shape[0])
        hc, hg = cloud[order[:n]].cpu().numpy().astype(np.float64), gt[:n].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        eng = skln.NearestNeighbors(n_neighbors=1, radius=density, algorithm="kd_tree", n_jobs=16).fit(hc)
        lists = eng.radius_neighbors(hc, radius=density, return_distance=False)
        t1 = time.perf_counter()
        mask = np.ones(n, bool)
        for i, near in enumerate(lists):
            if mask[i]:
                mask[near] = False
                mask[i] = True
        t2 = time.perf_counter()
        eng.fit(hg)
        eng.kneighbors(hc[mask], n_neighbors=1, return_distance=True)
        t3 = time.perf_counter()
        dev_thin, dkeep = timed(lambda: mesh_eval.downsample(cloud[order[:n]].contiguous(), density))
        sub, gsub = cloud[order[:n]][dkeep].contiguous(), gt[:n].contiguous()
        dev_nn, _ = timed(lambda: mesh_eval.nearest(sub, gsub, max_dist))
        r["host"] = {"n": n, "radius_lists_s": t1 - t0, "loop_s": t2 - t1, "kneighbors_s": t3 - t2, "kept": int(mask.sum()), "dev_thin_ms": dev_thin,
                     "dev_nearest_ms": dev_nn, "mask_diff": int((mask != dkeep.cpu().numpy()).sum())}
    return r


def print_mesh_eval(r):
    print("mesh_eval on the post-processed mesh (F %d), density %.6f, max_dist = 100 densities, gt %d points:" % (r["F"], r["density"], r["gt"]))
    print("  sample_surface (count + 64-bit scan + read-back + emit + read-back): %.3f ms -> %d points" % (r["sample_ms"], r["sampled"]))
    print("  downsample, shuffled order (keys + torch.sort + hierarchy + rounds, one read-back per batch): %.3f ms -> %d kept" % (r["thin_ms"], r["thinned"]))
    print("  hierarchy over gt (keys + torch.sort + gather + boxes): %.3f ms; pred -> gt queries on it (keys + torch.sort + walk): %.3f ms"
          % (r["build_ms"], r["d2s_ms"]))
    print("  nearest(gt, pred) (hierarchy + queries + read-back): %.3f ms" % r["nearest_s2d_ms"])
    print("  chamfer (both directions + sums + one read-back): %.3f ms; fscore at 2 densities: %.3f ms" % (r["chamfer_ms"], r["fscore_ms"]))
    print("  evaluate_mesh (all of the above from the mesh): %.3f ms" % r["evaluate_ms"])
    c, f = r["chamfer"], r["fscore"]
    print("  mean_d2s %.6g (%d) mean_s2d %.6g (%d) overall %.6g; precision %.4f recall %.4f F %.4f" % (c.mean_d2s, c.n_d2s, c.mean_s2d, c.n_s2d, c.overall,
                                                                                                        f.precision, f.recall, f.fscore))
    h = r.get("host")
    if h:
        print("  host, sklearn kd_tree with n_jobs = 16 on %d of the sampled points: radius lists %.2f s + the thinning loop %.2f s (%d kept; %d entries differ from the"
              " device's mask, which decides in f32), kneighbors of the kept against %d gt points %.2f s; the device on the same inputs: downsample %.3f ms, nearest %.3f ms"
              % (h["n"], h["radius_lists_s"], h["loop_s"], h["kept"], h["mask_diff"], h["n"], h["kneighbors_s"], h["dev_thin_ms"], h["dev_nearest_ms"]))


def bench_tnt(raw, post, voxel, host_points):
    """Stage times of ibgs_amd/registration.py (hipEvents around the Python calls, median of 3 after a warm-up, read-backs included)."""
    from tests import registration_ref as ref
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, reps=3):
        out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = ev(), ev()
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), out

    density = voxel / 3
    tau = 2 * density
    gt_cloud = mesh_eval.sample_surface(raw, 1.5 * density)
    gt = gt_cloud[mesh_eval.downsample(gt_cloud, 1.5 * density)]
    del gt_cloud
    planted = ref.similarity(1.01, 1.0, (0.3, -0.5, 0.8), (3 * tau, -2 * tau, 2.5 * tau))
    pred = registration.transform(post.vertices, np.linalg.inv(planted))          # evaluate_tnt has to find `planted`
    lo, hi = gt.amin(0).cpu().numpy().astype(np.float64), gt.amax(0).cpu().numpy().astype(np.float64)
    ext = hi - lo
    x0, y0, x1, y1 = lo[0] - 0.01 * ext[0], lo[1] - 0.01 * ext[1], hi[0] + 0.01 * ext[0], hi[1] + 0.01 * ext[1]
    poly = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y0 + 0.7 * (y1 - y0), 0], [x0 + 0.7 * (x1 - x0), y1, 0], [x0, y1, 0]])
    vol = registration.CropVolume("Z", lo[2] - 0.01 * ext[2], hi[2] + 0.01 * ext[2], poly)
    r = {"tau": tau, "pred": int(pred.shape[0]), "gt": int(gt.shape[0])}
    r["transform_ms"], moved = timed(lambda: registration.transform(pred, planted))
    r["crop_ms"], m_gt = timed(lambda: registration.crop(gt, vol))
    r["crop_T_ms"], m_pred = timed(lambda: registration.crop(pred, vol, planted))
    gt_c, pred_c = gt[m_gt], moved[m_pred]
    r["gt_cropped"], r["pred_cropped"] = int(gt_c.shape[0]), int(pred_c.shape[0])
    r["voxel_tau_ms"], t1 = timed(lambda: registration.voxel_down_sample(gt_c, tau))
    r["voxel_half_ms"], t2 = timed(lambda: registration.voxel_down_sample(gt_c, tau / 2))
    r["gt_at_tau"], r["gt_at_half"] = int(t1.shape[0]), int(t2.shape[0])
    s1 = registration.voxel_down_sample(pred_c, tau)
    r["moments_ms"], _ = timed(lambda: registration.moments(s1, t1, 20 * tau))
    icp1, _ = timed(lambda: registration.icp(s1, t1, 20 * tau, max_iter=1))
    icp5, r5 = timed(lambda: registration.icp(s1, t1, 20 * tau, max_iter=5, rel_fitness=0.0, rel_rmse=0.0))
    r["icp_iteration_ms"], r["icp_setup_ms"], r["icp_points"] = (icp5 - icp1) / 4, icp1 - (icp5 - icp1) / 4 * 2, (int(s1.shape[0]), int(t1.shape[0]))
    r["evaluate_ms"], e = timed(lambda: registration.evaluate_tnt(pred, gt, np.identity(4), vol, tau))
    r["evaluate"] = e
    r["planted_err"] = float(np.abs(e["transformation"] - planted).max())
    if host_points:
        from tests import mesh_eval_ref
        n = min(host_points, pred.shape[0], gt.shape[0])
        g = torch.Generator(device="cpu")
        g.manual_seed(0)
        hp = pred[torch.randperm(pred.shape[0], generator=g)[:n].to(pred.device)].cpu().numpy()
        hg = gt[torch.randperm(gt.shape[0], generator=g)[:n].to(gt.device)].cpu().numpy()
        volume = (vol.axis, vol.axis_min, vol.axis_max, vol.polygon)
        t0 = time.perf_counter()
        q = ref.transform(hp, planted)
        t1_ = time.perf_counter()
        mask = ref.crop(hg, *volume)
        t2_ = time.perf_counter()
        thin = ref.voxel_down_sample(hg[mask], tau)[0].astype(np.float32)
        t3_ = time.perf_counter()
        _, idx = mesh_eval_ref.nearest(q, thin, 20 * tau)
        t4_ = time.perf_counter()
        ref.moments(q, thin, idx, ref.pivot_of(thin))
        t5_ = time.perf_counter()
        dq, dg = torch.as_tensor(hp, device=pred.device), torch.as_tensor(hg, device=pred.device)
        dthin = registration.voxel_down_sample(dg[registration.crop(dg, vol)], tau)
        dev_vox, _ = timed(lambda: registration.voxel_down_sample(dg, tau))
        dev_mom, _ = timed(lambda: registration.moments(dq, dthin, 20 * tau, planted))
        r["host"] = {"n": n, "transform_s": t1_ - t0, "crop_s": t2_ - t1_, "voxel_s": t3_ - t2_, "nearest_s": t4_ - t3_, "moments_s": t5_ - t4_,
                     "dev_voxel_ms": dev_vox, "dev_moments_ms": dev_mom}
    return r


def print_tnt(r):
    e = r["evaluate"]
    print("registration on the post-processed mesh's %d vertices against %d gt points, tau %.6f (two thirds of the voxel), a 5-vertex volume:" % (r["pred"], r["gt"], r["tau"]))
    print("  transform: %.3f ms; crop of gt: %.3f ms -> %d; crop of pred through the fused T: %.3f ms -> %d" % (r["transform_ms"], r["crop_ms"], r["gt_cropped"],
                                                                                                      r["crop_T_ms"], r["pred_cropped"]))
    print("  voxel_down_sample of the cropped gt (bounds + keys + torch.sort + heads + scan + read-back + means): at tau %.3f ms -> %d, at tau / 2 %.3f ms -> %d"
          % (r["voxel_tau_ms"], r["gt_at_tau"], r["voxel_half_ms"], r["gt_at_half"]))
    print("  one ICP evaluation from scratch (hierarchy + bounds read-back + transform + nearest + moments + read-back), %d -> %d points: %.3f ms" % (r["icp_points"] + (r["moments_ms"],)))
    print("  one ICP iteration (transform + nearest + moments + read-back + 3 x 3 SVD on the host; from icp at 5 and at 1 updates): %.3f ms; the rest of an icp call: %.3f ms"
          % (r["icp_iteration_ms"], r["icp_setup_ms"]))
    print("  evaluate_tnt (three rounds + the final thinning + fscore): %.3f ms; iterations %s; precision %.4f recall %.4f F %.4f on %d / %d points; |T - planted| %.3g"
          % (r["evaluate_ms"], [x.iterations for x in e["rounds"]], e["precision"], e["recall"], e["fscore"], e["n_pred"], e["n_gt"], r["planted_err"]))
    h = r.get("host")
    if h:
        print("  numpy restatement (host) on %d points of each cloud: transform %.3f s, crop %.3f s, voxel_down_sample %.3f s, nearest (scipy kd-tree) %.3f s, moments %.3f s; "
              "the device on the same inputs: voxel_down_sample %.3f ms, one ICP evaluation %.3f ms"
              % (h["n"], h["transform_s"], h["crop_s"], h["voxel_s"], h["nearest_s"], h["moments_s"], h["dev_voxel_ms"], h["dev_moments_ms"]))


DTU_VIEWS, DTU_W, DTU_H, DTU_RADIUS = 49, 1600, 1200, 24


def bench_dtu(raw, post, voxel, host_vertices):
    """Stage times of ibgs_amd/dtu.py (hipEvents around the Python calls, median of 3 after a warm-up, read-backs included)."""
    from tests import dtu_ref as ref
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, reps=3):
        out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = ev(), ev()
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), out

    dev = raw.vertices.device
    n, W, H = DTU_VIEWS, DTU_W, DTU_H
    # the post-processed mesh (the largest cluster) frames the scene: the raw mesh's bounds are those of its farthest floater
    lo, hi = post.vertices.amin(0).cpu().numpy().astype(np.float64), post.vertices.amax(0).cpu().numpy().astype(np.float64)
    centre, ext = (lo + hi) / 2, hi - lo
    up_axis = int(np.argmin(ext))
    up = np.zeros(3)
    up[up_axis] = 1.0
    a1, a2 = [k for k in range(3) if k != up_axis]
    dist = 1.2 * float(ext.max())
    P = []
    for i in range(n):
        az, el = 2 * np.pi * i / n, np.deg2rad(30.0 if i % 2 == 0 else 55.0)
        eye = centre.copy()
        eye[a1] += dist * np.cos(el) * np.cos(az)
        eye[a2] += dist * np.cos(el) * np.sin(az)
        eye[up_axis] += dist * np.sin(el)
        P.append(ref.look_at(eye, centre, -up, 1.1 * W, W, H))
    P = torch.as_tensor(np.stack(P), device=dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    masks = torch.stack([(((xx - W / 2 - 40 * np.cos(i)) / (0.45 * W)) ** 2 + ((yy - H / 2 - 30 * np.sin(i)) / (0.45 * H)) ** 2 <= 1.0) for i in range(n)]).to(torch.uint8)
    density = voxel / 3
    r = {"V": int(raw.vertices.shape[0]), "F": int(raw.faces.shape[0]), "density": density, "F_post": int(post.faces.shape[0])}
    r["dilate_ms"], bits = timed(lambda: dtu.dilate_masks(masks, DTU_RADIUS))
    r["mask_set"] = float(masks.float().mean())
    r["cull_vertices_ms"], keep = timed(lambda: dtu.cull_vertices(raw.vertices, P, bits))
    r["kept"] = int(keep.sum())
    r["cull_mesh_ms"], culled = timed(lambda: dtu.cull_mesh(raw, P, bits, scale=1.0, offset=(0.0, 0.0, 0.0)))
    r["cull_mesh_raw_ms"], _ = timed(lambda: dtu.cull_mesh(raw, P, masks, radius=DTU_RADIUS))
    r["V2"], r["F2"] = int(culled.vertices.shape[0]), int(culled.faces.shape[0])
    gt_cloud = mesh_eval.sample_surface(raw, 1.5 * density)
    gt = gt_cloud[mesh_eval.downsample(gt_cloud, 1.5 * density)]
    del gt_cloud
    res = float(ext.max()) / 200
    inner = np.where(np.arange(3) == up_axis, 1.0, 0.7)          # the box: 70 % of the mesh's extent across, all of it along the up axis
    b0 = centre - inner * ext / 2
    cells = np.ceil(inner * ext / res)
    bb = np.stack([b0, b0 + res * cells]).astype(np.float32)
    shape = tuple(int(x) + 1 for x in cells)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    obs = (torch.rand(shape, generator=g, device=dev) < 0.7).to(torch.uint8)
    plane = np.zeros(4)
    plane[up_axis], plane[3] = 1.0, -(lo[up_axis] + 0.2 * ext[up_axis])
    patch = 5 * res
    cloud = mesh_eval.sample_surface(post, density)
    r["cloud"], r["gt"], r["obs_shape"] = int(cloud.shape[0]), int(gt.shape[0]), shape
    r["obs_filter_ms"], filt = timed(lambda: dtu.obs_mask_filter(cloud, obs, bb, res, patch))
    r["above_plane_ms"], above = timed(lambda: dtu.above_plane(gt, plane))
    r["inbound"], r["in_obs"], r["above"] = int(filt.inbound.sum()), int(filt.in_obs.sum()), int(above.sum())
    del cloud, filt
    r["evaluate_ms"], e = timed(lambda: dtu.evaluate_dtu(post, gt, obs, bb, res, plane, density=density, max_dist=100 * density, patch=patch))
    r["evaluate_cull_ms"], ec = timed(lambda: dtu.evaluate_dtu(post, gt, obs, bb, res, plane, density=density, max_dist=100 * density, patch=patch,
                                                                cull=dtu.Cull(P, bits)))
    r["evaluate"], r["evaluate_cull"] = e, ec
    if host_vertices:
        one = masks[0].cpu().numpy()
        t0 = time.perf_counter()
        want = ref.dilate(one, DTU_RADIUS)
        t1 = time.perf_counter()
        same_d = bool(np.array_equal(ref.pack_bits(want[None])[0], bits.words[0].cpu().numpy()))
        m = min(host_vertices, r["V"])
        sub = raw.vertices[torch.randperm(r["V"], device=dev)[:m]].contiguous()
        dil = ref.unpack_bits(bits.words.cpu().numpy(), W)[0]
        hv, hP = sub.cpu().numpy(), P.cpu().numpy()
        t2 = time.perf_counter()
        hk = ref.cull_vertices(hv, hP, dil)
        t3 = time.perf_counter()
        dev_ms, dk = timed(lambda: dtu.cull_vertices(sub, P, bits))
        r["host"] = {"dilate_one_s": t1 - t0, "dilate_equal": same_d, "n": m, "cull_s": t3 - t2, "cull_equal": bool(np.array_equal(hk, dk.cpu().numpy())),
                     "dev_cull_ms": dev_ms}
    return r


def print_dtu(r):
    print("DTU front end on the raw mesh (V %d, F %d), %d masks of %d x %d (%.0f %% set), radius %d:" % (r["V"], r["F"], DTU_VIEWS, DTU_W, DTU_H, 100 * r["mask_set"], DTU_RADIUS))
    print("  dilate_masks (pack + dilate): %.3f ms = %.1f G pixels/s" % (r["dilate_ms"], DTU_VIEWS * DTU_W * DTU_H / r["dilate_ms"] / 1e6))
    print("  cull_vertices (kernel + read-back): %.3f ms -> %d kept; %.1f G vertex-views/s if no thread stopped early" % (r["cull_vertices_ms"], r["kept"], r["V"] * DTU_VIEWS / r["cull_vertices_ms"] / 1e6))
    print("  cull_mesh from dilated bits (cull + mark + 2 scans + read-back + emit + read-back): %.3f ms -> V' %d, F' %d; from raw masks (dilation included): %.3f ms"
          % (r["cull_mesh_ms"], r["V2"], r["F2"], r["cull_mesh_raw_ms"]))
    print("  obs_mask_filter on the %d sampled points of the post-processed mesh (F %d), ObsMask %s: %.3f ms -> %d in bounds, %d observed; above_plane on %d gt points: %.3f ms -> %d"
          % (r["cloud"], r["F_post"], "x".join(str(x) for x in r["obs_shape"]), r["obs_filter_ms"], r["inbound"], r["in_obs"], r["gt"], r["above_plane_ms"], r["above"]))
    print("  evaluate_dtu (sample + thin + filters + chamfer): %.3f ms; with the cull in front: %.3f ms" % (r["evaluate_ms"], r["evaluate_cull_ms"]))
    print("    %s" % r["evaluate"])
    print("    %s" % r["evaluate_cull"])
    h = r.get("host")
    if h:
        print("  numpy restatement (host, for information): dilation of ONE mask %.2f s (x %d masks = %.0f s), equal to the device's: %s; the vertex rule on %d vertices x %d views %.2f s, "
              "equal: %s; the device on the same vertices: %.3f ms" % (h["dilate_one_s"], DTU_VIEWS, DTU_VIEWS * h["dilate_one_s"], h["dilate_equal"], h["n"], DTU_VIEWS, h["cull_s"],
                                                                      h["cull_equal"], h["dev_cull_ms"]))


def bench_voxel(views, span, dedup_ab=True, keep_mesh=None, mesh_eval_host=None, tnt_host=None, dtu_host=None):
    voxel = 2 * scenes.GROUND_HALF / span
    vol = tsdf.TSDFVolume(voxel, 4 * voxel, block_capacity=1 << 21)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def run(dedup):
        vol.reset()
        ms, active = [], []
        for c, d, col in views:
            a, b = ev(), ev()
            a.record()
            vol.integrate_view(c, d, color=col) if dedup else vol.integrate(d, c.Fx, c.Fy, c.Cx, c.Cy, _pose(c), color=col, dedup=False)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
            active.append(int(vol._state[_lib.TSDF_ACTIVE].item()))
        return ms, active

    run(True)          # warm-up: code objects, allocator
    ms, active = run(True)
    ms_nd, _ = run(False) if dedup_ab else (None, None)
    ms2, _ = run(True)          # the dedup run again after the A/B one: the spread of the same measurement
    vol.check()
    blocks = vol.num_blocks()
    a, b = ev(), ev()
    vol.extract_mesh()          # warm-up
    torch.cuda.synchronize()
    a.record()
    mesh = vol.extract_mesh()
    b.record()
    b.synchronize()
    ext = a.elapsed_time(b)
    assert vol.mesh_overruns() == 0

    def timed(fn, reps=3):
        out = fn()          # warm-up: code objects, allocator
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = ev(), ev()
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), out

    cl_ms, cl = timed(lambda: meshpp.cluster_connected_triangles(mesh))
    pp_ms, post = timed(lambda: meshpp.post_process_mesh(mesh, 1))
    pp = {"cluster_ms": cl_ms, "post_ms": pp_ms, "C": int(cl.cluster_n_triangles.shape[0]), "largest": int(cl.cluster_n_triangles.max()),
          "V2": int(post.vertices.shape[0]), "F2": int(post.faces.shape[0]), "scratch": _lib.load().ibgs_mesh_required_scratch(mesh.vertices.shape[0], mesh.faces.shape[0])}
    if keep_mesh is not None:
        keep_mesh.append((mesh, cl, post))
    me = bench_mesh_eval(mesh, post, voxel, mesh_eval_host) if mesh_eval_host is not None else None
    tnt = bench_tnt(mesh, post, voxel, tnt_host) if tnt_host is not None else None
    du = bench_dtu(mesh, post, voxel, dtu_host) if dtu_host is not None else None
    return {"pp": pp, "mesh_eval": me, "tnt": tnt, "dtu": du, "span": span, "voxel": voxel, "ms": ms, "ms_again": ms2, "ms_nodedup": ms_nd, "active": active, "blocks": blocks, "extract_ms": ext,
            "V": int(mesh.vertices.shape[0]), "F": int(mesh.faces.shape[0])}


def _pose(c):
    pose = np.identity(4)
    pose[:3, :3] = np.asarray(c.R, np.float64).T
    pose[:3, 3] = np.asarray(c.T, np.float64)
    return pose


def restatement_time():
    from tests import tsdf_ref as ref
    W, H, F = 160, 120, 140.0
    vol = ref.RefVolume(0.02, 0.08)
    t0 = time.perf_counter()
    for d in ref.fibonacci_directions(24):
        M = ref.look_at(2.0 * d)
        dep, col = ref.sphere_view(M, W, H, F, F, 80.0, 60.0, 0.5)
        vol.integrate(dep, F, F, 80.0, 60.0, M, color=col)
    t1 = time.perf_counter()
    import ctypes
    tab = (ctypes.c_int32 * 4096)()
    _lib.load().ibgs_tsdf_mc_table(tab)
    v, f, _, _ = ref.marching_cubes(vol.blocks(), 0.02, np.array(tab))
    t2 = time.perf_counter()
    return len(vol.coords), (t1 - t0) * 1e3 / 24, (t2 - t1) * 1e3, len(v), len(f)


def mesh_restatement_time(mesh, cl, post):
    """The host restatement of the post-processing (numpy + scipy, not Open3D) on a device mesh; its results must be the kernels'."""
    from tests import mesh_ref
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    t0 = time.perf_counter()
    lab, counts, _ = mesh_ref.cluster(v, f)
    t1 = time.perf_counter()
    rows, fo = mesh_ref.post_process(f, len(v), lab, counts, 1)
    t2 = time.perf_counter()
    same = bool(np.array_equal(lab, cl.triangle_clusters.cpu().numpy()) and np.array_equal(fo, post.faces.cpu().numpy())
                and v[rows].tobytes() == post.vertices.cpu().numpy().tobytes())
    return t1 - t0, t2 - t1, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--gaussians", type=int, default=400000)
    ap.add_argument("--spans", default="1024,2048")
    ap.add_argument("--kstats", default=None)
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--no-ab", action="store_true", help="skip the run without the LDS dedup (under the profiler: one allocation variant per kernel line)")
    ap.add_argument("--kstats-only", action="store_true", help="print the kernel split of --kstats DIR and exit (no GPU needed)")
    ap.add_argument("--active", type=int, default=None, help="with --kstats-only: active blocks per view, for the update's bytes per second")
    ap.add_argument("--faces", type=int, default=None, help="with --kstats-only: faces of the mesh, for the edge kernel's edges per second")
    ap.add_argument("--mesh-restatement", action="store_true", help="time tests/mesh_ref.py (numpy + scipy, host) on the first span's mesh and compare the results")
    ap.add_argument("--mesh-eval", action="store_true", help="time every stage of ibgs_amd/mesh_eval.py on each span's post-processed mesh")
    ap.add_argument("--mesh-eval-host", type=int, default=300000, help="with --mesh-eval / --tnt: points handed to the host engine (sklearn's kd-tree / the numpy restatement; 0: skip)")
    ap.add_argument("--tnt", action="store_true", help="time every stage of ibgs_amd/registration.py (evaluate_tnt) on each span's post-processed mesh")
    ap.add_argument("--dtu", action="store_true", help="time every stage of ibgs_amd/dtu.py (dilate_masks, cull_vertices, cull_mesh, the filters, evaluate_dtu) on each span's meshes")
    a = ap.parse_args()
    if a.kstats_only:
        print_split(a.kstats, a.active, a.faces)
        return
    assert torch.cuda.is_available(), "bench_tsdf.py measures on the GPU"
    dev = torch.device("cuda")
    W, H = 1920, 1080
    t0 = time.perf_counter()
    views = render_views(a.views, W, H, a.gaussians, dev)
    print("surface scene: %d Gaussians, %d views at %dx%d (two elevations), rendered in %.1f s; valid pixels per view %.0f"
          % (a.gaussians, a.views, W, H, time.perf_counter() - t0, np.mean([float((d > 0).sum()) for _, d, _ in views])))
    ks = bool(a.kstats)
    first_mesh = []
    for span in [int(s) for s in a.spans.split(",")]:
        r = bench_voxel(views, span, dedup_ab=not a.no_ab, keep_mesh=first_mesh if a.mesh_restatement and not first_mesh else None,
                        mesh_eval_host=a.mesh_eval_host if a.mesh_eval else None, tnt_host=a.mesh_eval_host if a.tnt else None,
                        dtu_host=a.mesh_eval_host if a.dtu else None)
        act = np.array(r["active"], np.float64)
        med = lambda x: float(np.median(x))
        print("\n== ground square spans %d voxels: voxel %.6f, sdf_trunc %.6f" % (span, r["voxel"], 4 * r["voxel"]))
        print("integrate per view (alloc + update, events): median %.3f ms (repeat %.3f ms), min %.3f, max %.3f"
              % (med(r["ms"]), med(r["ms_again"]), min(r["ms"]), max(r["ms"])))
        if r["ms_nodedup"]:
            print("  without the LDS dedup (every pixel's blocks to the global hash): median %.3f ms" % med(r["ms_nodedup"]))
        print("active blocks per view: median %.0f, min %.0f, max %.0f; allocated after %d views: %d" % (med(act), act.min(), act.max(), len(act), r["blocks"]))
        upd_bytes = med(act) * 512 * 40
        print("update traffic per view at the median: %.1f MB (40 B per voxel of an active block)" % (upd_bytes / 1e6))
        print("  over the whole call's median time: %.2f TB/s = %.0f %% of 8 TB/s (a lower bound for the update kernel alone)"
              % (upd_bytes / (med(r["ms"]) * 1e-3) / 1e12, 100 * upd_bytes / (med(r["ms"]) * 1e-3) / HBM_BYTES_PER_S))
        print("extract_mesh (sort + count + scan + read-back + emit): %.3f ms, V %d, F %d" % (r["extract_ms"], r["V"], r["F"]))
        p = r["pp"]
        print("cluster_connected_triangles (memsets + 4 kernels + scan + read-back): %.3f ms = %.2f x extract_mesh; C %d, largest cluster %d faces; scratch %.0f MB"
              % (p["cluster_ms"], p["cluster_ms"] / r["extract_ms"], p["C"], p["largest"], p["scratch"] / 1e6))
        print("post_process_mesh(mesh, 1) (clustering + top-k + mark + 2 scans + read-back + emit + read-back): %.3f ms = %.2f x extract_mesh; V' %d, F' %d"
              % (p["post_ms"], p["post_ms"] / r["extract_ms"], p["V2"], p["F2"]))
        if r["mesh_eval"]:
            print_mesh_eval(r["mesh_eval"])
        if r["tnt"]:
            print_tnt(r["tnt"])
        if r["dtu"]:
            print_dtu(r["dtu"])
    if ks:
        print_split(a.kstats)
    if first_mesh:
        t_cl, t_pp, same = mesh_restatement_time(*first_mesh[0])
        print("\nnumpy + scipy restatement of the post-processing (host; not Open3D) on the %d-face mesh: clustering %.2f s, filter %.2f s; results equal to the kernels': %s"
              % (first_mesh[0][0].faces.shape[0], t_cl, t_pp, same))
    if not a.no_restatement:
        nb, ms_view, ms_mc, V, F = restatement_time()
        print("\nnumpy restatement (host), sphere 160x120, 24 views, voxel 0.02: %d blocks, %.1f ms per view, marching cubes %.1f ms (V %d, F %d)"
              % (nb, ms_view, ms_mc, V, F))


if __name__ == "__main__":
    main()
