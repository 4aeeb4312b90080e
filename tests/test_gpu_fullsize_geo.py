"""The two geo workloads of bench.py's `--full` line at FULL size against the oracle, in the suite the driver runs (round 5; until round 4 these
tables were `tools/parity_c3.py geo ...` text files under profiles/):

  `geo`          C3 (1 M random-init Gaussians, 1920 x 1080, SH 3) + render_geo, 4 sources, L = 4          (SURVEY.md 8(d) "second line")
  `trained_geo`  the same on the trainer-like scene (plane-like, log-normal sizes, 30 % in one blob, trained opacities; ref train.py:287-292)

The inputs ARE the bench's: `bench.Workload(...)` builds them (source images / depth maps included) and the numpy copies go to the oracle.
Checked: R, the sorted lists and tile ranges (exact), the colour image, n_contrib, the median-buffer window caches and valid-source sets, the
seven geo planes, and ALL gradients incl. dL/dall_map.  Gradient bar: relative L2 <= 1e-3 against the fp32 oracle, or -- where the fp32 oracle
itself is further than that from the float64 build of the same C source -- |HIP - f64| <= 2 x |oracle fp32 - f64| (the arbiter of
tests/test_gpu_anisotropic.py).  A table of every number is printed and, when gpurun_out/ exists, written to gpurun_out/parity_fullsize_<name>.txt."""
import os
import time

import numpy as np
import pytest
import torch

import oracle
from ibgs_amd import rasterizer
from tests import hipref
from tests.metrics import l1, psnr, rel_l2
from tests.scenes import valid_source_histogram
from tests.test_gpu_anisotropic import F64_K
from tests.test_gpu_parity import GRAD_PAIRS, canon_valid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_geo_inputs(opacity, **shape):
    """bench.py's geo Workload (view 0) as an oracle-style input dict: same Gaussians, same camera, the same four source views with the
    images / depth maps bench.py renders for them."""
    import bench
    wl = bench.Workload("C3", 0, torch.device("cuda", 0), opacity, True, False, 1234, **shape)
    st = wl.st
    inp = dict(wl.inp)
    inp.update(all_map=wl.leaves["all_map"].detach().cpu().numpy(), render_geo=True, n_src=int(st.nb_src_images), buffer_length=int(st.buffer_length),
               depth_thr=float(st.depth_error_threshold), ref_to_src=st.ref_to_src_list.cpu().numpy(), src_cam_pos=st.src_cam_pos.cpu().numpy(),
               src_images=st.src_images.cpu().numpy(), src_depths=st.src_rendered_depths.cpu().numpy())
    assert inp["n_src"] == 4 and inp["buffer_length"] == 4 and inp["W"] == 1920 and inp["H"] == 1080 and inp["means3D"].shape[0] == 10 ** 6
    del wl
    torch.cuda.empty_cache()
    return inp


def full_size_geo_parity(name, inp, min_mean_valid=None, min_all_valid=None, extra_checks=None):
    """min_mean_valid / min_all_valid: bars on the oracle's valid-source histogram (mean count per covered pixel / share of covered pixels with all n_src
    valid) -- a scene that is to exercise the warp path says how much of it; extra_checks(o, ist, say) -> list of failures: more checks on the HIP outputs."""
    H, W = int(inp["H"]), int(inp["W"])
    lines = []

    def say(s):
        print(s); lines.append(s)

    r_ = np.random.default_rng(9)
    g = {"color": np.random.default_rng(1).standard_normal((3, H, W)).astype(np.float32), "normal_map": r_.standard_normal((3, H, W)).astype(np.float32),
         "median_depth": r_.standard_normal((1, H, W)).astype(np.float32), "warped_image": r_.standard_normal((15, H, W)).astype(np.float32)}
    t0 = time.time()
    ref = oracle.forward(inp, tex_quant=rasterizer.TEX_QUANT, cull=True)
    rb = oracle.backward(inp, ref, g["color"], g["normal_map"], g["median_depth"], g["warped_image"], tex_quant=rasterizer.TEX_QUANT)
    t1 = time.time()
    outs, lv, _ = hipref.run_forward(inp)
    ist = hipref.internal_state(outs, inp)
    o = hipref.to_np(outs)
    loss = 0
    for k, v in g.items():
        loss = loss + (outs[k] * torch.as_tensor(v, device="cuda")).sum()
    loss.backward()
    torch.cuda.synchronize()
    hip = {lk: lv[lk].grad.cpu().numpy() for lk, _ in GRAD_PAIRS if lv.get(lk) is not None and lv[lk].grad is not None}
    del outs, lv, loss
    torch.cuda.empty_cache()

    say("# %s at full size: %d Gaussians, %d x %d, n_src %d, L %d, depth_thr %g; oracle fp32 fwd+bwd %.1f s" % (name, inp["means3D"].shape[0], W, H, inp["n_src"], inp["buffer_length"],
                                                                                                          inp["depth_thr"], t1 - t0))
    # ---- integer stages: exact
    same_lists = ist["R"] == ref["num_rendered"] and np.array_equal(ist["point_list"], ref["point_list"]) and np.array_equal(ist["ranges"], ref["ranges"])
    say("R %d == %d, lists and tile ranges equal: %s, radii equal: %s" % (ist["R"], ref["num_rendered"], same_lists, np.array_equal(o["radii"], ref["radii"])))
    assert same_lists and np.array_equal(o["radii"], ref["radii"])
    # ---- the colour image and the per-pixel counters
    tgt = np.random.default_rng(2).random(ref["color"].shape).astype(np.float32)
    d_img = l1(o["color"], ref["color"]); same_n = (ist["n_contrib"] == ref["n_contrib"]).mean()
    say("image: mean L1 %.3e max %.3e, PSNR vs a common target HIP %.4f dB oracle %.4f dB, n_contrib equal on %.6f of the pixels"
        % (d_img, np.abs(o["color"] - ref["color"]).max(), psnr(o["color"], tgt)[0], psnr(ref["color"], tgt)[0], same_n))
    assert d_img < 1e-6 and same_n > 0.9999 and abs(psnr(o["color"], tgt)[0] - psnr(ref["color"], tgt)[0]) < 1e-3
    assert l1(ist["final_T"], ref["final_T"]) < 1e-6
    # ---- median buffer: window caches, valid-source sets
    win = ((ist["low_high"][:, 0] == ref["cache_low"]) & (ist["low_high"][:, 1] == ref["cache_high"])).mean()
    same = np.all(canon_valid(ist["valid_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    first = (ref["valid_src_idx"][0] >= 0).mean()
    say("median-buffer windows equal on %.6f of the pixels; valid-source sets equal on all but %d pixels; a first source is valid on %.3f, sum_w mean |d| %.2e"
        % (win, int((~same).sum()), first, np.abs(ist["sum_w"] - ref["cache_sum_w"]).mean()))
    # (both are DECISIONS on rounded floats -- `T > 0.5` picks the window, `err < depth_thr` the valid sources -- so a handful of the 2 M pixels flips
    # between any two fp32 evaluations; the oracle's own fma-contracted build beside it says how many the reference's arithmetic leaves open)
    with oracle.variant("fma"):
        tw = oracle.forward(inp, tex_quant=rasterizer.TEX_QUANT, cull=True)
    tw_win = ((tw["cache_low"] == ref["cache_low"]) & (tw["cache_high"] == ref["cache_high"])).mean()
    tw_same = np.all(canon_valid(tw["valid_src_idx"]) == canon_valid(ref["valid_src_idx"]), axis=0)
    say("    (the oracle against its own fma-contracted build: windows equal on %.6f, valid-source sets differ on %d pixels, n_contrib equal on %.6f)"
        % (tw_win, int((~tw_same).sum()), (tw["n_contrib"] == ref["n_contrib"]).mean()))
    assert first > 0.05, "the scene does not exercise the warp path"
    # ---- how many sources the warp finds valid per covered pixel: HIP and oracle, and the regime the caller asks for
    n_src = int(inp["n_src"])
    h_ref, m_ref = valid_source_histogram(ref["valid_src_idx"], ref["final_T"], n_src)
    h_hip, m_hip = valid_source_histogram(ist["valid_idx"], ist["final_T"], n_src)
    say("valid sources per covered pixel: oracle mean %.3f [%s], HIP mean %.3f [%s]" % (m_ref, " ".join("%.4f" % x for x in h_ref), m_hip,
                                                                                   " ".join("%.4f" % x for x in h_hip)))
    # (the two histograms can differ only by the pixels whose valid-source sets differ: asserted below)
    if min_mean_valid is not None:
        assert m_ref >= min_mean_valid, "the scene has drifted out of the multi-view-consistent regime"
    if min_all_valid is not None:
        assert h_ref[n_src] >= min_all_valid, "too few pixels with every source valid"
    assert win > 0.9999 and (~same).mean() <= 1e-4, "median-buffer windows / valid-source sets differ on more pixels than rounding explains"
    assert (1 - win) <= max(1e-5, 3 * (1 - tw_win)) and (~same).sum() <= max(20, 3 * int((~tw_same).sum())), "more decision flips than the reference's own arithmetic leaves open"
    ok = same.reshape(H, W)
    mask_same = (o["use_first_src_frame_mask"] == ref["use_first_src_frame_mask"])[:, ok].mean()
    say("use_first_src_frame_mask equal on %.6f of those pixels" % mask_same)
    assert mask_same == 1.0
    # ---- the seven planes (on the pixels whose valid-source sets agree: a slot shifted by one source is a different quantity)
    for k, tol in (("normal_map", 1e-5), ("median_depth", 1e-5), ("warped_image", 1e-5), ("cam_feat", 1e-5), ("camera_ray", 1e-5), ("min_depth_diff", 1e-4)):
        dd = np.abs(o[k] - ref[k])[:, ok]
        rel = dd.mean() / (np.abs(ref[k][:, ok]).mean() + 1e-12)
        say("    %-14s mean |d| %.2e (rel %.2e) max %.2e" % (k, dd.mean(), rel, dd.max()))
        assert rel < tol, k
    # ---- all gradients; float64 arbiter where the plain bar is exceeded
    t2 = time.time()
    with oracle.variant("f64"):
        r64 = oracle.forward(inp, tex_quant=rasterizer.TEX_QUANT, cull=True)
        b64 = oracle.backward(inp, r64, g["color"], g["normal_map"], g["median_depth"], g["warped_image"], tex_quant=rasterizer.TEX_QUANT)
    say("gradients, relative L2 (float64 build of the oracle: %.1f s): HIP vs oracle fp32 | HIP vs f64 | oracle fp32 vs f64" % (time.time() - t2))
    failed = []
    for lk, rk in GRAD_PAIRS:
        if lk not in hip:
            continue
        a = hip[lk]; b = np.asarray(rb[rk]).reshape(a.shape); t = np.asarray(b64[rk]).reshape(a.shape)
        if np.abs(b).max() == 0:
            assert np.abs(a).max() == 0, lk
            continue
        e32, e64, floor = rel_l2(a, b), rel_l2(a, t), rel_l2(b, t)
        verdict = "ok" if e32 <= 1e-3 else ("ok by the arbiter" if e64 <= F64_K * floor else "FAIL")
        say("    %-12s %.2e | %.2e | %.2e   %s" % (lk, e32, e64, floor, verdict))
        if verdict == "FAIL":
            failed.append(lk)
    if extra_checks is not None:
        failed += extra_checks(o, ist, say)
    out_dir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "parity_fullsize_%s.txt" % name), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not failed, failed


def test_c3_geo_full_size_against_the_oracle():
    """bench.py's `geo` object: C3 init opacities, render_geo, 4 sources (the neighbouring orbit views, images and depth maps rendered by the op), L 4."""
    full_size_geo_parity("geo", bench_geo_inputs("init"))


def test_trained_geo_full_size_against_the_oracle():
    """bench.py's `trained_geo` object: what train.py:289-292 runs in steady state (plane-like, heavy-tailed, clustered, trained opacities)."""
    full_size_geo_parity("trained_geo", bench_geo_inputs("trained", cluster=0.3, anisotropy="plane", scale_sigma=1.0))
