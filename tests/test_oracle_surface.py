"""The geo path on a MULTI-VIEW-CONSISTENT scene (tests/scenes.surface_scene: opaque discs on a sphere and a ground square, source depths = depth renders of
the same discs, depth_thr 0.01): the regime the trainer runs in, where most covered pixels see 3-5 valid sources -- slots 1-4 of every per-source plane,
the five-valid case without a -1 terminator, min_depth_diff far below its start value.  The random clouds of the other geo scenes validate a source on
a few per cent of their pixels.

Here (no GPU) the oracle is checked against CLOSED FORMS that do not come from any restatement of the reference: on the pixels whose ray hits the ground
square clear of the sphere, every buffered contributor is a ground disc lying exactly in the plane z = GROUND_Z, so the median depth is the ray/plane
depth, the normal is the ground's, the warped colour of a LINEAR source image is that function at the source projection of the ground point, and a
source is valid iff that point is in its frame and not hidden by the sphere.  tests/test_gpu_surface_geo.py applies the same checks to the HIP outputs."""
import time

import numpy as np
import pytest

import oracle
from tests.scenes import GROUND_HALF, GROUND_Z, SPHERE_R, SRC_AZIMUTHS, surface_scene, valid_source_histogram
from ibgs_amd import synthetic as syn

MIN_MEAN_VALID = 2.5          # mean valid sources per covered pixel the scene must keep ...
MIN_ALL_VALID_5 = 0.40        # ... and the share of covered pixels with all 5 valid (n_src 5)


def _seg_dist(a, b):
    """distance from the origin (the sphere's centre) to the segments a -> b (rows, float64)"""
    d = b - a
    t = np.clip(-(a * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0)
    return np.linalg.norm(a + t[:, None] * d, axis=-1)


def surface_truth(inp, margin_px=3.0):
    """Float64 closed forms on the surface scene for every pixel whose ray hits the ground square with a margin (4 ground-disc radii) and passes the
    sphere by more than 4 sphere-disc radii + `margin_px` pixels (every blended contributor there is a ground disc).  Pixel (px, py) looks along ((px - W/2) / fx, (py - H/2) / fy, 1) in the camera frame
    (the reference's convention).  Returns a dict of per-pixel arrays over those pixels (`pix`: flat indices) -- depth, world ray, ground normal in the
    camera frame, per source: projection (u, v), expected validity and whether that expectation is clear of every silhouette and frame border
    (`clear`), the source ray cosine."""
    W, H, n_src = int(inp["W"]), int(inp["H"]), int(inp["n_src"])
    g = inp["_g"]
    s_sph, s_gnd = g["disc_s"]["sphere"], g["disc_s"]["ground"]
    fx = W / (2.0 * float(inp["tanfovx"])); fy = H / (2.0 * float(inp["tanfovy"]))
    w2c = np.asarray(inp["viewmatrix"], np.float64).reshape(4, 4).T
    Rw, C = w2c[:3, :3], np.asarray(inp["campos"], np.float64)
    py, px = np.mgrid[0:H, 0:W]
    rc = np.stack([(px.ravel() - 0.5 * W) / fx, (py.ravel() - 0.5 * H) / fy, np.ones(W * H)], axis=1)
    d = rc @ Rw                                           # world direction with camera-frame z = 1
    t = (float(GROUND_Z) - C[2]) / d[:, 2]                # ray/plane depth (camera z)
    X = C + t[:, None] * d
    px_world = 1.0 / min(fx, fy)                         # world size of a pixel (its longer side) per unit depth
    on = (t > 0) & (np.abs(X[:, 0]) < GROUND_HALF - 4 * s_gnd) & (np.abs(X[:, 1]) < GROUND_HALF - 4 * s_gnd)
    on &= _seg_dist(np.broadcast_to(C, X.shape), X) > SPHERE_R + 4 * s_sph + margin_px * px_world * t
    pix = np.flatnonzero(on)
    X, t, d = X[pix], t[pix], d[pix]
    ray = (X - C) / np.linalg.norm(X - C, axis=1, keepdims=True)
    n_cam = Rw @ np.array([0.0, 0.0, 1.0])               # the ground normal faces every camera above it
    src = inp["_srcs"] if inp.get("_srcs") is not None else [syn.make_camera(W, H, azimuth_deg=a) for a in SRC_AZIMUTHS[:n_src]]
    u, v, valid, clear, cos, S = [], [], [], [], [], []
    for s in src:
        ws = np.asarray(s["viewmatrix"], np.float64).reshape(4, 4).T
        Sc = np.linalg.inv(ws)[:3, 3]
        Xs = X @ ws[:3, :3].T + ws[:3, 3]
        us, vs = fx * Xs[:, 0] / Xs[:, 2] + 0.5 * W, fy * Xs[:, 1] / Xs[:, 2] + 0.5 * H
        inside = (us >= 0) & (us <= W - 1) & (vs >= 0) & (vs <= H - 1)
        edge = np.minimum(np.minimum(us, W - 1 - us), np.minimum(vs, H - 1 - vs))
        ds = _seg_dist(np.broadcast_to(Sc, X.shape), X)
        seen = ds > SPHERE_R
        u.append(us); v.append(vs); valid.append(inside & seen)
        # (the source's depth render blurs the sphere's silhouette by about a disc radius: measured on the oracle, every pixel whose validity differs
        # from `inside & seen` passes within 0.85 sphere-disc radii of the sphere)
        clear.append((np.abs(edge) > 1.0) & (np.abs(ds - SPHERE_R) > 2 * s_sph + px_world * Xs[:, 2]))
        sr = (X - Sc) / np.linalg.norm(X - Sc, axis=1, keepdims=True)
        cos.append((sr * ray).sum(1)); S.append(Sc)
    return {"pix": pix, "depth": t, "ray": ray, "n_cam": n_cam, "u": np.array(u), "v": np.array(v), "valid": np.array(valid), "clear": np.array(clear),
            "cos": np.array(cos), "src_pos": np.array(S), "campos": C}


def closed_form_errors(inp, out, valid_idx, final_T, tex_quant, say=print, mdd_bar=2e-5, figures=None):
    """Every geo output of one forward (`out`: the public planes, `valid_idx` (MAX_SRC, HW), `final_T` (HW,)) against surface_truth on the pixels of its
    mask that are covered (final_T < 0.5).  Prints each error beside its bar and returns the list of failures (empty = all within their bars).
    mdd_bar: the bar of the `min_depth_diff max (>= 1 valid source)` row -- that figure is the error of reading a source's DEPTH MAP between its texels,
    which grows with the curvature of the depth over a texel (tests/test_oracle_inside_camera.py derives the bars of its low cameras).  figures: a dict
    that receives every row's (error, bar, pixels judged) by name."""
    W, H, n_src = int(inp["W"]), int(inp["H"]), int(inp["n_src"])
    HW = W * H
    tr = surface_truth(inp)
    T = np.asarray(final_T).reshape(HW)[tr["pix"]]
    keep = T < 0.5
    pix = tr["pix"][keep]
    sel = lambda k, ch: np.asarray(out[k], np.float64).reshape(-1, HW)[ch][pix]
    vi = np.asarray(valid_idx).reshape(-1, HW)[:, pix]
    valid, clear = tr["valid"][:, keep], tr["clear"][:, keep]
    rows, fails = [], []

    def row(name, err, bar, n):
        rows.append((name, err, bar, n))
        if figures is not None:
            figures[name] = (err, bar, n)
        if not err <= bar:
            fails.append(name)

    # validity: slot k holds the k-th valid source, -1 ends the list (or all n_src slots are full)
    want = np.full((vi.shape[0], pix.size), -1, np.int64)
    cnt = np.zeros(pix.size, np.int64)
    for si in range(n_src):
        want[cnt[valid[si]], np.flatnonzero(valid[si])] = si
        cnt += valid[si]
    got = np.where(np.cumprod(vi != -1, axis=0) > 0, vi, -1)
    unamb = clear.all(0)
    same = np.all(got == want, axis=0)
    say("surface closed forms on %d ground pixels (%.1f %% of the frame); %d of them clear of every silhouette and source border, valid-source sets differ "
        "from the closed form on %d pixels next to one" % (pix.size, 100.0 * pix.size / HW, unamb.sum(), int((~same & ~unamb).sum())))
    row("valid-source sets (pixels that differ, clear px)", int((~same & unamb).sum()), max(2, int(1e-3 * unamb.sum())), int(unamb.sum()))
    assert unamb.sum() > 0.3 * pix.size and pix.size > 0.1 * HW, "the ground mask is too small to say anything"
    med = sel("median_depth", 0)
    row("median_depth max rel", float((np.abs(med - tr["depth"][keep]) / tr["depth"][keep]).max()), 1e-5, pix.size)
    ray = np.stack([sel("camera_ray", c) for c in range(3)], 1)
    row("camera_ray max |d|", float(np.abs(ray - tr["ray"][keep]).max()), 1e-5, pix.size)
    nrm = np.stack([sel("normal_map", c) for c in range(3)], 1) / (1.0 - T[keep])[:, None]
    row("normal_map / (1 - T) max |d|", float(np.abs(nrm - tr["n_cam"][None]).max()), 1e-5, pix.size)
    ok = same & unamb
    mdd = sel("min_depth_diff", 0)
    row("min_depth_diff max (>= 1 valid source)", float(mdd[ok & (cnt > 0)].max()) if (ok & (cnt > 0)).any() else 0.0, mdd_bar, int((ok & (cnt > 0)).sum()))
    row("min_depth_diff == 1 (no valid source): pixels that differ", int((mdd[ok & (cnt == 0)] != 1.0).sum()), 0, int((ok & (cnt == 0)).sum()))
    row("use_first_src_frame_mask: pixels that differ", int((sel("use_first_src_frame_mask", 0)[ok] != valid[0][ok]).sum()), 0, int(ok.sum()))
    coef = inp.get("_src_coef")
    e_pos = e_cos = e_warp = e_zero = 0.0
    w_bar = 1e-5
    if coef is not None and tex_quant:
        w_bar += 2.0 ** -9 * float((np.abs(coef[:, :, 1]) + np.abs(coef[:, :, 2])).max())      # 8-bit filter weights: <= 2^-9 of a texel step per axis
    n_slot = np.zeros(vi.shape[0], np.int64)
    for k in range(vi.shape[0]):
        for si in range(n_src):
            m = ok & (want[k] == si)
            if not m.any():
                continue
            n_slot[k] += m.sum()
            cf = np.stack([sel("cam_feat", 4 * k + c)[m] for c in range(4)], 1)
            e_pos = max(e_pos, float(np.abs(cf[:, :3] - (tr["campos"] - tr["src_pos"][si])[None]).max()))
            e_cos = max(e_cos, float(np.abs(cf[:, 3] - tr["cos"][si][keep][m]).max()))
            if coef is not None:
                us, vs = tr["u"][si][keep][m], tr["v"][si][keep][m]
                inner = (us >= 1) & (us <= W - 2) & (vs >= 1) & (vs <= H - 2)
                for c in range(3):
                    lin = coef[si, c, 0] + coef[si, c, 1] * us + coef[si, c, 2] * vs
                    e_warp = max(e_warp, float(np.abs(sel("warped_image", 3 * k + c)[m][inner] - lin[inner]).max(initial=0.0)))
        m = ok & (cnt <= k)
        if m.any():          # slots past the last valid source are zero
            e_zero = max(e_zero, max(float(np.abs(sel("cam_feat", 4 * k + c)[m]).max()) for c in range(4)),
                         max(float(np.abs(sel("warped_image", 3 * k + c)[m]).max()) for c in range(3)))
    row("cam_feat campos - src_campos max |d|", e_pos, 1e-5, int(n_slot.sum()))
    row("cam_feat ray cosine max |d|", e_cos, 1e-5, int(n_slot.sum()))
    if coef is not None:
        row("warped_image (linear sources) max |d|", e_warp, w_bar, int(n_slot.sum()))
    row("unused slots max |value|", e_zero, 0.0, int(ok.sum()))
    say("    valid sources per slot on those pixels: %s" % n_slot.tolist())
    for name, err, bar, n in rows:
        say("    %-50s %-10s bar %-10s (%d px)  %s" % (name, ("%.2e" % err) if isinstance(err, float) else err, ("%.2e" % bar) if isinstance(bar, float) else bar, n,
                                                   "ok" if err <= bar else "FAIL"))
    return fails


def regime(out, n_src, say=print, label=""):
    """The valid-source histogram of one forward, printed, with the two regime bars asserted."""
    hist, mean = valid_source_histogram(out["valid_src_idx"], out["final_T"], n_src)
    say("%svalid sources per covered pixel (%.1f %% of the frame covered): mean %.2f; share at 0..%d: %s" % (
        label, 100.0 * (np.asarray(out["final_T"]) < 0.5).mean(), mean, n_src, " ".join("%.3f" % h for h in hist)))
    assert mean >= MIN_MEAN_VALID, "the scene has drifted out of the multi-view-consistent regime"
    if n_src == 5:
        assert hist[5] >= MIN_ALL_VALID_5, "too few pixels with all five sources valid"
    return hist, mean


@pytest.mark.parametrize("n_src,L,seed", [(5, 4, 1), (5, 8, 2), (4, 4, 3), (3, 5, 4)])
def test_surface_scene_regime_and_closed_forms(n_src, L, seed):
    t0 = time.time()
    inp = surface_scene(P=60000, W=480, H=272, seed=seed, n_src=n_src, L=L, images="linear")
    out = oracle.forward(inp, cull=True)
    print("\n[surface n_src %d L %d seed %d] %d Gaussians, %d x %d" % (n_src, L, seed, inp["means3D"].shape[0], inp["W"], inp["H"]))
    regime(out, n_src)
    fails = closed_form_errors(inp, out, out["valid_src_idx"], out["final_T"], tex_quant=False)
    assert not fails, fails
    # the texture unit's 8-bit filter weights (rasterizer.TEX_QUANT): the warped colours move by at most 2^-9 of a texel step, nothing else does
    q = oracle.forward(inp, tex_quant=True, cull=True)
    fails = closed_form_errors(inp, q, q["valid_src_idx"], q["final_T"], tex_quant=True)
    assert not fails, fails
    print("    (%.1f s)" % (time.time() - t0))


def test_surface_scene_every_slot_and_the_full_list():
    """The regime in numbers that the old scenes never reach: slots 1-4 written on most covered pixels, and all five valid (no -1 terminator)."""
    inp = surface_scene(P=20000, W=176, H=112, seed=1, n_src=5, L=8)
    out = oracle.forward(inp, cull=True)
    cov = out["final_T"] < 0.5
    v = out["valid_src_idx"]
    for k in range(5):
        assert (v[k][cov] >= 0).mean() > 0.4, k
    assert (v[4][cov] >= 0).mean() == valid_source_histogram(v, out["final_T"], 5)[0][5]
    mdd = out["min_depth_diff"].reshape(-1)
    assert np.median(mdd[cov & (v[0] >= 0)]) < 1e-3
