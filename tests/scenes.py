"""Seeded scenes shared by the parity tests, the fixture generators under tests/golden/ and the tools."""
import numpy as np

import oracle
from ibgs_amd import synthetic as syn


def scene(P=4000, W=208, H=144, deg=3, seed=1, opacity="init", planes=False, scale_mul=1.0, anisotropy=None):
    inp = syn.make_scene(P, W, H, sh_degree=deg, seed=seed, opacity=opacity, with_planes=planes, anisotropy=anisotropy)
    if scale_mul != 1.0:
        inp["scales"] = (inp["scales"] * scale_mul).astype(np.float32)
        if planes:
            inp["all_map"] = syn.plane_all_map(inp["means3D"], inp["scales"], inp["rotations"], inp["_cam"])
    return inp


def camera_at(W, H, eye, target, fovx, fovy):
    """A camera at `eye` looking at `target` with the two fields of view given INDEPENDENTLY (make_camera derives fovy from fovx's focal length, so
    fx == fy there; here fx = W / (2 tan(fovx / 2)) and fy = H / (2 tan(fovy / 2)) are whatever the arguments make them)."""
    R, t = syn.look_at_camera(eye, target)
    return syn.camera_from_pose(W, H, R, t, fovx, fovy)


def inside_cloud(P, W, H, eye, target, fovx, fovy, seed, deg, opacity, scale_mul=1.0, anisotropy=None, planes=False):
    """make_scene's random cloud (half-extent 1.3) seen by camera_at from an eye INSIDE it: most Gaussians fail the near cull, half lie behind the camera,
    the survivors come as close as z = 0.2 with footprints many times the frame, and most visible centres are off the frame and beyond the 1.3 tan clamp.
    Returns make_gaussians' arrays plus make_scene's input dict with that camera (also as inp["_cam"])."""
    g = syn.make_gaussians(P, seed, sh_degree=deg, opacity=opacity, anisotropy=anisotropy)
    if scale_mul != 1.0:
        g["scales"] = (g["scales"] * scale_mul).astype(np.float32)
    cam = camera_at(W, H, eye, target, fovx, fovy)
    inp = dict(g)
    inp.update({"W": W, "H": H, "tanfovx": cam["tanfovx"], "tanfovy": cam["tanfovy"], "viewmatrix": cam["viewmatrix"], "projmatrix": cam["projmatrix"],
                "campos": cam["campos"], "bg": np.zeros(3, np.float32), "sh_degree": deg, "scale_modifier": 1.0, "render_geo": False,
                "render_depth_only": False, "n_src": 1, "buffer_length": 4, "depth_thr": 0.01, "_cam": cam})
    if planes:
        inp["all_map"] = syn.plane_all_map(g["means3D"], g["scales"], g["rotations"], cam)
    return inp


def giant_needles(P=300, W=208, H=144, seed=5, stretch=4.0, thin=0.05, deg=1, opacity="trained"):
    """Needles far longer than the frame and thinner than a pixel: the fp32 inversion of cov2D leaves conics within rounding of singular
    (some indefinite), the regime in which the reference's `power > 0` test (forward.cu:420, backward.cu:645) decides which pairs blend.
    The longest axis of every "needle" Gaussian is stretched again, the other two shrunk."""
    inp = scene(P=P, W=W, H=H, deg=deg, seed=seed, opacity=opacity, anisotropy="needle")
    s0 = inp["scales"]
    k = np.argmax(s0, axis=1); rows = np.arange(P)
    s = s0 * thin
    s[rows, k] = s0[rows, k] * stretch
    inp["scales"] = s.astype(np.float32)
    return inp


SRC_AZIMUTHS = (7.0, -7.0, 14.0, -14.0, 21.0)         # add_sources' source views (make_camera azimuths; the reference view is at 0)


def add_sources(inp, n_src=3, L=4, seed=5, depth=None, srcs=None):
    """Geo inputs for `inp`: source views (the orbit cameras at SRC_AZIMUTHS, or the camera dicts `srcs`, which then set n_src), uniform-noise source
    images and, unless `depth` is given, the oracle's depth-only renders of the same Gaussians from those views as source depths."""
    W, H = inp["W"], inp["H"]
    if srcs is None:
        srcs = [syn.make_camera(W, H, azimuth_deg=a) for a in SRC_AZIMUTHS[:n_src]]
    n_src = len(srcs)
    r2s, scp = syn.ref_to_src(inp["_cam"], srcs)
    rng = np.random.default_rng(seed)
    if depth is None:   # plausible source depths: the oracle's own depth-only render of each source view
        deps = []
        for s in srcs:
            d = dict(inp); d.update(viewmatrix=s["viewmatrix"], projmatrix=s["projmatrix"], campos=s["campos"],
                                    render_geo=False, render_depth_only=True, buffer_length=4,
                                    all_map=syn.plane_all_map(inp["means3D"], inp["scales"], inp["rotations"], s))
            deps.append(oracle.forward(d)["median_depth"])
        depth = np.stack(deps)
    inp = dict(inp)
    inp.update(render_geo=True, n_src=n_src, buffer_length=L, ref_to_src=r2s, src_cam_pos=scp,
               src_images=rng.uniform(0, 1, (n_src, 3, H, W)).astype(np.float32), src_depths=depth.astype(np.float32), depth_thr=0.05)
    return inp


def consumer_scene():
    """The scene of tests/golden/consumer.npz (make_consumer_fixture.py): small enough for a committed fixture, H and W
    divisible by 4 (the reference's ColorFusionResidualNet pools twice), 3 sources so that every slot level is used."""
    return add_sources(scene(P=700, W=48, H=32, deg=1, seed=61, opacity="trained", planes=True, scale_mul=2.2), n_src=3, L=4)


def fuse_color_inputs(render, cam_feat, warped_image, camera_ray, nb_visible_src_frames=3):
    """numpy restatement of how the reference's only consumer reads the geo outputs (color_aggregation_network.py:156-198,
    231-233, no exposure correction, residual_resolution_scale 1): slot k of `warped_image` = channels 3k..3k+2, slot k of
    `cam_feat` = channels 4k..4k+3; the number of slot levels used = the count of levels whose warped colours are not all
    zero (capped); a slot of a pixel is valid iff the sum of its 4 cam_feat values is > 0; per-view features = [warped -
    render (masked), cam_feat].  Returns (x_views (HW, levels, 7), ray_dir (HW, 3), c_3dgs (HW, 3), levels)."""
    _, H, W = render.shape
    wl = warped_image.reshape(-1, 3, H, W).transpose(2, 3, 0, 1)             # (H, W, 5, 3)
    ft = cam_feat.reshape(-1, 4, H, W).transpose(2, 3, 0, 1)                 # (H, W, 5, 4)
    levels = min(int(np.count_nonzero(wl.sum(axis=(0, 1, 3)))), nb_visible_src_frames)
    ft, wl = ft[:, :, :levels], wl[:, :, :levels]
    valid = (ft.sum(-1, keepdims=True) > 0.0).astype(np.float32)
    resid = (wl - render.transpose(1, 2, 0)[:, :, None, :]) * valid
    x = np.concatenate([resid, ft], axis=-1).reshape(H * W, levels, 7)
    return x, camera_ray.reshape(3, -1).T, render.transpose(1, 2, 0).reshape(-1, 3), levels


# ---- a multi-view-consistent scene: opaque discs on a sphere and a ground square ---------------------------------------------------------
SPHERE_R = 0.8                    # sphere centred at the origin
GROUND_Z = np.float32(-0.8)       # the ground square's plane z = GROUND_Z (the float32 value: the discs lie on it exactly) ...
GROUND_HALF = 1.6                 # ... for |x|, |y| <= GROUND_HALF


def quat_z_to(n):
    """(P,4) unit quaternions (w,x,y,z) of the shortest rotations taking e_z onto the unit vectors n (P,3); n = -e_z takes a half turn about x."""
    n = np.asarray(n, np.float64)
    q = np.stack([1.0 + n[:, 2], -n[:, 1], n[:, 0], np.zeros(n.shape[0])], axis=1)
    q[q[:, 0] < 1e-9] = (0.0, 1.0, 0.0, 0.0)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def surface_discs(P, seed, deg=2, ground_frac=0.55, scale_mul=1.0, opacity=0.9):
    """Gaussians that form two opaque surfaces: flat discs tangent to the sphere and discs lying on the ground square.  Scales (s, s, 0.01 s) with s chosen
    so that each surface is covered by ~3 disc areas, rotations taking z onto the outward surface normal (the smallest axis IS the normal), opacity
    `opacity`, SH colours as in synthetic.make_gaussians.  Returns make_gaussians' dict plus "normal" (P,3) and "offset" (P,1) zeros -- the learnt plane
    parameters that describe the same planes (ibgs_amd.simple_scene.SimpleGaussians) -- and "disc_s" {"sphere": s, "ground": s}."""
    rng = np.random.default_rng(seed)
    ng = int(round(ground_frac * P)); ns = P - ng
    d = rng.normal(size=(ns, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    xy = rng.uniform(-GROUND_HALF, GROUND_HALF, size=(ng, 2))
    xyz = np.concatenate([SPHERE_R * d, np.concatenate([xy, np.full((ng, 1), GROUND_Z)], axis=1)]).astype(np.float32)
    nrm = np.concatenate([d, np.tile([0.0, 0.0, 1.0], (ng, 1))]).astype(np.float32)
    s_sph = scale_mul * np.sqrt(4 * np.pi * SPHERE_R ** 2 / max(ns, 1))
    s_gnd = scale_mul * np.sqrt((2 * GROUND_HALF) ** 2 / max(ng, 1))
    s = np.concatenate([np.full(ns, s_sph), np.full(ng, s_gnd)])
    scales = np.stack([s, s, 0.01 * s], axis=1).astype(np.float32)
    g = syn.make_gaussians(P, seed, sh_degree=deg, max_coeffs=(deg + 1) ** 2)
    g.update(means3D=xyz, scales=scales, rotations=quat_z_to(nrm).astype(np.float32), opacities=np.full((P, 1), opacity, np.float32),
             normal=nrm, offset=np.zeros((P, 1), np.float32), disc_s={"sphere": float(s_sph), "ground": float(s_gnd)})
    return g


def linear_source_images(n_src, W, H, seed):
    """Source images that are LINEAR in the source pixel coordinates: channel c of source k = a + b u / W + c v / H (values in [0.1, 0.9]).
    Bilinear sampling reproduces them exactly, so a warped colour has a closed form.  Returns (images (n,3,H,W) float32, coefficients (n,3,3) float64 =
    [a, b / W, c / H] per (source, channel))."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.4, 0.6, (n_src, 3)); b = rng.uniform(-0.3, 0.3, (n_src, 3)); c = rng.uniform(-0.3, 0.3, (n_src, 3))
    coef = np.stack([a, b / W, c / H], axis=-1)
    u = np.arange(W, dtype=np.float64)[None, None, None, :]; v = np.arange(H, dtype=np.float64)[None, None, :, None]
    img = coef[..., 0, None, None] + coef[..., 1, None, None] * u + coef[..., 2, None, None] * v
    return img.astype(np.float32), coef


def surface_scene(P=20000, W=176, H=112, seed=1, n_src=5, L=4, deg=2, images="noise", depth_thr=0.01, ref_pose=None, src_poses=None, fovx=None, fovy=None,
                  **disc_kw):
    """The multi-view-consistent geo scene: surface_discs seen from make_camera(azimuth 0) with add_sources' n_src source views, source depths = the
    oracle's depth-only renders of the same discs from those views, depth_thr 0.01 (the trainer's).  images = "noise" (add_sources' uniform noise) or
    "linear" (linear_source_images; the coefficients are returned as inp["_src_coef"]).  inp["_g"] holds surface_discs' dict.
    With ref_pose = (eye, target), src_poses = [(eye, target), ...] and fovx, fovy the reference and source views are camera_at's instead (all with the
    same two fields of view; n_src = len(src_poses)), and the source cameras are returned as inp["_srcs"]."""
    g = surface_discs(P, seed, deg=deg, **disc_kw)
    posed = ref_pose is not None
    assert posed == (src_poses is not None) == (fovx is not None) == (fovy is not None), "ref_pose, src_poses, fovx and fovy come together"
    srcs = None
    if posed:
        cam = camera_at(W, H, ref_pose[0], ref_pose[1], fovx, fovy)
        srcs = [camera_at(W, H, e, t, fovx, fovy) for e, t in src_poses]
        n_src = len(srcs)
    else:
        cam = syn.make_camera(W, H)
    inp = {k: g[k] for k in ("means3D", "shs", "scales", "rotations", "opacities")}
    inp.update({"W": W, "H": H, "tanfovx": cam["tanfovx"], "tanfovy": cam["tanfovy"], "viewmatrix": cam["viewmatrix"], "projmatrix": cam["projmatrix"],
                "campos": cam["campos"], "bg": np.zeros(3, np.float32), "sh_degree": deg, "scale_modifier": 1.0, "render_geo": False,
                "render_depth_only": False, "n_src": 1, "buffer_length": L, "depth_thr": depth_thr, "_cam": cam,
                "all_map": syn.plane_all_map(g["means3D"], g["scales"], g["rotations"], cam)})
    inp = add_sources(inp, n_src=n_src, L=L, seed=seed + 1, srcs=srcs)
    inp["depth_thr"] = depth_thr
    inp["_g"] = g
    if posed:
        inp["_srcs"] = srcs
    if images == "linear":
        inp["src_images"], inp["_src_coef"] = linear_source_images(n_src, W, H, seed + 2)
    return inp


def valid_source_histogram(valid_src_idx, final_T, n_src):
    """Share of the COVERED pixels (final_T < 0.5) at each count 0..n_src of valid sources (valid_src_idx (MAX_SRC, HW): slot k holds the k-th valid
    source, -1 ends the list), and their mean count.  Returns (hist (n_src + 1,), mean)."""
    v = np.asarray(valid_src_idx).reshape(valid_src_idx.shape[0], -1)
    cnt = np.cumprod(v != -1, axis=0).sum(axis=0)
    cov = np.asarray(final_T).reshape(-1) < 0.5
    c = cnt[cov]
    hist = np.bincount(c, minlength=n_src + 1)[:n_src + 1] / max(1, c.size)
    return hist, float(c.mean()) if c.size else 0.0
