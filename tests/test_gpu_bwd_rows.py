"""The per-Gaussian backward (csrc/preprocess_bwd.hip) alone, row by row against the float64 oracle (tests/bwd_rows.py).

ibgs_backward with R = 0 skips the blend and runs the per-Gaussian stage on whatever the caller's grad_acc rows hold (include/ibgs_rast.h), so every case here
seeds the rows itself: per column group, per SH layout, at the buffer ends, under both formats of a near-singular conic's row -- and one case per scene takes
the rows a real blend wrote.  Every pointer the calls get lies inside a tensor this file allocated; every output sits between sentinels that must survive."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from ibgs_amd import _lib
from tests import bwd_rows as br
from tests import hipref

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
PAD = 64          # floats in front of and behind every output: 256 bytes, so the output itself starts 16-byte aligned like its allocation


class Guarded:
    """A float32 tensor of `shape` inside a larger allocation filled with a sentinel."""

    def __init__(self, shape, dev, fill=SENTINEL):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[PAD:PAD + self.n].view(*shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0, "a sentinel buffer must start 16-byte aligned"

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all().item() and (self.buf[PAD + self.n:] == SENTINEL).all().item())

    def numpy(self):
        return self.t.cpu().numpy().copy()


def aligned_copy(t):
    """A contiguous copy of t that starts 16-byte aligned (the ABI's demand on split SH arrays; a small torch allocation need not be)."""
    n = t.numel()
    buf = torch.empty(n + 8, dtype=t.dtype, device=t.device)
    off = (-buf.data_ptr() % 16) // t.element_size()
    out = buf[off:off + n].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 0
    return out


def hip_forward(inp):
    """The product forward and what the backward needs of it; the oracle's forward beside it, with the stage's inputs asserted equal."""
    outs, lv, st = hipref.run_forward(inp, debug=True)
    ist = hipref.internal_state(outs, inp)
    node = next(outs[k].grad_fn for k in ("color", "median_depth", "normal_map") if outs.get(k) is not None and outs[k].grad_fn is not None)
    saved = node.saved_tensors
    ref = oracle.forward(inp, cull=True)
    radii = outs["radii"].cpu().numpy()
    assert np.array_equal(radii, ref["radii"])
    # (with cov3D_precomp the arena's cov3D is never written nor read: the stage takes the caller's array, and so does the restatement)
    pre = inp.get("cov3D_precomp")
    cov = np.ascontiguousarray(pre, np.float32) if pre is not None else ist["cov3D"]
    for a, b in ((cov, pre if pre is not None else ref["cov3D"]), (ist["rec"][:, 4:7], ref["conic_opacity"][:, :3]), (ist["rec"][:, 2], ref["conic_opacity"][:, 3])):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), "the forward's record / cov3D is not the oracle's"
    if inp.get("shs") is not None:
        _, bits = br.clamp_bits(ref["clamped"])
        used = ref["tiles_touched"] > 0
        assert np.array_equal(ist["clamped"][used], bits[used]) and not ist["clamped"][~used].any()
    return {"outs": outs, "lv": lv, "st": st, "ist": ist, "geom": saved[-3], "binning": saved[-2], "img": saved[-1], "ref": ref, "radii": radii,
            "fwd_like": {"radii": radii, "clamped": ist["clamped"] if inp.get("shs") is not None else np.zeros(radii.shape[0], np.uint8), "cov3D": cov}}


def _p(t):
    return None if t is None else t.data_ptr()


def run_stage(fw, inp, rows, flags=0, layout="combined", R=0, dL_dcolor=None):
    """ibgs_backward on the forward `fw` with the given grad_acc rows (R = 0: the per-Gaussian stage alone).  layout: "combined" | "split" (shs_rest).
    Returns (outputs as numpy arrays under the oracle's names, the rows after the call)."""
    lib = _lib.load()
    dev = torch.device("cuda")
    lv, st, outs = fw["lv"], fw["st"], fw["outs"]
    P = int(inp["means3D"].shape[0]); W, H = int(inp["W"]), int(inp["H"])
    geo = bool(inp.get("render_geo", False))
    shs = lv["shs"].detach().contiguous() if lv.get("shs") is not None else None
    M = int(shs.shape[1]) if shs is not None else 0
    factored = bool(flags & _lib.FLAG_SH_FACTORED)
    keep = []          # tensors the call reads: alive until it has run
    g = {"rows": Guarded((P, 16), dev, 0.0)}
    g["rows"].t.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
    for name, shape in (("dL_dmeans2D", (P, 3)), ("dL_dmeans2D_abs", (P, 3)), ("dL_dconic", (P, 4)), ("dL_dopacity", (P, 1)), ("dL_dcolors", (P, 3)),
                        ("dL_dmeans3D", (P, 3)), ("dL_dcov3D", (P, 6))):
        g[name] = Guarded(shape, dev)
    if geo:
        g["dL_dall_map"] = Guarded((P, 5), dev)
    if lv.get("scales") is not None:
        g["dL_dscales"] = Guarded((P, 3), dev); g["dL_drotations"] = Guarded((P, 4), dev)
    a = _lib.BackwardArgs()
    a.stream = torch.cuda.current_stream().cuda_stream
    a.P, a.D, a.M, a.W, a.H = P, int(inp.get("sh_degree", 0)), M, W, H
    a.R = int(R)
    a.means3D = _p(lv["means3D"].detach())
    if shs is not None and layout == "split":
        dc = aligned_copy(shs[:, :1]); rest = aligned_copy(shs[:, 1:]); keep += [dc, rest]
        a.shs = _p(dc); a.shs_rest = _p(rest)
        if not factored:
            g["dL_dsh_dc"] = Guarded((P, 1, 3), dev); g["dL_dsh_rest"] = Guarded((P, M - 1, 3), dev)
            a.dL_dsh = _p(g["dL_dsh_dc"].t); a.dL_dsh_rest = _p(g["dL_dsh_rest"].t)
    elif shs is not None:
        keep.append(shs)
        a.shs = _p(shs)
        if not factored:
            g["dL_dsh"] = Guarded((P, M, 3), dev)
            a.dL_dsh = _p(g["dL_dsh"].t)
    for name in ("colors_precomp", "scales", "rotations", "cov3D_precomp", "all_map"):
        t = lv.get(name)
        if t is not None:
            t = t.detach().contiguous(); keep.append(t)
            setattr(a, name, _p(t))
    a.scale_modifier = float(st.scale_modifier)
    a.bg = _p(st.bg); a.viewmatrix = _p(st.viewmatrix); a.projmatrix = _p(st.projmatrix); a.campos = _p(st.campos)
    a.tanfovx = float(st.tanfovx); a.tanfovy = float(st.tanfovy)
    a.n_src = int(st.nb_src_images)
    a.ref_to_src = _p(st.ref_to_src_list); a.src_cam_pos = _p(st.src_cam_pos); a.src_images = _p(st.src_images); a.src_depths = _p(st.src_rendered_depths)
    radii = outs["radii"].contiguous(); keep.append(radii)
    a.radii = _p(radii)
    a.geom = _p(fw["geom"]); a.img = _p(fw["img"])
    a.binning = _p(fw["binning"]) if R > 0 else None
    if geo:
        depth = outs["median_depth"].detach().contiguous(); warped = outs["warped_image"].detach().contiguous()
        tex = torch.zeros(int(lib.ibgs_required_tex(a.n_src, W, H)) + 256, dtype=torch.uint8, device=dev)
        a.buffer_length = int(st.buffer_length)
        tab = torch.zeros(int(lib.ibgs_required_geo_table_for(W, H, a.buffer_length)) + 256, dtype=torch.uint8, device=dev)
        keep += [depth, warped, tex, tab]
        a.out_depth = _p(depth); a.out_warped = _p(warped)
        a.tex = _p(tex); a.tex_bytes = tex.numel(); a.geo_table = _p(tab); a.geo_table_bytes = tab.numel()
        a.dL_dall_map = _p(g["dL_dall_map"].t)
    a.render_geo = int(geo)
    a.flags = int(flags) | _lib.FLAG_DEBUG
    if R > 0:
        gc = torch.as_tensor(dL_dcolor, dtype=torch.float32, device=dev).contiguous(); keep.append(gc)
        a.dL_dcolor = _p(gc)
        a.flags |= _lib.FLAG_DETERMINISTIC
        det = torch.zeros(int(lib.ibgs_required_deterministic_for(int(R), P, W, H, int(geo), int(a.flags))) + 256, dtype=torch.uint8, device=dev); keep.append(det)
        a.det_scratch = _p(det); a.det_scratch_bytes = det.numel()
    a.grad_acc = _p(g["rows"].t)
    a.dL_dmean2D = _p(g["dL_dmeans2D"].t); a.dL_dmean2D_abs = _p(g["dL_dmeans2D_abs"].t); a.dL_dconic = _p(g["dL_dconic"].t)
    a.dL_dopacity = _p(g["dL_dopacity"].t); a.dL_dcolors = _p(g["dL_dcolors"].t)
    a.dL_dmean3D = _p(g["dL_dmeans3D"].t); a.dL_dcov3D = _p(g["dL_dcov3D"].t)
    if "dL_dscales" in g:
        a.dL_dscale = _p(g["dL_dscales"].t); a.dL_drot = _p(g["dL_drotations"].t)
    rc = lib.ibgs_backward(ctypes.byref(a))
    torch.cuda.synchronize()
    assert rc >= 0, "ibgs_backward failed (%d): %s" % (rc, _lib.last_error())
    for name, t in g.items():
        assert t.intact(), "the sentinels around %s did not survive" % name
    out = {k: v.numpy() for k, v in g.items() if k != "rows"}
    if "dL_dsh_dc" in out:
        out["dL_dsh"] = np.concatenate([out.pop("dL_dsh_dc"), out.pop("dL_dsh_rest")], axis=1)
    del keep
    return out, g["rows"].numpy()


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def judge(inp, fw, rows, hip, rows_after, fmt, cleared=False, factored=False, per_class=False):
    """Every assertion of one call: the short outputs to their derived bounds, the chain's outputs to the row bar, exact zeros where nothing is computed, the
    rows back as they went in (or re-zeroed where consumed)."""
    rec = fw["ist"]["rec"]
    inter, refs, r64, live = br.reference(inp, fw["fwd_like"], rows, rec, fmt)
    vis = fw["radii"] > 0
    if cleared:
        assert not rows_after[live].any(), "consumed rows were not re-zeroed"
        assert bits_equal(rows_after[~live], rows[~live]), "rows that were not consumed changed"
    else:
        assert bits_equal(rows_after, rows), "the rows changed although IBGS_FLAG_CLEAR_GRAD_ACC was not given"
    if factored:          # dL_dcolors leaves as the clamp-masked rgb, and there is no dL_dsh
        flags, _ = br.clamp_bits(fw["fwd_like"]["clamped"])
        inter["dL_dcolors"] = np.where(live[:, None], rows[:, 8:11].astype(np.float64) * (1 - flags), 0.0)
        assert "dL_dsh" not in hip
    short = br.check_short(hip, inter, live)
    assert not short, "%d short outputs off their bound; first: %s" % (len(short), short[:5])
    names = [n for n in br.CHAIN_OUTPUTS if n in hip]
    hip = dict(hip)
    lf = (inter["cls"] == br.LFORM) & live
    if lf.any():
        hip["dL_dconic_lform"] = np.where(lf[:, None], hip["dL_dconic"], 0.0); names.append("dL_dconic_lform")
    ra = (inter["cls"] == br.ASSOC)
    classes = [("all", vis)] if not per_class else [("near-singular", vis & (inter["cls"] != br.ORDINARY)), ("ordinary", vis & (inter["cls"] == br.ORDINARY))]
    for tag, sel in classes:
        fails, worst = br.row_verdict(hip, refs, r64, sel, names=names)
        print("[bwd rows] %s rows %d, worst r / max(rho_i, rho_bar): %s" % (tag, int((sel & live).sum()), ", ".join("%s %.2f" % kv for kv in worst.items())))
        assert not fails, tag + ": " + br.verdict_message(fails)
    if (ra & live).any():          # RA_ASSOC rows, the reference's ill-conditioned chain: the whole-array arbiter rule as well
        fails, seen = br.array_verdict(hip, refs[0], r64, ra & live, [n for n in names if n != "dL_dconic_lform"])
        print("[bwd rows] RA_ASSOC rows %d, relL2 vs float64 (HIP | oracle fp32): %s" % (int((ra & live).sum()), ", ".join("%s %.1e|%.1e" % ((k,) + v) for k, v in seen.items())))
        assert not fails, "; ".join(fails)
    if "_zero_opacity" in inp:          # the `o > 0 ? ... : 0` guard is taken by rows that are computed
        zo = np.zeros(live.shape[0], bool); zo[inp["_zero_opacity"]] = True
        assert (zo & live & (rec[:, 2] == 0)).sum() >= 15, "too few zero-opacity Gaussians kept a live row"
    D = int(inp.get("sh_degree", 0))
    if "dL_dsh" in hip:
        assert not hip["dL_dsh"][:, (D + 1) ** 2:].any(), "coefficients above the active degree are not exact zeros"
    for name, v in hip.items():          # nothing is computed for an invisible Gaussian or an all-zero row
        assert not v[~live].any(), name
    return inter, live


def assert_populated(inp, ref, need):
    c = br.class_counts(inp, ref)
    for k, n in need.items():
        got = min(c[k]) if k == "clamp_masks" else c[k]
        assert got >= n, (k, c)
    return c


def seeded(inp, fw, group, seed):
    P = fw["radii"].shape[0]
    rows, zr, nz = br.seed_rows(P, group, fw["radii"], seed)
    vis = fw["radii"] > 0
    if P >= 1000:
        assert zr.size == 50 and nz.size == 10 and (np.signbit(rows[nz]).all() and not rows[nz].any())
    assert rows[~vis].any(axis=1).all(), "every invisible Gaussian gets a non-zero row"
    return rows


BASE_CLASSES = {"x_clamped": 100, "y_clamped": 100, "invisible": 100, "clamp_masks": 10, "zero_opacity": 20}
SMALL_CLASSES = {"x_clamped": 50, "y_clamped": 50, "invisible": 100, "clamp_masks": 10, "zero_opacity": 20}


# ---- 1. the chain, M = 16 combined, D = 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(br.GROUPS))
@pytest.mark.parametrize("mod", [1.0, 0.7])
def test_chain_per_column_group(mod, group):
    inp = br.base_scene(2000)
    inp["scale_modifier"] = mod
    fw = hip_forward(inp)
    assert_populated(inp, fw["ref"], BASE_CLASSES)
    rows = seeded(inp, fw, group, 100 + list(br.GROUPS).index(group))
    hip, after = run_stage(fw, inp, rows)
    judge(inp, fw, rows, hip, after, "lform")


# ---- 2. layouts and degrees ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,layout,factored", [(M, D, "combined", False) for M, D in br.LAYOUTS] + [(16, 3, "split", False), (9, 2, "split", False),
                                                                                                       (16, 3, "combined", True), (16, 3, "split", True)])
def test_layouts_and_degrees(M, D, layout, factored):
    inp = br.base_scene(1000, M=M, deg=D)
    fw = hip_forward(inp)
    assert_populated(inp, fw["ref"], SMALL_CLASSES)
    rows = seeded(inp, fw, "all", 200 + M + D)
    hip, after = run_stage(fw, inp, rows, flags=_lib.FLAG_SH_FACTORED if factored else 0, layout=layout)
    judge(inp, fw, rows, hip, after, "lform", factored=factored)


# ---- 3. no SH and no scales -----------------------------------------------------------------------------------------------------------------------------------------
def test_precomputed_colours_and_covariance():
    inp = br.precomp_scene(1000)
    fw = hip_forward(inp)
    c = assert_populated(inp, fw["ref"], {"x_clamped": 50, "y_clamped": 50, "invisible": 100})
    rows = seeded(inp, fw, "all", 300)
    hip, after = run_stage(fw, inp, rows)
    assert "dL_dsh" not in hip and "dL_dscales" not in hip and "dL_dcov3D" in hip
    _, live = judge(inp, fw, rows, hip, after, "lform")
    assert bits_equal(hip["dL_dcolors"][live], rows[live, 8:11])


# ---- 4. the ends ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,layout", [(16, 3, "combined"), (16, 3, "split"), (9, 2, "split")])
@pytest.mark.parametrize("P", br.END_SIZES)
def test_ends(P, M, D, layout):
    """An odd row count leaves 45 nrows and 3 nrows off a multiple of 4: the scalar tails of the split staging and of the split store."""
    inp = br._with_layout(br.end_scene(P), M, D)
    fw = hip_forward(inp)
    assert fw["ref"]["tiles_touched"][0] > 0
    rows = seeded(inp, fw, "all", 400 + P + M)
    assert br.live_rows(rows, fw["radii"]).any()
    hip, after = run_stage(fw, inp, rows, layout=layout)
    judge(inp, fw, rows, hip, after, "lform")


# ---- 5. IBGS_FLAG_CLEAR_GRAD_ACC ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["combined", "split"])
def test_clear_flag_changes_no_output_and_zeroes_what_it_consumed(layout):
    inp = br.base_scene(1000)
    fw = hip_forward(inp)
    assert_populated(inp, fw["ref"], SMALL_CLASSES)
    rows = seeded(inp, fw, "all", 600)
    hip0, after0 = run_stage(fw, inp, rows, layout=layout)
    hip1, after1 = run_stage(fw, inp, rows, flags=_lib.FLAG_CLEAR_GRAD_ACC, layout=layout)
    for k in hip0:
        assert bits_equal(hip0[k], hip1[k]), k
    judge(inp, fw, rows, hip1, after1, "lform", cleared=True)


# ---- 6. near-singular conics --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,flags", [("lform", 0), ("assoc", _lib.FLAG_REF_ARITH)])
def test_near_singular_conics(fmt, flags):
    inp = br.needle_scene()
    fw = hip_forward(inp)
    assert_populated(inp, fw["ref"], {"near_singular": 100})
    assert (br.near_singular(fw["ist"]["rec"]) & (fw["radii"] > 0)).sum() >= 100
    rows = seeded(inp, fw, "all", 500)
    hip, after = run_stage(fw, inp, rows, flags=flags)
    inter, live = judge(inp, fw, rows, hip, after, fmt, per_class=True)
    assert ((inter["cls"] == br.FORMATS[fmt]) & live).sum() >= 100


# ---- the blend's own rows -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["base", "needle"])
def test_rows_the_blend_writes(which):
    """A real backward (R > 0, deterministic, no clear flag): the rows survive the call, and the restatement applied to THOSE rows holds every output.
    Of the Gaussians that blend into some pixel in the oracle's backward (a non-zero accumulator there; at least 300, asserted), 90 % or more have a non-zero
    row here.  A share of the Gaussians WITH TILES cannot be asked for: on these scenes the pixels saturate behind the first few hundred Gaussians, and
    the oracle itself leaves most rows of Gaussians with tiles at zero (asserted below, so that the denominator is not changed back unnoticed)."""
    inp = dict(br.base_scene(2000) if which == "base" else br.needle_scene(), render_geo=False, all_map=None)
    fw = hip_forward(inp)
    H, W = inp["H"], inp["W"]
    g = np.random.default_rng(1).normal(size=(3, H, W)).astype(np.float32)
    zero = np.zeros((fw["radii"].shape[0], 16), np.float32)
    hip, rows = run_stage(fw, inp, zero, R=fw["ist"]["R"], dL_dcolor=g)
    gb = oracle.backward(inp, fw["ref"], g)
    blended = np.any([np.asarray(gb[k]).reshape(zero.shape[0], -1).any(axis=1) for k in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors")], axis=0)
    touched = rows.any(axis=1)
    tiled = fw["ref"]["tiles_touched"] > 0
    print("[bwd rows] %s: %d Gaussians with tiles, %d blended by the oracle, %d non-zero rows" % (which, tiled.sum(), blended.sum(), touched.sum()))
    assert blended.sum() >= 300 and (touched & blended).sum() >= 0.9 * blended.sum() and not touched[~tiled].any()
    assert blended.sum() < 0.5 * tiled.sum()
    inter, refs, r64, live = br.reference(inp, fw["fwd_like"], rows, fw["ist"]["rec"], "lform")
    short = br.check_short(hip, inter, live)
    assert not short, "%d short outputs off their bound; first: %s" % (len(short), short[:5])
    names = [n for n in br.CHAIN_OUTPUTS if n in hip]
    lf = (inter["cls"] == br.LFORM) & live
    if which == "needle":
        assert lf.sum() >= 50
        hip["dL_dconic_lform"] = np.where(lf[:, None], hip["dL_dconic"], 0.0); names.append("dL_dconic_lform")
    vis = fw["radii"] > 0
    for tag, sel in (("near-singular", vis & (inter["cls"] != br.ORDINARY)), ("ordinary", vis & (inter["cls"] == br.ORDINARY))):
        fails, worst = br.row_verdict(hip, refs, r64, sel, names=names)
        print("[bwd rows] %s %s rows %d, worst ratio: %s" % (which, tag, int((sel & live).sum()), ", ".join("%s %.2f" % kv for kv in worst.items())))
        assert not fails, tag + ": " + br.verdict_message(fails)
