"""Builds libibgs_rast.so (the gfx950 HIP library behind include/ibgs_rast.h) in-tree with hipcc.

No torch.utils.cpp_extension here: under ROCm it would hipify the sources, and the library has no
torch types in its ABI anyway.  One hipcc invocation per translation unit (parallel), then a link.
preprocess.hip is compiled with -ffp-contract=off so its integer outputs are bit-identical to the
C oracle (see the header of that file); so is scan_sort.hip, whose depth sort launches also run the SH
colours (sh_color.h); so is tsdf.hip, whose f32 operation order is part of the TSDF contract (its header, tests/tsdf_ref.py), and mesh.hip (the f64 triangle areas), and mesh_eval.hip (f64 sample positions, f32 squared distances),
and registration.hip (the f64 transform, crop, voxel index and moment terms), and dtu.hip (the f32 projection chain of the vertex culling, the f64 filters).
ssim.hip takes no such flag: its contract is a tolerance, its filter passes are fma chains, and the per-pixel expressions that must not be contracted say so
themselves (#pragma clang fp contract(off)); geoloss.hip, which runs the same passes and forms (csrc/shared/ssim_window.h), is built the same way, and so is coloragg.hip
(the colour aggregation front end: a tolerance contract, its products are matrix-core fma chains), and hourglass.hip (the CNN behind it, forward only: the same), and hgtrain.hip (that CNN's backward: the same),
and hghalf.hip (that CNN's forward in half precision: the same; csrc/shared/hg_net.h states the network -- its layers, its stage arena, its host-side checks -- once for
these units), and hghtrain.hip (that CNN's backward in half precision: the same; csrc/shared/conv_tile_f16.h states the f16 matrix-core convolution, the octet read and
the recomputed head once for these two), and lpips.hip (LPIPS on VGG16 for the image evaluation: a tolerance contract as well, its convolutions
are the same matrix-core fma chains -- csrc/shared/conv_tile.h states their 16 x 16 tile and the rule by which a layer reads its source once for it and the three
hourglass units; the z-score's two operations say themselves that they are not contracted), and exposure.hip (the exposure correction of
the colour network: a tolerance contract too; its moments add exact f64 products of f32 values, so contraction cannot change them, and its application is an fma chain), and resample.hip
(the reduced-resolution colour tail: a tolerance contract; its blends are written as fmaf, its MLP is the matrix-core chain it shares with coloragg.hip
(csrc/shared/pv_mlp.h), and the expressions that must not be contracted say so themselves), and rsztrain.hip (that tail's backward: the same chain, the
blends it shares with resample.hip (csrc/shared/rsz_taps.h), the per-slot backward it shares with coloragg.hip (csrc/shared/pv_mlp_bwd.h), and a gather whose
products and sums say themselves that they are not contracted), and export.hip (the frame export: a contract of equal bytes, and no flag either: the unit
states at file scope that none of its operations is contracted).
csrc/block_ops.h holds the workgroup reduce / scan helpers of knn, tsdf, mesh, mesh_eval, registration and dtu (no multiply-add in them: the flag above does
not bear on them); ibgs_amd/_device.py is the Python side those six units share.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libibgs_rast.so")
SOURCES = ["api", "preprocess", "scan_sort", "binning", "render_fwd", "render_bwd", "preprocess_bwd", "knn", "adam", "compact", "deterministic", "loss", "depth_normal", "activate", "tsdf", "mesh", "mesh_eval", "registration", "dtu", "ssim", "geoloss", "coloragg", "exposure", "export", "resample", "rsztrain", "lpips", "hgtrain", "hghalf", "hghtrain", "hourglass"]
EXTRA = {
    "preprocess": ["-ffp-contract=off"],           # bit-identical to the oracle (see preprocess.hip)
    "scan_sort": ["-ffp-contract=off"],            # runs the SH colours of sh_color.h too (the sort itself has no float arithmetic)
    "tsdf": ["-ffp-contract=off"],                 # the update / marching-cubes operation order is the contract (tests/tsdf_ref.py restates it)
    "mesh": ["-ffp-contract=off"],                 # a triangle's f64 area is the restatement's to the bit (tests/mesh_ref.py); the rest is integers
    "mesh_eval": ["-ffp-contract=off"],            # the f64 sample positions and the f32 squared distances are the restatement's to the bit (tests/mesh_eval_ref.py)
    "registration": ["-ffp-contract=off"],         # the f64 transform, crop crossings, voxel indices and moment terms are the restatement's to the bit (tests/registration_ref.py)
    "dtu": ["-ffp-contract=off"],                  # the f32 projection / grid_sample chain of the vertex culling and the f64 filters are the restatement's to the bit (tests/dtu_ref.py): no fma
    # no SLP packing: v_pk_*_f32 is not faster than two scalar VALU ops on gfx950 and costs v_mov / s_nop glue
    "render_fwd": ["-fno-slp-vectorize"],
    "render_bwd": ["-fno-slp-vectorize", "-fno-signed-zeros"],
}
ARCH = "gfx950"
BASE_FLAGS = ["-O3", "-fPIC", "-std=c++17"]


def compile_flags(name):
    """Every flag a translation unit is compiled with, target included (tools/hot_loop_isa.py reads its assembly with the same list)."""
    return ["--offload-arch=" + ARCH] + BASE_FLAGS + EXTRA.get(name, [])
# headers that not every unit includes: hashed into the profile stamps (tu_shas) of the units they are listed under and of no other, rebuild triggers like the
# others.  Those under csrc/shared/ have two to four users each; they sit in a subdirectory because every csrc/*.h enters every unit's stamp.  A unit's list
# is every header it includes, directly or through another, outside csrc/*.h and include/ibgs_rast.h.
SSIM_WINDOW_H, PV_MLP_H, PV_MLP_BWD_H, RSZ_TAPS_H, HG_NET_H, CONV_TILE_H, CONV_TILE_F16_H = (os.path.join(CSRC, "shared", f) for f in ("ssim_window.h", "pv_mlp.h", "pv_mlp_bwd.h", "rsz_taps.h", "hg_net.h", "conv_tile.h", "conv_tile_f16.h"))
UNIT_HEADERS = {"tsdf": [os.path.join(HERE, "..", "include", "ibgs_tsdf.h")], "mesh": [os.path.join(HERE, "..", "include", "ibgs_mesh.h")],
                "mesh_eval": [os.path.join(HERE, "..", "include", "ibgs_mesh_eval.h")],
                "registration": [os.path.join(HERE, "..", "include", "ibgs_registration.h")],
                "dtu": [os.path.join(HERE, "..", "include", "ibgs_dtu.h")],
                "ssim": [os.path.join(HERE, "..", "include", "ibgs_ssim.h"), SSIM_WINDOW_H],
                "geoloss": [os.path.join(HERE, "..", "include", "ibgs_geo_loss.h"), SSIM_WINDOW_H],
                "coloragg": [os.path.join(HERE, "..", "include", "ibgs_color_agg.h"), PV_MLP_H, PV_MLP_BWD_H],
                "hourglass": [os.path.join(HERE, "..", "include", "ibgs_hourglass.h"), HG_NET_H, CONV_TILE_H],
                "hgtrain": [os.path.join(HERE, "..", "include", "ibgs_hg_train.h"), os.path.join(HERE, "..", "include", "ibgs_hourglass.h"), HG_NET_H, CONV_TILE_H],
                "hghalf": [os.path.join(HERE, "..", "include", "ibgs_hg_half.h"), os.path.join(HERE, "..", "include", "ibgs_hourglass.h"), HG_NET_H, CONV_TILE_H, CONV_TILE_F16_H],
                "hghtrain": [os.path.join(HERE, "..", "include", "ibgs_hg_half_train.h"), os.path.join(HERE, "..", "include", "ibgs_hg_half.h"),
                             os.path.join(HERE, "..", "include", "ibgs_hourglass.h"), HG_NET_H, CONV_TILE_H, CONV_TILE_F16_H],
                "lpips": [os.path.join(HERE, "..", "include", "ibgs_lpips.h"), CONV_TILE_H],
                "exposure": [os.path.join(HERE, "..", "include", "ibgs_exposure.h")],
                "export": [os.path.join(HERE, "..", "include", "ibgs_export.h")],
                "resample": [os.path.join(HERE, "..", "include", "ibgs_resample.h"), PV_MLP_H, RSZ_TAPS_H],
                "rsztrain": [os.path.join(HERE, "..", "include", "ibgs_resample_train.h"), os.path.join(HERE, "..", "include", "ibgs_resample.h"), PV_MLP_H, PV_MLP_BWD_H,
                             RSZ_TAPS_H]}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _newest_dep():
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))]
    deps.append(os.path.join(HERE, "..", "include", "ibgs_rast.h"))
    deps += [h for name in SOURCES for h in UNIT_HEADERS.get(name, [])]
    return max(os.path.getmtime(d) for d in deps)


def _code_only(text):
    """C / HIP source without comments and blank lines (string literals in these sources never hold comment markers)."""
    import re
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return "\n".join(l.rstrip() for l in text.split("\n") if l.strip())


def csrc_sha():
    """Fingerprint of the kernel sources (csrc/*.hip, csrc/*.h, include/ibgs_rast.h), comments and blank lines excluded.
    profiles/summarize.py stamps it into the committed rocprofv3 summaries and bench.py quotes profile-derived numbers only when the
    stamp matches this tree."""
    import hashlib
    h = hashlib.sha1()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(_code_only(open(os.path.join(CSRC, f), "r").read()).encode())
    h.update(_code_only(open(os.path.join(HERE, "..", "include", "ibgs_rast.h"), "r").read()).encode())
    return h.hexdigest()[:12]


# which translation unit a kernel of the step lives in (substring of its name -> TU): profile-derived numbers of a kernel stay valid while ITS
# unit (and the headers) are unchanged -- a host-only edit of api.hip does not make the blend kernels' counters stale
# ("meval_" first: the later entries match by substring, and a meval_cell_count would otherwise be credited to binning; "dtu_" before "mesh_" and "scan_":
# a dtu_emit_mesh_* or dtu_scan_* would otherwise go to those units; "lpips_" ahead of every entry that could claim one of its kernels by substring -- all but
# "meval_", which no lpips_* name holds; no other unit's substring occurs in an expo_* name, and "expo_" in no other unit's kernel; the same holds for "rsz_" and "rzt_", and for "fexp_")
KERNEL_TU = (("meval_", "mesh_eval"), ("lpips_", "lpips"), ("geoloss_", "geoloss"), ("cagg_", "coloragg"), ("expo_", "exposure"), ("fexp_", "export"), ("rsz_", "resample"), ("rzt_", "rsztrain"), ("pcreg_", "registration"), ("dtu_", "dtu"), ("ssim_", "ssim"), ("tsdf_", "tsdf"), ("mesh_", "mesh"), ("render_fwd", "render_fwd"), ("pack_rgba", "render_fwd"), ("render_bwd", "render_bwd"), ("geo_window", "render_bwd"), ("tile_order", "render_bwd"),
             ("preprocess_bwd", "preprocess_bwd"), ("sh_grad", "preprocess_bwd"), ("preprocess_kernel", "preprocess"), ("sh_color", "preprocess"), ("mark_visible", "preprocess"),
             ("onesweep", "scan_sort"), ("radix", "scan_sort"), ("scan_", "scan_sort"), ("cell_", "binning"), ("expand_", "binning"), ("tile_ranges", "binning"),
             ("rendered_note", "api"), ("l1_", "loss"), ("depth_normal", "depth_normal"), ("activate_", "activate"), ("adam", "adam"), ("compact", "compact"), ("det_", "deterministic"), ("knn", "knn"), ("hght_", "hghtrain"), ("hgh_", "hghalf"), ("hgb_", "hgtrain"), ("hg_", "hourglass"))


def tu_of(kernel_name):
    for sub, tu in KERNEL_TU:
        if sub in kernel_name:
            return tu
    return None


# units that are built and attributed like the others but carry no profile stamp: no committed rocprofv3 summary holds a kernel of theirs and bench.py quotes
# none (the frame export runs after the step, outside everything bench.py measures; its numbers are tools/bench_export.py's own text, profiles/export.txt).
# tu_of() still names the unit for such a kernel, and bench.py's tu_shas().get(unit) then finds no stamp: nothing stale can be quoted for it.
UNSTAMPED = ("export",)


def tu_shas():
    """{translation unit: fingerprint of its .hip + every header (csrc/*.h, include/ibgs_rast.h)}, comments and blank lines excluded; the units of UNSTAMPED have none."""
    import hashlib
    hdr = hashlib.sha1()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".h"):
            hdr.update(f.encode()); hdr.update(_code_only(open(os.path.join(CSRC, f), "r").read()).encode())
    hdr.update(_code_only(open(os.path.join(HERE, "..", "include", "ibgs_rast.h"), "r").read()).encode())
    out = {}
    for name in SOURCES:
        if name in UNSTAMPED:
            continue
        h = hdr.copy()
        h.update(_code_only(open(os.path.join(CSRC, name + ".hip"), "r").read()).encode())
        for u in UNIT_HEADERS.get(name, []):
            h.update(_code_only(open(u, "r").read()).encode())
        h.update(" ".join(EXTRA.get(name, [])).encode())
        out[name] = h.hexdigest()[:12]
    return out


def needs_build():
    if not os.path.exists(LIB):
        return True
    newest = _newest_dep()
    objs = [os.path.join(OBJ, n + ".o") for n in SOURCES]
    return any((not os.path.exists(o)) or os.path.getmtime(o) < newest for o in objs) or os.path.getmtime(LIB) < newest


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    hdr_time = max([os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h")]
                   + [os.path.getmtime(os.path.join(HERE, "..", "include", "ibgs_rast.h"))])

    def compile_one(name):
        src = os.path.join(CSRC, name + ".hip")
        obj = os.path.join(OBJ, name + ".o")
        newest = max([os.path.getmtime(src), hdr_time] + [os.path.getmtime(h) for h in UNIT_HEADERS.get(name, [])])
        if (not force) and os.path.exists(obj) and os.path.getmtime(obj) >= newest:
            return obj
        cmd = [hipcc] + compile_flags(name) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    if force or (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(o) for o in objs):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
