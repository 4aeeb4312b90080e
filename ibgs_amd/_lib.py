"""ctypes binding of libibgs_rast.so (C ABI declared in include/ibgs_rast.h).

The library is the product path: if it is missing or fails to load this module raises -- there is
no Python / PyTorch / oracle fallback (a silent fallback would void every parity claim).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# IBGS_LIB: another build of the same ABI (A/B runs of two builds on ONE box: tools/ab_lib.sh); never a fallback -- a path that does not load raises
LIB_PATH = os.environ.get("IBGS_LIB") or os.path.join(_HERE, "libibgs_rast.so")

MAX_SRC = 5
MAX_BUFFER_LENGTH = 8
FLAG_DEBUG = 1
FLAG_TEX_QUANT = 2
FLAG_NO_TILE_CULL = 4
FLAG_CLEAR_GRAD_ACC = 8
FLAG_SH_FACTORED = 16
FLAG_TILE_WAVES = 32
FLAG_QUADRANT_WAVES = 64
FLAG_DETERMINISTIC = 128
FLAG_TEX_PACKED = 256
FLAG_NO_REF_POWER_SKIP = 512
FLAG_NO_ABS_GRAD = 1024
FLAG_NO_PLAIN_CHUNKS = 2048
FLAG_REF_ARITH = 4096
FLAG_SRC_DEPTH_SLOTS = 8192
PLANE_NONE, PLANE_LEARNT, PLANE_SMALLEST_AXIS = 0, 1, 2
MAX_VIEWS = 8

c_float_p = ctypes.c_void_p  # raw device pointers travel as integers

ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class ForwardArgs(ctypes.Structure):
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("P", ctypes.c_int32), ("D", ctypes.c_int32), ("M", ctypes.c_int32),
        ("W", ctypes.c_int32), ("H", ctypes.c_int32),
        ("means3D", c_float_p), ("shs", c_float_p), ("colors_precomp", c_float_p), ("opacities", c_float_p),
        ("scales", c_float_p), ("rotations", c_float_p), ("cov3D_precomp", c_float_p), ("all_map", c_float_p),
        ("scale_modifier", ctypes.c_float),
        ("bg", c_float_p), ("viewmatrix", c_float_p), ("projmatrix", c_float_p), ("campos", c_float_p),
        ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float),
        ("n_src", ctypes.c_int32),
        ("ref_to_src", c_float_p), ("src_cam_pos", c_float_p), ("src_images", c_float_p), ("src_depths", c_float_p),
        ("buffer_length", ctypes.c_int32), ("depth_error_threshold", ctypes.c_float),
        ("prefiltered", ctypes.c_int32), ("render_geo", ctypes.c_int32), ("render_depth_only", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("geom", ctypes.c_void_p), ("geom_bytes", ctypes.c_size_t),
        ("img", ctypes.c_void_p), ("img_bytes", ctypes.c_size_t),
        ("binning_alloc", ALLOC_FN), ("binning_user", ctypes.c_void_p),
        ("tex", ctypes.c_void_p), ("tex_bytes", ctypes.c_size_t),
        ("out_color", c_float_p), ("radii", ctypes.c_void_p), ("out_normal", c_float_p), ("out_depth", c_float_p),
        ("out_cam_feat", c_float_p), ("out_warped", c_float_p), ("out_min_depth_diff", c_float_p),
        ("out_camera_ray", c_float_p), ("out_mask", ctypes.c_void_p),
        ("rendered_hint", ctypes.c_int64),
        ("plane_normal", c_float_p), ("plane_offset", c_float_p), ("plane_mode", ctypes.c_int32),
        ("n_views", ctypes.c_int32), ("view_tanfovx", ctypes.c_float * 8), ("view_tanfovy", ctypes.c_float * 8),
        ("tile_order_hint", ctypes.c_void_p),
        ("binning", ctypes.c_void_p), ("binning_bytes", ctypes.c_size_t),
        ("shs_rest", c_float_p),
        ("src_depth_slot", ctypes.c_int32 * 5),
    ]


class AdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("bias_correction1", ctypes.c_double), ("bias_correction2", ctypes.c_double)]


class CompactTensor(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("append", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("width", ctypes.c_int32), ("reserved", ctypes.c_int32)]


COMPACT_MAX_TENSORS = 40


class BackwardArgs(ctypes.Structure):
    _fields_ = [
        ("stream", ctypes.c_void_p),
        ("P", ctypes.c_int32), ("D", ctypes.c_int32), ("M", ctypes.c_int32),
        ("W", ctypes.c_int32), ("H", ctypes.c_int32),
        ("R", ctypes.c_int64),
        ("means3D", c_float_p), ("shs", c_float_p), ("colors_precomp", c_float_p),
        ("scales", c_float_p), ("rotations", c_float_p), ("cov3D_precomp", c_float_p), ("all_map", c_float_p),
        ("scale_modifier", ctypes.c_float),
        ("bg", c_float_p), ("viewmatrix", c_float_p), ("projmatrix", c_float_p), ("campos", c_float_p),
        ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float),
        ("n_src", ctypes.c_int32),
        ("ref_to_src", c_float_p), ("src_cam_pos", c_float_p), ("src_images", c_float_p), ("src_depths", c_float_p),
        ("radii", ctypes.c_void_p),
        ("out_depth", c_float_p), ("out_warped", c_float_p),
        ("geom", ctypes.c_void_p), ("binning", ctypes.c_void_p), ("img", ctypes.c_void_p),
        ("tex", ctypes.c_void_p), ("tex_bytes", ctypes.c_size_t),
        ("dL_dcolor", c_float_p), ("dL_dnormal", c_float_p), ("dL_ddepth", c_float_p), ("dL_dwarped", c_float_p),
        ("grad_acc", c_float_p),
        ("dL_dmean2D", c_float_p), ("dL_dmean2D_abs", c_float_p), ("dL_dconic", c_float_p), ("dL_dopacity", c_float_p),
        ("dL_dcolors", c_float_p), ("dL_dmean3D", c_float_p), ("dL_dcov3D", c_float_p), ("dL_dsh", c_float_p),
        ("dL_dscale", c_float_p), ("dL_drot", c_float_p), ("dL_dall_map", c_float_p),
        ("render_geo", ctypes.c_int32), ("flags", ctypes.c_uint32),
        ("plane_normal", c_float_p), ("plane_offset", c_float_p), ("plane_mode", ctypes.c_int32),
        ("dL_dplane_normal", c_float_p), ("dL_dplane_offset", c_float_p),
        ("geo_table", ctypes.c_void_p), ("geo_table_bytes", ctypes.c_size_t),
        ("det_scratch", ctypes.c_void_p), ("det_scratch_bytes", ctypes.c_size_t),
        ("buffer_length", ctypes.c_int32),
        ("tile_order_out", ctypes.c_void_p),
        ("shs_rest", c_float_p), ("dL_dsh_rest", c_float_p),
    ]


# every symbol include/ibgs_rast.h declares
EXPORTS = ["ibgs_required_geom", "ibgs_required_img", "ibgs_required_binning", "ibgs_required_tex",
           "ibgs_forward", "ibgs_backward", "ibgs_mark_visible", "ibgs_tile_order_slots",
           "ibgs_geom_offset", "ibgs_img_offset", "ibgs_binning_offset",
           "ibgs_sizeof_forward_args", "ibgs_sizeof_backward_args", "ibgs_grad_acc_offsets_fit32", "ibgs_clamp_free", "ibgs_clamp_free_threshold", "ibgs_timing_enable", "ibgs_timing_collect",
           "ibgs_required_knn", "ibgs_knn_mean_dist2", "ibgs_sh_grad_from_views", "ibgs_adam_step", "ibgs_adam_step_sh",
           "ibgs_required_compact", "ibgs_compact_plan", "ibgs_compact_apply", "ibgs_densify_stats", "ibgs_required_deterministic", "ibgs_required_geo_table", "ibgs_required_deterministic_for", "ibgs_required_geo_table_for", "ibgs_last_forward_stats", "ibgs_check_async",
           "ibgs_required_l1", "ibgs_l1_loss", "ibgs_l1_grad", "ibgs_l1_rescale",
           "ibgs_depth_normal_forward", "ibgs_depth_normal_backward", "ibgs_activate_forward", "ibgs_activate_backward",
           "ibgs_last_error", "ibgs_version"]

# every symbol include/ibgs_tsdf.h declares (a list of its own: EXPORTS mirrors ibgs_rast.h, tests/test_abi.py compares the two)
TSDF_EXPORTS = ["ibgs_tsdf_sizeof_volume", "ibgs_tsdf_sizeof_view", "ibgs_tsdf_sizeof_mesh_scratch", "ibgs_tsdf_mc_table",
                "ibgs_tsdf_integrate", "ibgs_tsdf_mesh_count", "ibgs_tsdf_mesh_emit"]
TSDF_STATE_WORDS = 8
TSDF_ALLOCATED, TSDF_FAILED, TSDF_IGNORED, TSDF_ACTIVE, TSDF_VERTICES, TSDF_FACES, TSDF_OVERRUN, TSDF_TABLE_FULL = range(8)
TSDF_FLAG_NO_DEDUP = 1


class TsdfVolume(ctypes.Structure):
    _fields_ = [("voxel_length", ctypes.c_float), ("sdf_trunc", ctypes.c_float), ("capacity", ctypes.c_int32), ("slot_bits", ctypes.c_int32),
                ("slot_key", ctypes.c_void_p), ("slot_block", ctypes.c_void_p), ("slot_mark", ctypes.c_void_p), ("active", ctypes.c_void_p),
                ("block_key", ctypes.c_void_p), ("tsdf", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("color", ctypes.c_void_p),
                ("state", ctypes.c_void_p)]


class TsdfView(ctypes.Structure):
    _fields_ = [("W", ctypes.c_int32), ("H", ctypes.c_int32), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("depth_trunc", ctypes.c_float), ("world_to_camera", ctypes.c_float * 12),
                ("camera_to_world", ctypes.c_float * 12)]


class TsdfMeshScratch(ctypes.Structure):
    _fields_ = [("order", ctypes.c_void_p), ("rank", ctypes.c_void_p), ("vinfo", ctypes.c_void_p), ("vcount", ctypes.c_void_p),
                ("fcount", ctypes.c_void_p)]


# every symbol include/ibgs_mesh.h declares (tests/test_mesh_host.py compares the two)
MESH_EXPORTS = ["ibgs_mesh_sizeof_mesh", "ibgs_mesh_required_scratch", "ibgs_mesh_cluster", "ibgs_mesh_filter_count", "ibgs_mesh_filter_emit"]
MESH_STATE_WORDS = 8
MESH_BAD_FACES, MESH_CLUSTERS, MESH_VERTICES_OUT, MESH_FACES_OUT, MESH_TABLE_FULL, MESH_OVERRUN = range(6)
MESH_KEEP_VERTICES, MESH_KEEP_DEGENERATE = 1, 2


class Mesh(ctypes.Structure):
    _fields_ = [("V", ctypes.c_int32), ("F", ctypes.c_int32), ("vertices", ctypes.c_void_p), ("faces", ctypes.c_void_p), ("scratch", ctypes.c_void_p),
                ("scratch_bytes", ctypes.c_size_t), ("state", ctypes.c_void_p)]


# every symbol include/ibgs_mesh_eval.h declares (tests/test_mesh_eval_host.py compares the two)
MESH_EVAL_EXPORTS = ["ibgs_meval_required_sample_scratch", "ibgs_meval_sample_count", "ibgs_meval_sample_emit", "ibgs_meval_keys", "ibgs_meval_required_tree",
                     "ibgs_meval_build", "ibgs_meval_thin_rounds", "ibgs_meval_nearest", "ibgs_meval_reduce"]
MEVAL_STATE_WORDS = 8
MEVAL_BAD_FACES, MEVAL_SAMPLE_OVERFLOW, MEVAL_BAD_POINTS, MEVAL_OVERRUN, MEVAL_UNDECIDED = range(5)
MEVAL_MAX_SIDE = 32768
MEVAL_LEAF = 8
MEVAL_THIN_UNDECIDED, MEVAL_THIN_KEPT, MEVAL_THIN_REMOVED = 0, 1, 2

# every symbol include/ibgs_registration.h declares (tests/test_registration_host.py compares the two)
PCREG_EXPORTS = ["ibgs_pcreg_required_scratch", "ibgs_pcreg_bounds", "ibgs_pcreg_transform", "ibgs_pcreg_crop", "ibgs_pcreg_voxel_keys",
                 "ibgs_pcreg_voxel_count", "ibgs_pcreg_voxel_emit", "ibgs_pcreg_moments"]
PCREG_STATE_WORDS = 8
PCREG_BAD_POINTS, PCREG_KEY_OVERFLOW, PCREG_BAD_INDEX, PCREG_OVERRUN = range(4)
PCREG_MAX_POLYGON = 1024
PCREG_MAX_INDEX = (1 << 21) - 1
PCREG_LONG_SEGMENT = 64
PCREG_MOMENTS = 18

# every symbol include/ibgs_dtu.h declares (tests/test_dtu_host.py compares the two)
DTU_EXPORTS = ["ibgs_dtu_required_dilate_scratch", "ibgs_dtu_dilate", "ibgs_dtu_cull_vertices", "ibgs_dtu_required_cull_scratch", "ibgs_dtu_cull_count",
               "ibgs_dtu_cull_emit", "ibgs_dtu_obs_filter", "ibgs_dtu_above_plane"]
DTU_STATE_WORDS = 8
DTU_BAD_FACES, DTU_BAD_POINTS, DTU_OVERRUN, DTU_VERTICES_OUT, DTU_FACES_OUT = range(5)
DTU_MAX_RADIUS = 255
DTU_MAX_SIDE = 65536

# every symbol include/ibgs_ssim.h declares (tests/test_ssim_host.py compares the two)
SSIM_EXPORTS = ["ibgs_ssim_required_scratch", "ibgs_ssim_tile", "ibgs_ssim_forward", "ibgs_ssim_backward"]
SSIM_WINDOW = 11
SSIM_MAX_SIDE = 65536

# every symbol include/ibgs_geo_loss.h declares (tests/test_geoloss_host.py compares the two)
GEOLOSS_EXPORTS = ["ibgs_geoloss_required_scratch", "ibgs_geoloss_tile", "ibgs_geoloss_photo_forward", "ibgs_geoloss_photo_backward",
                   "ibgs_geoloss_normal_forward", "ibgs_geoloss_rescale"]
GEOLOSS_MAX_SRC = 5
GEOLOSS_MAX_SIDE = 65536

# every symbol include/ibgs_color_agg.h declares (tests/test_coloragg_host.py compares the two)
CAGG_EXPORTS = ["ibgs_cagg_required_scratch", "ibgs_cagg_levels", "ibgs_cagg_forward", "ibgs_cagg_backward"]
CAGG_MAX_SRC = 5
CAGG_MAX_SIDE = 65536
CAGG_FEATURES = 32
CAGG_MEAN, CAGG_MAX = 0, 1

# every symbol include/ibgs_hourglass.h declares (tests/test_hourglass_host.py compares the two)
HG_EXPORTS = ["ibgs_hg_required_scratch", "ibgs_hg_forward"]
HG_CHANNELS = 38
HG_MIN_SIDE = 4
HG_MAX_SIDE = 8192

# every symbol include/ibgs_hg_train.h declares (tests/test_hourglass_train_host.py compares the two)
HGB_EXPORTS = ["ibgs_hgb_required_scratch", "ibgs_hgb_backward"]

# every symbol include/ibgs_hg_half.h declares (tests/test_hghalf_host.py compares the two)
HGH_EXPORTS = ["ibgs_hgh_required_scratch", "ibgs_hgh_forward"]
HGH_PACKED_WEIGHT_BYTES = 281600

# every symbol include/ibgs_hg_half_train.h declares (tests/test_hghtrain_host.py compares the two), and its constants
HGHT_EXPORTS = ["ibgs_hgh_train_required_scratch", "ibgs_hgh_train_backward"]
HGHT_E_TARGET = 10
HGHT_SCALE_AUTO, HGHT_SCALE_FIXED = 0, 1
HGHT_PACKED_WEIGHT_BYTES = 405504

# every symbol include/ibgs_lpips.h declares (tests/test_lpips_host.py compares the two)
LPIPS_EXPORTS = ["ibgs_lpips_required_scratch", "ibgs_lpips_conv3", "ibgs_lpips_forward"]
LPIPS_MIN_SIDE = 16
LPIPS_MAX_SIDE = 4096
LPIPS_CONVS = 13
LPIPS_TAPS = 5
# channels in and out of the thirteen convolutions, the resolution level (number of pools in front) of each one's output, and the convolution whose ReLU is tap k
LPIPS_CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_LEVEL = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
LPIPS_TAP_CONV = (1, 3, 6, 9, 12)

# every symbol include/ibgs_exposure.h declares (tests/test_exposure_host.py compares the two)
EXPO_EXPORTS = ["ibgs_expo_required_scratch", "ibgs_expo_fit", "ibgs_expo_apply", "ibgs_expo_apply_backward"]
EXPO_MAX_SIDE = 65536
EXPO_SUMS = 22
EXPO_THREADS = 256
EXPO_MAX_GROUPS = 256
EXPO_PIXELS_PER_THREAD = 4
EXPO_MOMENTS, EXPO_SOLVE, EXPO_FIT = 1, 2, 3
EXPO_PIVOT_MIN = 1e-11

# every symbol include/ibgs_export.h declares (tests/test_frame_export_host.py compares the two)
FEXP_EXPORTS = ["ibgs_fexp_sizeof_frame", "ibgs_required_export", "ibgs_fexp_frame_u8", "ibgs_fexp_percentile", "ibgs_fexp_quantize"]
FEXP_MAX_SIDE = 65536
FEXP_MAX_PIXELS = 1 << 30
FEXP_MAX_SELECT = 1 << 24
FEXP_MAX_IMAGES = 8
FEXP_MAX_Q = 4
FEXP_ROUND, FEXP_TRUNCATE, FEXP_NORMAL, FEXP_RESIDUAL, FEXP_COLORIZE = range(5)
FEXP_ZERO_RESIDUAL, FEXP_NO_VALID = 1, 2


class FexpImage(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("mode", ctypes.c_int32), ("channels", ctypes.c_int32), ("bgr", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class FexpFrame(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("n_images", ctypes.c_int32), ("reserved", ctypes.c_int32), ("images", FexpImage * 8),
                ("lut", ctypes.c_void_p), ("invalid_mask", ctypes.c_void_p), ("use_invalid_val", ctypes.c_int32), ("invalid_val", ctypes.c_float),
                ("have_vmin", ctypes.c_int32), ("have_vmax", ctypes.c_int32), ("vmin", ctypes.c_float), ("vmax", ctypes.c_float), ("q32", ctypes.c_float * 2),
                ("background", ctypes.c_uint8 * 4), ("status", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_size_t)]


# every symbol include/ibgs_resample.h declares (tests/test_resample_host.py compares the two)
RSZ_EXPORTS = ["ibgs_rsz_features_forward", "ibgs_rsz_residual_upsample"]
RSZ_MAX_SRC = 5
RSZ_MAX_SIDE = 65536
RSZ_FEATURES = 32
RSZ_MEAN, RSZ_MAX = 0, 1

# every symbol include/ibgs_resample_train.h declares (tests/test_resample_train_host.py compares the two); its limits and modes are ibgs_resample.h's
RZT_EXPORTS = ["ibgs_rzt_required_scratch", "ibgs_rzt_features_backward", "ibgs_rzt_upsample_backward"]


_lib = None


class RasterizerLibraryError(RuntimeError):
    pass


def load():
    """Load libibgs_rast.so (after torch, so that the HIP runtime torch ships is the one in use)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RasterizerLibraryError(
            "libibgs_rast.so is not built (%s). Run `python -m ibgs_amd._build` or __graft_entry__.build(); "
            "there is no fallback path." % LIB_PATH)
    import torch  # noqa: F401  (loads libamdhip64 first; both sides then share one HIP runtime)
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_required_geom.restype = ctypes.c_size_t
    lib.ibgs_required_geom.argtypes = [ctypes.c_int32]
    lib.ibgs_required_img.restype = ctypes.c_size_t
    lib.ibgs_required_img.argtypes = [ctypes.c_int32, ctypes.c_int32]
    lib.ibgs_required_binning.restype = ctypes.c_size_t
    lib.ibgs_required_binning.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    lib.ibgs_required_tex.restype = ctypes.c_size_t
    lib.ibgs_required_tex.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    lib.ibgs_forward.restype = ctypes.c_int64
    lib.ibgs_forward.argtypes = [ctypes.POINTER(ForwardArgs)]
    lib.ibgs_backward.restype = ctypes.c_int32
    lib.ibgs_backward.argtypes = [ctypes.POINTER(BackwardArgs)]
    lib.ibgs_mark_visible.restype = ctypes.c_int32
    lib.ibgs_mark_visible.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    for f in (lib.ibgs_geom_offset,):
        f.restype = ctypes.c_int64
        f.argtypes = [ctypes.c_int32, ctypes.c_char_p]
    lib.ibgs_img_offset.restype = ctypes.c_int64
    lib.ibgs_img_offset.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p]
    lib.ibgs_binning_offset.restype = ctypes.c_int64
    lib.ibgs_binning_offset.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p]
    lib.ibgs_last_error.restype = ctypes.c_char_p
    lib.ibgs_version.restype = ctypes.c_char_p
    lib.ibgs_timing_enable.restype = None
    lib.ibgs_timing_enable.argtypes = [ctypes.c_uint32]
    lib.ibgs_timing_collect.restype = ctypes.c_int32
    lib.ibgs_timing_collect.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.ibgs_required_knn.restype = ctypes.c_size_t
    lib.ibgs_required_knn.argtypes = [ctypes.c_int32]
    lib.ibgs_sh_grad_from_views.restype = ctypes.c_int32
    lib.ibgs_sh_grad_from_views.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p]
    lib.ibgs_adam_step.restype = ctypes.c_int32
    lib.ibgs_adam_step.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.ibgs_adam_step_sh.restype = ctypes.c_int32
    lib.ibgs_adam_step_sh.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ibgs_tile_order_slots.restype = ctypes.c_size_t
    lib.ibgs_tile_order_slots.argtypes = [ctypes.c_int32, ctypes.c_int32]
    lib.ibgs_required_l1.restype = ctypes.c_size_t
    lib.ibgs_required_l1.argtypes = []
    lib.ibgs_l1_loss.restype = ctypes.c_int32
    lib.ibgs_l1_loss.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    lib.ibgs_l1_grad.restype = ctypes.c_int32
    lib.ibgs_l1_grad.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
    lib.ibgs_densify_stats.restype = ctypes.c_int32
    lib.ibgs_densify_stats.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 8
    lib.ibgs_depth_normal_forward.restype = ctypes.c_int32
    lib.ibgs_depth_normal_forward.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_float] * 4 + [ctypes.c_void_p] * 2
    lib.ibgs_depth_normal_backward.restype = ctypes.c_int32
    lib.ibgs_depth_normal_backward.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_float] * 4 + [ctypes.c_void_p] * 3
    lib.ibgs_activate_forward.restype = ctypes.c_int32
    lib.ibgs_activate_forward.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 6
    lib.ibgs_activate_backward.restype = ctypes.c_int32
    lib.ibgs_activate_backward.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 9
    lib.ibgs_l1_rescale.restype = ctypes.c_int32
    lib.ibgs_l1_rescale.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.ibgs_required_geo_table.restype = ctypes.c_size_t
    lib.ibgs_required_geo_table.argtypes = [ctypes.c_int32, ctypes.c_int32]
    lib.ibgs_last_forward_stats.restype = None
    lib.ibgs_last_forward_stats.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.ibgs_check_async.restype = ctypes.c_int32
    lib.ibgs_check_async.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.ibgs_required_geo_table_for.restype = ctypes.c_size_t
    lib.ibgs_required_geo_table_for.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    lib.ibgs_required_deterministic_for.restype = ctypes.c_size_t
    lib.ibgs_required_deterministic_for.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32]
    lib.ibgs_required_deterministic.restype = ctypes.c_size_t
    lib.ibgs_required_deterministic.argtypes = [ctypes.c_int64, ctypes.c_int32]
    lib.ibgs_required_compact.restype = ctypes.c_size_t
    lib.ibgs_required_compact.argtypes = [ctypes.c_int32]
    lib.ibgs_compact_plan.restype = ctypes.c_int64
    lib.ibgs_compact_plan.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.ibgs_compact_apply.restype = ctypes.c_int32
    lib.ibgs_compact_apply.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    lib.ibgs_knn_mean_dist2.restype = ctypes.c_int32
    lib.ibgs_knn_mean_dist2.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    for name in TSDF_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    for f in (lib.ibgs_tsdf_sizeof_volume, lib.ibgs_tsdf_sizeof_view, lib.ibgs_tsdf_sizeof_mesh_scratch):
        f.restype = ctypes.c_size_t
        f.argtypes = []
    lib.ibgs_tsdf_mc_table.restype = ctypes.c_int32
    lib.ibgs_tsdf_mc_table.argtypes = [ctypes.c_void_p]
    lib.ibgs_tsdf_integrate.restype = ctypes.c_int32
    lib.ibgs_tsdf_integrate.argtypes = [ctypes.c_void_p, ctypes.POINTER(TsdfVolume), ctypes.POINTER(TsdfView), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    lib.ibgs_tsdf_mesh_count.restype = ctypes.c_int32
    lib.ibgs_tsdf_mesh_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(TsdfVolume), ctypes.POINTER(TsdfMeshScratch)]
    lib.ibgs_tsdf_mesh_emit.restype = ctypes.c_int32
    lib.ibgs_tsdf_mesh_emit.argtypes = [ctypes.c_void_p, ctypes.POINTER(TsdfVolume), ctypes.POINTER(TsdfMeshScratch), ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 4
    if (lib.ibgs_tsdf_sizeof_volume() != ctypes.sizeof(TsdfVolume) or lib.ibgs_tsdf_sizeof_view() != ctypes.sizeof(TsdfView)
            or lib.ibgs_tsdf_sizeof_mesh_scratch() != ctypes.sizeof(TsdfMeshScratch)):
        raise RasterizerLibraryError("ctypes TSDF struct layout does not match libibgs_rast.so (stale build?)")
    for name in MESH_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_mesh_sizeof_mesh.restype = ctypes.c_size_t
    lib.ibgs_mesh_sizeof_mesh.argtypes = []
    lib.ibgs_mesh_required_scratch.restype = ctypes.c_size_t
    lib.ibgs_mesh_required_scratch.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.ibgs_mesh_cluster.restype = ctypes.c_int32
    lib.ibgs_mesh_cluster.argtypes = [ctypes.c_void_p, ctypes.POINTER(Mesh)] + [ctypes.c_void_p] * 3
    lib.ibgs_mesh_filter_count.restype = ctypes.c_int32
    lib.ibgs_mesh_filter_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(Mesh), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32]
    lib.ibgs_mesh_filter_emit.restype = ctypes.c_int32
    lib.ibgs_mesh_filter_emit.argtypes = [ctypes.c_void_p, ctypes.POINTER(Mesh), ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]
    if lib.ibgs_mesh_sizeof_mesh() != ctypes.sizeof(Mesh):
        raise RasterizerLibraryError("ctypes mesh struct layout does not match libibgs_rast.so (stale build?)")
    for name in MESH_EVAL_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    vp, i32, i64, f32, f64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    for f in (lib.ibgs_meval_required_sample_scratch, lib.ibgs_meval_required_tree):
        f.restype = sz
        f.argtypes = [i64]
    for f, args in ((lib.ibgs_meval_sample_count, [vp, i32, i32, vp, vp, f64, vp, sz, vp, vp]),
                    (lib.ibgs_meval_sample_emit, [vp, i32, i32, vp, vp, f64, vp, sz, i64, vp, vp]),
                    (lib.ibgs_meval_keys, [vp, i32, vp, vp, vp, vp]),
                    (lib.ibgs_meval_build, [vp, i32, vp, vp, vp, vp, sz, vp]),
                    (lib.ibgs_meval_thin_rounds, [vp, i32, vp, sz, f32, vp, i32, vp]),
                    (lib.ibgs_meval_nearest, [vp, i32, vp, vp, i32, vp, sz, f32, vp, vp, vp]),
                    (lib.ibgs_meval_reduce, [vp, i32, vp, f32, vp, vp])):
        f.restype = i32
        f.argtypes = args
    for name in PCREG_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_pcreg_required_scratch.restype = sz
    lib.ibgs_pcreg_required_scratch.argtypes = [i64]
    for f, args in ((lib.ibgs_pcreg_bounds, [vp, i32, vp, vp, sz, vp, vp]),
                    (lib.ibgs_pcreg_transform, [vp, i32, vp, vp, vp, vp]),
                    (lib.ibgs_pcreg_crop, [vp, i32, vp, vp, i32, f64, f64, i32, vp, vp, vp]),
                    (lib.ibgs_pcreg_voxel_keys, [vp, i32, vp, vp, f64, vp, vp]),
                    (lib.ibgs_pcreg_voxel_count, [vp, i32, vp, vp, sz, vp, vp]),
                    (lib.ibgs_pcreg_voxel_emit, [vp, i32, vp, vp, vp, vp, sz, i32, vp, vp, vp]),
                    (lib.ibgs_pcreg_moments, [vp, i32, vp, vp, i32, vp, vp, vp, sz, vp, vp])):
        f.restype = i32
        f.argtypes = args
    for name in DTU_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_dtu_required_dilate_scratch.restype = sz
    lib.ibgs_dtu_required_dilate_scratch.argtypes = [i64, i64, i64]
    lib.ibgs_dtu_required_cull_scratch.restype = sz
    lib.ibgs_dtu_required_cull_scratch.argtypes = [i64, i64]
    for f, args in ((lib.ibgs_dtu_dilate, [vp, i32, i32, i32, i32, vp, vp, sz, vp]),
                    (lib.ibgs_dtu_cull_vertices, [vp, i32, vp, i32, vp, i32, i32, vp, vp, vp]),
                    (lib.ibgs_dtu_cull_count, [vp, i32, i32, vp, vp, vp, sz, vp]),
                    (lib.ibgs_dtu_cull_emit, [vp, i32, i32, vp, vp, vp, vp, vp, sz, f32, vp, i32, i32, vp, vp, vp, vp, vp]),
                    (lib.ibgs_dtu_obs_filter, [vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, f64, vp, vp, vp]),
                    (lib.ibgs_dtu_above_plane, [vp, i32, vp, vp, vp, vp])):
        f.restype = i32
        f.argtypes = args
    for name in SSIM_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_ssim_required_scratch.restype = sz
    lib.ibgs_ssim_required_scratch.argtypes = [i64, i64, i64]
    lib.ibgs_ssim_tile.restype = None
    lib.ibgs_ssim_tile.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.ibgs_ssim_forward.restype = i32
    lib.ibgs_ssim_forward.argtypes = [vp, i32, i32, i32, i32] + [vp] * 10 + [sz]
    lib.ibgs_ssim_backward.restype = i32
    lib.ibgs_ssim_backward.argtypes = [vp, i32, i32, i32, i32] + [vp] * 6
    for name in GEOLOSS_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_geoloss_required_scratch.restype = sz
    lib.ibgs_geoloss_required_scratch.argtypes = [i64, i64, i64]
    lib.ibgs_geoloss_tile.restype = None
    lib.ibgs_geoloss_tile.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.ibgs_geoloss_photo_forward.restype = i32
    lib.ibgs_geoloss_photo_forward.argtypes = [vp, i32, i32, i32, vp, vp, vp, f64, f64, vp, vp, vp, vp, sz]
    lib.ibgs_geoloss_photo_backward.restype = i32
    lib.ibgs_geoloss_photo_backward.argtypes = [vp, i32, i32, i32, i32] + [vp] * 6 + [f64, f64, vp]
    lib.ibgs_geoloss_normal_forward.restype = i32
    lib.ibgs_geoloss_normal_forward.argtypes = [vp, i32, i32, vp, vp, f64, vp, vp, vp, vp, sz]
    lib.ibgs_geoloss_rescale.restype = i32
    lib.ibgs_geoloss_rescale.argtypes = [vp, i64, vp, vp]
    for name in CAGG_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_cagg_required_scratch.restype = sz
    lib.ibgs_cagg_required_scratch.argtypes = [i64, i64, i64]
    lib.ibgs_cagg_levels.restype = i32
    lib.ibgs_cagg_levels.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, sz]
    lib.ibgs_cagg_forward.restype = i32
    lib.ibgs_cagg_forward.argtypes = [vp, i32, i32, i32, i32] + [vp] * 10
    lib.ibgs_cagg_backward.restype = i32
    lib.ibgs_cagg_backward.argtypes = [vp, i32, i32, i32, i32] + [vp] * 16 + [sz]
    for name in HG_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_hg_required_scratch.restype = sz
    lib.ibgs_hg_required_scratch.argtypes = [i64, i64]
    lib.ibgs_hg_forward.restype = i32
    lib.ibgs_hg_forward.argtypes = [vp, i32, i32, vp] + [vp] * 18 + [f32, vp, vp, vp, sz]
    for name in HGB_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_hgb_required_scratch.restype = sz
    lib.ibgs_hgb_required_scratch.argtypes = [i64, i64]
    lib.ibgs_hgb_backward.restype = i32
    # (stream, H, W, x, 18 parameters, burned, stages arena, grad_residual, grad_image_pred, grad_x, 18 gradients, scratch, bytes)
    lib.ibgs_hgb_backward.argtypes = [vp, i32, i32, vp] + [vp] * 18 + [f32, vp, vp, vp, vp] + [vp] * 18 + [vp, sz]
    for name in HGH_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_hgh_required_scratch.restype = sz
    lib.ibgs_hgh_required_scratch.argtypes = [i64, i64]
    lib.ibgs_hgh_forward.restype = i32
    lib.ibgs_hgh_forward.argtypes = [vp, i32, i32, vp] + [vp] * 18 + [f32, vp, vp, vp, sz]
    for name in HGHT_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_hgh_train_required_scratch.restype = sz
    lib.ibgs_hgh_train_required_scratch.argtypes = [i64, i64]
    lib.ibgs_hgh_train_backward.restype = i32
    # (stream, H, W, x, 18 parameters, burned, forward arena, grad_residual, grad_image_pred, scale mode, grad_scale_log2, status, grad_x, 18 gradients, scratch, bytes)
    lib.ibgs_hgh_train_backward.argtypes = [vp, i32, i32, vp] + [vp] * 18 + [f32, vp, vp, vp, i32, i32, vp, vp] + [vp] * 18 + [vp, sz]
    for name in LPIPS_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_lpips_required_scratch.restype = sz
    lib.ibgs_lpips_required_scratch.argtypes = [i64, i64]
    lib.ibgs_lpips_conv3.restype = i32
    # (stream, hs, ws, cin, cout, pool, zscore, in_x, in_y, weight, bias, out)
    lib.ibgs_lpips_conv3.argtypes = [vp] + [i32] * 6 + [vp] * 5
    lib.ibgs_lpips_forward.restype = i32
    # (stream, H, W, x, y, conv_w[13], conv_b[13], lin_w[5], lpips, tap_values, maps[5], scratch, bytes): the three tables and maps are host arrays of pointers
    lib.ibgs_lpips_forward.argtypes = [vp, i32, i32, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, ctypes.POINTER(vp), vp, sz]
    for name in EXPO_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_expo_required_scratch.restype = sz
    lib.ibgs_expo_required_scratch.argtypes = [i64, i64]
    lib.ibgs_expo_fit.restype = i32
    # (stream, H, W, render, warped, mask, affine_out, status_out, scratch, bytes, phases)
    lib.ibgs_expo_fit.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, sz, i32]
    for f in (lib.ibgs_expo_apply, lib.ibgs_expo_apply_backward):          # (stream, H, W, affine, status, image, out)
        f.restype = i32
        f.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    for name in FEXP_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_fexp_sizeof_frame.restype = sz
    lib.ibgs_fexp_sizeof_frame.argtypes = []
    lib.ibgs_required_export.restype = sz
    lib.ibgs_required_export.argtypes = [i64, i64]
    lib.ibgs_fexp_frame_u8.restype = i32
    lib.ibgs_fexp_frame_u8.argtypes = [vp, ctypes.POINTER(FexpFrame)]
    lib.ibgs_fexp_percentile.restype = i32
    # (stream, n, values, invalid_mask, use_invalid_val, invalid_val, nq, q32 (host), out, status, scratch, bytes)
    lib.ibgs_fexp_percentile.argtypes = [vp, i64, vp, vp, i32, f32, i32, ctypes.POINTER(f32), vp, vp, vp, sz]
    lib.ibgs_fexp_quantize.restype = i32
    lib.ibgs_fexp_quantize.argtypes = [vp, i64, vp, vp]
    if lib.ibgs_fexp_sizeof_frame() != ctypes.sizeof(FexpFrame):
        raise RasterizerLibraryError("ctypes frame-export struct layout does not match libibgs_rast.so (stale build?)")
    for name in RSZ_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_rsz_features_forward.restype = i32
    # (stream, S, H, W, Hr, Wr, mode, render, warped, cam_feat, camera_ray, w1, b1, w2, b2, levels, out)
    lib.ibgs_rsz_features_forward.argtypes = [vp, i32, i32, i32, i32, i32, i32] + [vp] * 10
    lib.ibgs_rsz_residual_upsample.restype = i32
    # (stream, H, W, Hr, Wr, residual_r, render, render_scale, residual_out, image_pred_out)
    lib.ibgs_rsz_residual_upsample.argtypes = [vp, i32, i32, i32, i32, vp, vp, f32, vp, vp]
    for name in RZT_EXPORTS:
        if not hasattr(lib, name):
            raise RasterizerLibraryError("libibgs_rast.so lacks symbol %s" % name)
    lib.ibgs_rzt_required_scratch.restype = sz
    lib.ibgs_rzt_required_scratch.argtypes = [i64] * 5
    lib.ibgs_rzt_features_backward.restype = i32
    # (stream, S, H, W, Hr, Wr, mode, render, warped, cam_feat, w1, b1, w2, b2, levels, grad_out, 6 gradients, scratch, bytes)
    lib.ibgs_rzt_features_backward.argtypes = [vp, i32, i32, i32, i32, i32, i32] + [vp] * 16 + [sz]
    lib.ibgs_rzt_upsample_backward.restype = i32
    # (stream, H, W, Hr, Wr, grad_residual_out, grad_image_pred, grad_residual_r)
    lib.ibgs_rzt_upsample_backward.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    lib.ibgs_grad_acc_offsets_fit32.restype = ctypes.c_int32
    lib.ibgs_grad_acc_offsets_fit32.argtypes = [ctypes.c_int64]
    lib.ibgs_clamp_free.restype = ctypes.c_int32
    lib.ibgs_clamp_free.argtypes = [ctypes.c_float]
    lib.ibgs_clamp_free_threshold.restype = ctypes.c_float
    lib.ibgs_clamp_free_threshold.argtypes = []
    lib.ibgs_sizeof_forward_args.restype = ctypes.c_size_t
    lib.ibgs_sizeof_backward_args.restype = ctypes.c_size_t
    if (lib.ibgs_sizeof_forward_args() != ctypes.sizeof(ForwardArgs)
            or lib.ibgs_sizeof_backward_args() != ctypes.sizeof(BackwardArgs)):
        raise RasterizerLibraryError("ctypes struct layout does not match libibgs_rast.so (stale build?)")
    _lib = lib
    return lib


# "binning" = coarse entries placed per cell + per-tile counts + ranges, "list_scatter" = the ids to their slots (two-level binning,
# csrc/binning.hip); "ranges" has no kernel of its own any more (always 0)
STAGES = ["preprocess", "depth_sort", "scan", "binning", "list_scatter", "ranges", "render_fwd", "render_bwd",
          "preprocess_bwd", "geo_window", "tile_order"]


def timing_enable(stages):
    """Bracket the named stages with hipEvents on the op's stream (bench.py roofline)."""
    mask = 0
    for s in stages:
        mask |= 1 << STAGES.index(s)
    load().ibgs_timing_enable(mask)


def timing_collect():
    """-> {stage: (total_ms, launches)} since the previous collect."""
    ms = (ctypes.c_float * len(STAGES))()
    n = (ctypes.c_int32 * len(STAGES))()
    rc = load().ibgs_timing_collect(ms, n)
    if rc < 0:
        raise RuntimeError("ibgs_timing_collect failed: %s" % last_error())
    return {STAGES[i]: (float(ms[i]), int(n[i])) for i in range(len(STAGES))}


def last_error():
    return load().ibgs_last_error().decode("utf-8", "replace")


def last_forward_stats():
    """(R, coarse binning entries or -1, hint missed?) of this thread's last ibgs_forward."""
    out = (ctypes.c_int64 * 3)()
    load().ibgs_last_forward_stats(out)
    return int(out[0]), int(out[1]), bool(out[2])
