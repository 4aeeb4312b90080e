/*
 * ibgs_registration.h -- C ABI of the point-cloud registration in libibgs_rast.so (ibgs_amd/csrc/registration.hip): rigid / affine transform of a cloud,
 * crop to a polygon selection volume, voxel-grid thinning, and the moment sums of a point-to-point similarity fit (one ICP step).
 *
 * Replaces the Open3D stages of the reference's scripts/tnt_eval (registration.py:106-195, evaluation.py:74-91): PointCloud.transform,
 * SelectionPolygonVolume.crop_point_cloud, voxel_down_sample, and the inner sums of registration_icp with TransformationEstimationPointToPoint(True).  The
 * correspondence search of ICP is ibgs_meval_nearest (ibgs_mesh_eval.h).  The contract is this project's own statement of those stages: DESIGN.md section 11
 * ("Registration") and the header of registration.hip; tests/registration_ref.py restates it.
 *
 * Conventions are those of ibgs_mesh_eval.h: device pointers unless the name starts with "host_", `stream` is a hipStream_t passed as void*, return value
 * >= 0 on success, < 0 = -(IBGS_ERR_*) with ibgs_last_error() holding the message.  The caller owns every array (ibgs_amd/registration.py allocates them
 * with torch, and orders the voxel keys with torch.sort); the library keeps no state and never waits for the device.
 *
 * Limits: 0 <= N, Q < 2^31; 3 <= polygon vertices <= IBGS_PCREG_MAX_POLYGON.
 */
#ifndef IBGS_REGISTRATION_H
#define IBGS_REGISTRATION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* words of `state` (uint32, device; zeroed by the caller; all sticky: a non-zero word means the caller must fail the call) */
#define IBGS_PCREG_BAD_POINTS 0           /* points with a non-finite coordinate (before or after the transform) */
#define IBGS_PCREG_KEY_OVERFLOW 1         /* points whose voxel index along an axis exceeds IBGS_PCREG_MAX_INDEX: the voxel size is too small */
#define IBGS_PCREG_BAD_INDEX 2            /* correspondences >= N or entries of `order` outside [0, N): never dereferenced */
#define IBGS_PCREG_OVERRUN 3              /* voxels that fell outside the output (0 unless M passed to voxel_emit is not voxel_count's total) */
#define IBGS_PCREG_STATE_WORDS 8

#define IBGS_PCREG_MAX_POLYGON 1024       /* vertices of a crop polygon */
#define IBGS_PCREG_MAX_INDEX 2097151      /* largest voxel index along an axis (21 bits) */
#define IBGS_PCREG_LONG_SEGMENT 64        /* voxels of more points than this are summed by a whole wave */
#define IBGS_PCREG_MOMENTS 18             /* doubles of a moment block: n, S_s[3], S_t[3], S_st[9] (row = s, column = t), S_ss, S_dd */

/* One scratch serves every call below on clouds of up to N points (128-byte aligned); 0 when N is out of range. */
size_t ibgs_pcreg_required_scratch(int64_t N);

/* bounds[0..2] = the per-axis minimum, bounds[3..5] = the maximum of the N > 0 points (6 floats, device). */
int32_t ibgs_pcreg_bounds(void* stream, int32_t N, const float* points, void* scratch, size_t scratch_bytes, float* bounds, uint32_t* state);

/* out = T points: host_T is a row-major 4 x 4 whose last row is 0 0 0 1, passed to the kernel by value.  x' = ((T00 x + T01 y) + T02 z) + T03 in f64 from
 * the f32 coordinates, rounded once to f32.  out may be `points`. */
int32_t ibgs_pcreg_transform(void* stream, int32_t N, const float* points, const double* host_T, float* out, uint32_t* state);

/* mask[i] = 1 iff point i (after host_T, when that is not null: exactly ibgs_pcreg_transform's result) lies in the volume: axis_min <= p[w] <= axis_max
 * and an odd number of polygon edges cross to the left of it.  axis = w = 0, 1, 2 (u, v = the other two axes, ascending); polygon = n_poly x {u, v} doubles
 * on the device. */
int32_t ibgs_pcreg_crop(void* stream, int32_t N, const float* points, const double* host_T, int32_t axis, double axis_min, double axis_max, int32_t n_poly,
                        const double* polygon, uint8_t* mask, uint32_t* state);

/* keys[i] = ix << 42 | iy << 21 | iz with i = floor((p - (lo - voxel / 2)) / voxel) in f64; lo = bounds[0..2] (device, ibgs_pcreg_bounds of the same cloud). */
int32_t ibgs_pcreg_voxel_keys(void* stream, int32_t N, const float* points, const float* bounds, double voxel, int64_t* keys, uint32_t* state);

/* sorted_keys (N, ascending): marks the first point of every voxel and scans the marks (both left in the scratch); total[0] = the number of voxels. */
int32_t ibgs_pcreg_voxel_count(void* stream, int32_t N, const int64_t* sorted_keys, void* scratch, size_t scratch_bytes, uint32_t* total, uint32_t* state);

/* out (M x 3 floats, M = voxel_count's total): per voxel, in ascending key order, the f64 sum of points[order[k]] over its members divided by their number,
 * rounded once to f32.  order (N int64): the points' indices in ascending key order, equal keys in index order.  out_keys (M int64, or null): the voxel's key. */
int32_t ibgs_pcreg_voxel_emit(void* stream, int32_t N, const float* points, const int64_t* order, const int64_t* sorted_keys, const void* scratch,
                              size_t scratch_bytes, int32_t M, float* out, int64_t* out_keys, uint32_t* state);

/* out[0 .. 18): over the queries i with 0 <= index[i] < N, s = query[i], t = target[index[i]], about the pivot c = host_pivot[0..2]:
 * n, sum(s - c), sum(t - c), sum (s - c)(t - c)^T, sum |s - c|^2, sum d^2 with d^2 = (dx dx + dy dy) + dz dz of the widened differences.  f64, summed in a
 * fixed order without atomics: the same bits on every run. */
int32_t ibgs_pcreg_moments(void* stream, int32_t Q, const float* query, const int32_t* index, int32_t N, const float* target, const double* host_pivot,
                           void* scratch, size_t scratch_bytes, double* out, uint32_t* state);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_REGISTRATION_H */
