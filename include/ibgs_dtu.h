/*
 * ibgs_dtu.h -- C ABI of the DTU evaluation front end in libibgs_rast.so (ibgs_amd/csrc/dtu.hip): dilation of the object masks, culling of a mesh's vertices
 * against the dilated masks of every view, compaction of the culled mesh, and the observation-mask / ground-plane filters of the point clouds.
 *
 * Replaces the host stages of the reference's scripts/eval_dtu (evaluate_single_scene.py:53-95: cv2 / skimage dilation, torch CPU grid_sample, trimesh
 * update_vertices / update_faces; eval.py:98-110 and 126-130: numpy).  The contract is this project's own statement of those stages: DESIGN.md section 11
 * ("DTU evaluation") and the header of dtu.hip; tests/dtu_ref.py restates it.
 *
 * Conventions are those of ibgs_mesh_eval.h: device pointers unless the name starts with "host_", `stream` is a hipStream_t passed as void*, return value
 * >= 0 on success, < 0 = -(IBGS_ERR_*) with ibgs_last_error() holding the message.  The caller owns every array (ibgs_amd/dtu.py allocates them with torch);
 * the library keeps no state, never waits for the device and never writes an input.
 *
 * Mask bits: a view's dilated mask is H rows of ceil(W / 64) 64-bit words; bit (x & 63) of word (x >> 6) is pixel x of the row, bits at x >= W are zero.
 *
 * Limits: n, V, N >= 0 (int32: every index is formed in size_t, so nothing beyond the type bounds them); 0 <= F < 2^30; 2 <= H, W <= IBGS_DTU_MAX_SIDE;
 * 0 <= radius <= IBGS_DTU_MAX_RADIUS; n H ceil(W / 64) < 2^32.
 */
#ifndef IBGS_DTU_H
#define IBGS_DTU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* words of `state` (uint32, device; zeroed by the caller).  The first three are sticky: a non-zero word means the caller must fail the call. */
#define IBGS_DTU_BAD_FACES 0              /* faces with a vertex index outside [0, V): never dereferenced */
#define IBGS_DTU_BAD_POINTS 1             /* points with a non-finite coordinate (obs_filter, above_plane) */
#define IBGS_DTU_OVERRUN 2                /* a pixel or an output row outside its array: a library fault, never dereferenced */
#define IBGS_DTU_VERTICES_OUT 3           /* cull_count: vertices kept */
#define IBGS_DTU_FACES_OUT 4              /* cull_count: faces kept */
#define IBGS_DTU_STATE_WORDS 8

#define IBGS_DTU_MAX_RADIUS 255
#define IBGS_DTU_MAX_SIDE 65536

/* bytes of the scratch of ibgs_dtu_dilate (the undilated bits: n x H x ceil(W / 64) words, 128-byte aligned); 0 when an argument is out of range */
size_t ibgs_dtu_required_dilate_scratch(int64_t n, int64_t H, int64_t W);

/* masks: n x H x W bytes, non-zero = set.  out (n x H x ceil(W / 64) words): out[y, x] = OR of in[y + dy, x + dx] over dx dx + dy dy <= radius radius inside
 * the image (binary dilation by a disc, zero outside the image). */
int32_t ibgs_dtu_dilate(void* stream, int32_t n, int32_t H, int32_t W, int32_t radius, const uint8_t* masks, void* scratch, size_t scratch_bytes,
                        uint64_t* out);

/* keep[v] = 1 iff every view i either does not see vertex v or sees it on a set bit of view i's mask.  projections: n x 3 x 4 floats (rows 0..2 of
 * K world_to_camera).  All in f32, one rounding per operation, nothing contracted:
 *   c_r = ((P_r0 x + P_r1 y) + P_r2 z) + P_r3;  u = c_0 / (c_2 + 1e-6f), v = c_1 / (c_2 + 1e-6f);  gx = (u / (W - 1) - 0.5f) * 2, gy = (v / (H - 1) - 0.5f) * 2;
 *   seen iff -1 < gx < 1 and -1 < gy < 1;  ix = rint(((gx + 1) / 2) * (W - 1)), iy = rint(((gy + 1) / 2) * (H - 1)) (ties to even). */
int32_t ibgs_dtu_cull_vertices(void* stream, int32_t V, const float* vertices, int32_t n, const float* projections, int32_t H, int32_t W, const uint64_t* bits,
                               uint8_t* keep, uint32_t* state);

/* One scratch serves cull_count and cull_emit on a mesh of V vertices and F faces (128-byte aligned); 0 when V or F is out of range. */
size_t ibgs_dtu_required_cull_scratch(int64_t V, int64_t F);

/* keep (V bytes): a face survives iff its three indices are in range and kept.  Leaves the output row of every vertex and face in the scratch and
 * state[VERTICES_OUT], state[FACES_OUT]; faces with an index outside [0, V) are counted in state[BAD_FACES]. */
int32_t ibgs_dtu_cull_count(void* stream, int32_t V, int32_t F, const int32_t* faces, const uint8_t* keep, void* scratch, size_t scratch_bytes, uint32_t* state);

/* After cull_count on the same arguments, V_out / F_out = its totals.  vertices_out (V_out x 3): the kept vertices in index order, each coordinate
 * v * scale + host_offset[k] in f32 (a multiply, then an add); colors / normals (or null) are copied to colors_out / normals_out bit for bit; faces_out
 * (F_out x 3): the surviving faces in order, re-indexed. */
int32_t ibgs_dtu_cull_emit(void* stream, int32_t V, int32_t F, const float* vertices, const int32_t* faces, const float* colors, const float* normals,
                           const void* scratch, size_t scratch_bytes, float scale, const float* host_offset, int32_t V_out, int32_t F_out, float* vertices_out,
                           int32_t* faces_out, float* colors_out, float* normals_out, uint32_t* state);

/* In f64 from the f32 points: inbound[i] = all_k (p_k >= host_lo[k] and p_k < host_hi[k]); g_k = rint((p_k - host_bb0[k]) / res) (ties to even);
 * in_obs[i] = inbound[i] and all_k (0 <= g_k < shape_k) and obs_mask[g_0, g_1, g_2] != 0.  obs_mask: X x Y x Z bytes. */
int32_t ibgs_dtu_obs_filter(void* stream, int32_t N, const float* points, const uint8_t* obs_mask, int32_t X, int32_t Y, int32_t Z, const float* host_lo,
                            const float* host_hi, const double* host_bb0, double res, uint8_t* inbound, uint8_t* in_obs, uint32_t* state);

/* out[i] = ((P_0 x + P_1 y) + P_2 z) + P_3 > 0 in f64 from the f32 point; host_plane = P (4 doubles). */
int32_t ibgs_dtu_above_plane(void* stream, int32_t N, const float* points, const double* host_plane, uint8_t* out, uint32_t* state);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_DTU_H */
