/*
 * ibgs_mesh_eval.h -- C ABI of the mesh evaluation in libibgs_rast.so (ibgs_amd/csrc/mesh_eval.hip): surface sampling of a triangle mesh, thinning of a
 * point cloud to a minimum spacing, exact nearest neighbours with a cut-off, and the sums behind the Chamfer distance and the F-score.
 *
 * Replaces the host-side stages of the reference's scripts/eval_dtu/eval.py (sampling, the radius-neighbour thinning loop, two kd-tree sweeps) and the
 * counts of scripts/tnt_eval/evaluation.py:176-180.  The contract is this project's own statement of those stages: DESIGN.md section 11 ("Mesh
 * evaluation") and the header of mesh_eval.hip; tests/mesh_eval_ref.py restates it.
 *
 * Conventions are those of ibgs_rast.h: device pointers unless the name starts with "host_", `stream` is a hipStream_t passed as void*, return value
 * >= 0 on success, < 0 = -(IBGS_ERR_*) with ibgs_last_error() holding the message.  The caller owns every array (ibgs_amd/mesh_eval.py allocates them
 * with torch, and does the two sorts with torch.sort); the library keeps no state and never waits for the device.
 *
 * Limits: 0 <= V < 2^31, 0 <= F < 2^30, 0 <= N, Q < 2^31.
 */
#ifndef IBGS_MESH_EVAL_H
#define IBGS_MESH_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* words of `state` (uint32, device; zeroed by the caller; all sticky: a non-zero word other than UNDECIDED means the caller must fail the call) */
#define IBGS_MEVAL_BAD_FACES 0            /* triangles with a vertex index outside [0, V): never dereferenced, they yield no samples */
#define IBGS_MEVAL_SAMPLE_OVERFLOW 1      /* triangles with n1 or n2 above IBGS_MEVAL_MAX_SIDE: they yield no samples */
#define IBGS_MEVAL_BAD_POINTS 2           /* points or queries with a non-finite coordinate */
#define IBGS_MEVAL_OVERRUN 3              /* samples that fell outside the output (0 unless n_out passed to sample_emit is not sample_count's total) */
#define IBGS_MEVAL_UNDECIDED 4            /* points the last round of ibgs_meval_thin_rounds left undecided (overwritten by every call, not sticky) */
#define IBGS_MEVAL_STATE_WORDS 8

#define IBGS_MEVAL_MAX_SIDE 32768         /* largest n1 / n2 of one triangle */
#define IBGS_MEVAL_LEAF 8                 /* points per leaf box = boxes per parent box of the search hierarchy */

/* thin_rounds' status of a point */
#define IBGS_MEVAL_THIN_UNDECIDED 0
#define IBGS_MEVAL_THIN_KEPT 1
#define IBGS_MEVAL_THIN_REMOVED 2

/* ---- surface sampling: count per triangle -> 64-bit scan -> emit -------------------------------------------------------------------------------- */
size_t ibgs_meval_required_sample_scratch(int64_t F);          /* 0 when F is out of range */

/* Samples per triangle (left in the scratch, scanned) and their total (total[0], uint64, device).  density > 0. */
int32_t ibgs_meval_sample_count(void* stream, int32_t V, int32_t F, const float* vertices, const int32_t* faces, double density, void* scratch,
                                size_t scratch_bytes, uint64_t* total, uint32_t* state);

/* The samples, triangles in index order, i-major within a triangle: out is n_out x 3 floats, n_out = sample_count's total (same mesh, density, scratch). */
int32_t ibgs_meval_sample_emit(void* stream, int32_t V, int32_t F, const float* vertices, const int32_t* faces, double density, const void* scratch,
                               size_t scratch_bytes, int64_t n_out, float* out, uint32_t* state);

/* ---- the search hierarchy over a point set ------------------------------------------------------------------------------------------------------ */
/* Morton key (63 bits) of every point inside bounds = {lo x, y, z, hi x, y, z} (6 floats, device; points outside are clamped).  The keys only order
 * the points; no result depends on them. */
int32_t ibgs_meval_keys(void* stream, int32_t N, const float* points, const float* bounds, int64_t* keys, uint32_t* state);

size_t ibgs_meval_required_tree(int64_t N);                    /* 0 when N is out of range */

/* order (N int64): the points' indices in ascending key order (an entry outside [0, N) is counted in state[IBGS_MEVAL_OVERRUN], never dereferenced).
 * tag (N int32, or null): the word that travels with point i (null: i itself).  tree: ibgs_meval_required_tree(N) bytes, 128-byte aligned. */
int32_t ibgs_meval_build(void* stream, int32_t N, const float* points, const int64_t* order, const int32_t* tag, void* tree, size_t tree_bytes,
                         uint32_t* state);

/* ---- thinning: `rounds` rounds of the rule over a hierarchy whose tags are the points' visiting ranks ------------------------------------------- */
/* status (N uint32, in the hierarchy's order, zeroed before the first call).  state[IBGS_MEVAL_UNDECIDED] = what the last round left. */
int32_t ibgs_meval_thin_rounds(void* stream, int32_t N, const void* tree, size_t tree_bytes, float radius, uint32_t* status, int32_t rounds,
                               uint32_t* state);

/* ---- exact nearest neighbour of every query among the N points of a hierarchy whose tags are the points' indices -------------------------------- */
/* qorder (Q int64, or null): the order in which the queries are walked (a locality hint; results go to the query's own row). */
int32_t ibgs_meval_nearest(void* stream, int32_t Q, const float* query, const int64_t* qorder, int32_t N, const void* tree, size_t tree_bytes,
                           float max_dist, float* dist, int32_t* index, uint32_t* state);

/* sum[0] += the f64 sum and count[0] += the number of the dist[i] < threshold (both zeroed by the caller). */
int32_t ibgs_meval_reduce(void* stream, int32_t Q, const float* dist, float threshold, double* sum, uint64_t* count);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_MESH_EVAL_H */
