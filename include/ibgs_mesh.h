/*
 * ibgs_mesh.h -- C ABI of the triangle-mesh post-processing in libibgs_rast.so (ibgs_amd/csrc/mesh.hip): clustering of the triangles by edge
 * connectivity and removal of the small clusters.
 *
 * Replaces the host-side Open3D calls of the reference's `post_process_mesh` and `clean_mesh` (render.py:34-66:
 * cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices, remove_degenerate_triangles).  The contract is this
 * project's own statement of those routines: DESIGN.md section 11 ("Mesh post-processing") and the header of mesh.hip; tests/mesh_ref.py restates it twice.
 *
 * Conventions are those of ibgs_rast.h: device pointers unless the name starts with "host_", `stream` is a hipStream_t passed as void*,
 * return value >= 0 on success, < 0 = -(IBGS_ERR_*) with ibgs_last_error() holding the message.  The caller owns every array (ibgs_amd/mesh.py
 * allocates them with torch); the library keeps no state and never waits for the device.
 *
 * Limits: 0 <= V < 2^31, 0 <= F < 2^30.
 */
#ifndef IBGS_MESH_H
#define IBGS_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* words of ibgs_mesh.state (uint32, device; zeroed by the caller before ibgs_mesh_cluster) */
#define IBGS_MESH_BAD_FACES 0             /* triangles with a vertex index outside [0, V): never dereferenced; the caller must fail the call (sticky) */
#define IBGS_MESH_CLUSTERS 1              /* C, after ibgs_mesh_cluster */
#define IBGS_MESH_VERTICES_OUT 2          /* V', after ibgs_mesh_filter_count */
#define IBGS_MESH_FACES_OUT 3             /* F', after ibgs_mesh_filter_count */
#define IBGS_MESH_TABLE_FULL 4            /* edges that found no slot of the edge table (0 unless the library is broken: the table holds twice the edges) */
#define IBGS_MESH_OVERRUN 5               /* emits that fell outside the output arrays (0 unless V' / F' passed to filter_emit are not filter_count's) */
#define IBGS_MESH_STATE_WORDS 8

#define IBGS_MESH_KEEP_VERTICES 1         /* filter: leave the vertex arrays alone (clean_mesh); faces keep their indices, V' = V */
#define IBGS_MESH_KEEP_DEGENERATE 2       /* filter: do not remove surviving triangles that repeat a vertex index */

typedef struct ibgs_mesh {
    int32_t V, F;
    const float* vertices;                /* V x 3 */
    const int32_t* faces;                 /* F x 3 */
    void* scratch;                        /* ibgs_mesh_required_scratch(V, F) bytes, 128-byte aligned; its content links the calls on one mesh */
    size_t scratch_bytes;
    uint32_t* state;                      /* IBGS_MESH_STATE_WORDS */
} ibgs_mesh;

size_t ibgs_mesh_sizeof_mesh(void);

/* bytes of ibgs_mesh.scratch for a mesh of V vertices and F faces (0 when V or F is out of range) */
size_t ibgs_mesh_required_scratch(int64_t V, int64_t F);

/* Connected components of the triangles under "share an edge" (an edge = an unordered pair of vertex indices, {a, a} included).
 * triangle_clusters (F): cluster of every triangle, clusters numbered in ascending order of their smallest triangle index.
 * cluster_n_triangles (F int32) and cluster_area (F float64): the first C entries are written (C = state[IBGS_MESH_CLUSTERS]), the rest are zero. */
int32_t ibgs_mesh_cluster(void* stream, const ibgs_mesh* mesh, int32_t* triangle_clusters, int32_t* cluster_n_triangles, double* cluster_area);

/* Filter, pass 1.  A triangle survives when keep_cluster[triangle_clusters[t]] != 0 (keep_cluster: C bytes); vertices that no survivor refers to are
 * dropped (unless IBGS_MESH_KEEP_VERTICES); then survivors that repeat a vertex index are dropped (unless IBGS_MESH_KEEP_DEGENERATE).  Leaves the
 * output positions in the scratch and the totals in state[IBGS_MESH_VERTICES_OUT / FACES_OUT]. */
int32_t ibgs_mesh_filter_count(void* stream, const ibgs_mesh* mesh, const int32_t* triangle_clusters, const uint8_t* keep_cluster, int32_t C, uint32_t flags);

/* Filter, pass 2 (same flags): faces_out (F' x 3) re-indexed, and each of n_attr per-vertex arrays of 3 floats gathered: attr_out[i] (V' x 3) from
 * attr_in[i] (V x 3).  host_attr_in / host_attr_out are host arrays of n_attr device pointers (n_attr <= 8; 0 with IBGS_MESH_KEEP_VERTICES).
 * Survivors keep their relative order; rows are copied bit for bit. */
int32_t ibgs_mesh_filter_emit(void* stream, const ibgs_mesh* mesh, uint32_t flags, int32_t V_out, int32_t F_out, int32_t* faces_out,
                              int32_t n_attr, const float* const* host_attr_in, float* const* host_attr_out);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_MESH_H */
