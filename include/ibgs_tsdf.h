/*
 * ibgs_tsdf.h -- C ABI of the TSDF fusion and marching-cubes mesh extraction in libibgs_rast.so (ibgs_amd/csrc/tsdf.hip).
 *
 * Replaces the host-side Open3D volume of the reference's mesh output (render.py:262-286, 328-331, 355-364:
 * ScalableTSDFVolume(voxel_length, sdf_trunc = 4 voxel_length, RGB8).integrate / extract_triangle_mesh).  The contract -- block layout,
 * the per-voxel update and the marching cubes -- is stated in DESIGN.md section 11 and in the header of tsdf.hip.
 *
 * Conventions are those of ibgs_rast.h: device pointers unless the name starts with "host_", `stream` is a hipStream_t passed as void*,
 * return value >= 0 on success, < 0 = -(IBGS_ERR_*) with ibgs_last_error() holding the message.  The caller owns every array (ibgs_amd/tsdf.py
 * allocates them with torch); the library keeps no state.
 */
#ifndef IBGS_TSDF_H
#define IBGS_TSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_TSDF_BLOCK 8                 /* voxels per block side: 8^3 = 512 voxels, one workgroup */
#define IBGS_TSDF_COORD_BITS 21           /* signed block coordinates in [-2^20, 2^20 - 1], packed x | y << 21 | z << 42 (biased by 2^20) */

/* words of ibgs_tsdf_volume.state (uint32, device) */
#define IBGS_TSDF_ALLOCATED 0             /* blocks handed out so far (may pass `capacity`: the excess failed) */
#define IBGS_TSDF_FAILED 1                /* distinct blocks that found no room (sticky until the arrays are reset) */
#define IBGS_TSDF_IGNORED 2               /* valid pixels whose truncation cube leaves the packable range */
#define IBGS_TSDF_ACTIVE 3                /* blocks active in the current view (the length of `active`) */
#define IBGS_TSDF_VERTICES 4              /* marching cubes: vertex total (after ibgs_tsdf_mesh_count) */
#define IBGS_TSDF_FACES 5                 /* marching cubes: face total */
#define IBGS_TSDF_OVERRUN 6               /* marching cubes: emits that fell outside the output arrays (0 unless the library is broken) */
#define IBGS_TSDF_TABLE_FULL 7            /* insertions that found every hash slot taken (sticky; FAILED then counts only the keys that got a slot) */
#define IBGS_TSDF_STATE_WORDS 8

#define IBGS_TSDF_FLAG_NO_DEDUP 1         /* allocation without the per-workgroup LDS dedup: every (pixel, block) goes to the global hash (A/B only) */

typedef struct ibgs_tsdf_volume {
    float voxel_length;                   /* v */
    float sdf_trunc;                      /* tau */
    int32_t capacity;                     /* blocks */
    int32_t slot_bits;                    /* the hash has 2^slot_bits slots (>= capacity) */
    int64_t* slot_key;                    /* 2^slot_bits packed keys, -1 = empty */
    int32_t* slot_block;                  /* 2^slot_bits block index of the slot's key, -1 = none (empty or failed) */
    uint32_t* slot_mark;                  /* 2^slot_bits, 1 while the slot's block is active in the current view (all 0 between views) */
    int32_t* active;                      /* 2^slot_bits slots active in the current view */
    int64_t* block_key;                   /* capacity packed keys of the allocated blocks, INT64_MAX for free ones */
    float* tsdf;                          /* capacity x 512, voxel l = i + 8 j + 64 k of a block; zeroed by the caller before first use */
    float* weight;                        /* capacity x 512 */
    float* color;                         /* 3 x capacity x 512 (planar) */
    uint32_t* state;                      /* IBGS_TSDF_STATE_WORDS, zeroed by the caller */
} ibgs_tsdf_volume;

typedef struct ibgs_tsdf_view {
    int32_t W, H;
    float fx, fy, cx, cy;                 /* pixel centres at integer coordinates */
    float depth_trunc;                    /* a pixel is valid iff 0 < depth <= depth_trunc */
    float world_to_camera[12];            /* rows 0..2 of the 4 x 4 pose */
    float camera_to_world[12];            /* rows 0..2 of its inverse (the caller's: the reference restatement uses the same numbers) */
} ibgs_tsdf_view;

typedef struct ibgs_tsdf_mesh_scratch {
    const int64_t* order;                 /* capacity block indices in ascending key order (the allocated blocks first) */
    int32_t* rank;                        /* capacity: position of each block in `order` */
    uint16_t* vinfo;                      /* capacity x 512: edge mask (3 bits) | in-block vertex offset << 3 */
    int32_t* vcount;                      /* capacity + 1: vertices per block, then their exclusive offsets */
    int32_t* fcount;                      /* capacity + 1: faces per block, then their exclusive offsets */
} ibgs_tsdf_mesh_scratch;

size_t ibgs_tsdf_sizeof_volume(void);
size_t ibgs_tsdf_sizeof_view(void);
size_t ibgs_tsdf_sizeof_mesh_scratch(void);

/* The marching-cubes triangle table: host_out[256 * 16], row = case (bit c set when corner c = dx | dy << 1 | dz << 2 is negative), up to five
 * triangles of three edge indices (edge 4 a + (ob | oc << 1): axis a, owner offsets ob / oc on the other two axes), -1 after the last. */
int32_t ibgs_tsdf_mc_table(int32_t* host_out);

/* One view: allocate / activate the blocks of every valid pixel's truncation cube, then update every voxel of the active blocks.  Issues a
 * memset and two kernels on `stream`; never waits for the device.  color (3 x H x W) may be NULL: the colours are then left as they are. */
int32_t ibgs_tsdf_integrate(void* stream, const ibgs_tsdf_volume* vol, const ibgs_tsdf_view* view, const float* depth, const float* color, uint32_t flags);

/* Marching cubes, passes 1-2: per-block counts and their exclusive scan; the totals land in state[IBGS_TSDF_VERTICES / FACES]. */
int32_t ibgs_tsdf_mesh_count(void* stream, const ibgs_tsdf_volume* vol, const ibgs_tsdf_mesh_scratch* scratch);

/* Marching cubes, pass 3: vertices (V x 3), their normals and colours (V x 3), faces (F x 3); V / F are the totals of mesh_count. */
int32_t ibgs_tsdf_mesh_emit(void* stream, const ibgs_tsdf_volume* vol, const ibgs_tsdf_mesh_scratch* scratch, int32_t V, int32_t F,
                            float* vertices, float* normals, float* colors, int32_t* faces);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_TSDF_H */
