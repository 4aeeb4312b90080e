// TSDF fusion and marching-cubes mesh extraction (C ABI: include/ibgs_tsdf.h; Python: ibgs_amd/tsdf.py; contract: DESIGN.md section 11).
//
// The reference fuses the median depth of every training view into Open3D's ScalableTSDFVolume on the host and writes extract_triangle_mesh()
// (render.py:262-286, 328-331, 355-364).  This unit is that stage on the device: sparse blocks of 8^3 voxels behind an open-addressing hash of
// packed block keys, one workgroup per block.
//
// Volume.  Voxel (i, j, k) has its centre at ((i + 0.5) v, (j + 0.5) v, (k + 0.5) v); block (bx, by, bz) holds voxels 8 bx .. 8 bx + 7 etc.,
// voxel l = i + 8 j + 64 k inside it.  Each voxel stores tsdf, weight and colour (f32), all 0 in a new block.
//
// integrate, for one view, in this f32 operation order (the kernels are compiled with -ffp-contract=off; tests/tsdf_ref.py follows it):
//   valid pixel      0 < d <= depth_trunc
//   allocation       xc = ((u - cx) / fx) * d,  yc = ((v - cy) / fy) * d,  zc = d
//                    p_r = ((M_r0 xc + M_r1 yc) + M_r2 zc) + M_r3                       M = camera_to_world
//                    every block b with floor((p - tau) / B) <= b <= floor((p + tau) / B) on each axis, B = 8 v, is allocated if new and
//                    marked active for this view; a pixel whose range leaves [-2^20, 2^20 - 1] is ignored and counted (state[IGNORED])
//   update           X = ((float)I + 0.5) * v  (per axis)
//   (each voxel of   x_r = ((W_r0 X + W_r1 Y) + W_r2 Z) + W_r3                            W = world_to_camera; skip unless z > 0
//   an active block) pu = floor(((fx x) / z + cx) + 0.5),  pv = floor(((fy y) / z + cy) + 0.5); skip if outside the image or invalid
//                    a = (pu - cx) / fx,  b = (pv - cy) / fy,  sdf = (d - z) * sqrt((1 + a a) + b b); skip unless sdf > -tau
//                    t = min(1, sdf / tau);  tsdf = (tsdf w + t) / (w + 1);  colour_c = (colour_c w + C_c) / (w + 1);  w = w + 1
//
// extract (marching cubes over cells of 8 voxels i..i+1, j..j+1, k..k+1, across block boundaries):
//   a cell is emitted iff all 8 weights are > 0; corner bit = tsdf < 0; triangles from TSDF_MC_TRI (tools/gen_mc_table.py)
//   one vertex per crossing edge (q, axis a) that an emitted cell uses, at x0 + t (x1 - x0) with t = f0 / (f0 - f1) (per component; the same t
//   for the colour); its normal = the sum, in the order (cell around the edge k = ob | oc << 1, triangle of the cell), of (p1 - p0) x (p2 - p0)
//   over the triangles that use the vertex, divided by its length sqrt((nx nx + ny ny) + nz nz) (zero stays zero)
//   order: blocks by ascending packed key, then cell / voxel l, then edge axis (vertices) or table order (faces): equal volumes give
//   bit-identical meshes whatever their hash slots
//
// Kernels and what bounds them (numbers: DESIGN.md section 11, profiles/tsdf.txt):
//   tsdf_alloc_kernel      pixel-parallel, 16 x 16 pixels per workgroup.  The blocks a tile's cubes touch are first merged in an LDS hash
//                          (neighbouring pixels hit the same blocks), then each distinct one goes to the global hash once: one global CAS
//                          per (workgroup, block) instead of per (pixel, block).  The first touch of a block's slot this view appends the slot
//                          to the active list (the per-slot mark is exchanged atomically), so the list needs no pass over the table.
//   tsdf_integrate_kernel  one 512-thread workgroup per active block (grid-stride over the device-side count), one thread per voxel: no atomics
//                          on voxel data, deterministic.  HBM-bound: 20 B read + 20 B written per voxel (12 + 12 without colour).
//   tsdf_mc_count_kernel   per block in key order: the 10^3 voxels around it into LDS, cell cases, vertex edges, in-block vertex offsets
//   tsdf_mc_scan_kernel    one workgroup: exclusive scan of the per-block vertex / face counts, totals into state[]
//   tsdf_mc_emit_kernel    per block: vertices (position, colour, normal from the <= 4 cells around the edge: no float atomics) and faces
//                          (vertex indices of neighbouring blocks from their offsets); every store is bounds-checked against V / F.
// integrate never waits for the device; extract reads back the totals once (ibgs_amd/tsdf.py).
#include <cmath>
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_tsdf.h"

namespace ibgs {

constexpr int TB = IBGS_TSDF_BLOCK;                 // 8
constexpr int TVOX = TB * TB * TB;                  // 512 voxels = threads of a block's workgroup
constexpr int64_t TSDF_EMPTY = -1;
constexpr int TSDF_BIAS = 1 << (IBGS_TSDF_COORD_BITS - 1);
constexpr int TSDF_CMASK = (1 << IBGS_TSDF_COORD_BITS) - 1;

// The marching-cubes table (tools/gen_mc_table.py; checked exhaustively by tests/test_tsdf_table.py).  Corner c = dx | dy << 1 | dz << 2,
// edge e = 4 a + (ob | oc << 1) (axis a, owner offsets ob / oc on the two other axes in increasing order).
static constexpr int8_t TSDF_MC_TRI[256][16] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   0
    { 0,  4,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   1
    { 0,  9,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   2
    { 4,  9,  5,  4,  8,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   3
    { 1, 10,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   4
    { 0, 10,  8,  0,  1, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   5
    { 0,  9,  5,  1, 10,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   6
    { 8,  1, 10,  8,  5,  1,  8,  9,  5, -1, -1, -1, -1, -1, -1, -1},  //   7
    { 1,  5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   8
    { 0,  4,  8,  1,  5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //   9
    { 0, 11,  1,  0,  9, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  10
    { 9,  4,  8,  9,  1,  4,  9, 11,  1, -1, -1, -1, -1, -1, -1, -1},  //  11
    { 4, 11, 10,  4,  5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  12
    {10,  5, 11, 10,  0,  5, 10,  8,  0, -1, -1, -1, -1, -1, -1, -1},  //  13
    {11,  0,  9, 11,  4,  0, 11, 10,  4, -1, -1, -1, -1, -1, -1, -1},  //  14
    { 8, 11, 10,  8,  9, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  15
    { 2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  16
    { 0,  6,  2,  0,  4,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  17
    { 0,  9,  5,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  18
    { 4,  9,  5,  4,  2,  9,  4,  6,  2, -1, -1, -1, -1, -1, -1, -1},  //  19
    { 1, 10,  4,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  20
    { 0,  6,  2,  0, 10,  6,  0,  1, 10, -1, -1, -1, -1, -1, -1, -1},  //  21
    { 0,  9,  5,  1, 10,  4,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1},  //  22
    { 1,  9,  5,  1,  2,  9,  1,  6,  2,  1, 10,  6, -1, -1, -1, -1},  //  23
    { 1,  5, 11,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  24
    { 0,  6,  2,  0,  4,  6,  1,  5, 11, -1, -1, -1, -1, -1, -1, -1},  //  25
    { 0, 11,  1,  0,  9, 11,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1},  //  26
    {11,  2,  9, 11,  6,  2, 11,  4,  6, 11,  1,  4, -1, -1, -1, -1},  //  27
    { 2,  8,  6,  4, 11, 10,  4,  5, 11, -1, -1, -1, -1, -1, -1, -1},  //  28
    { 0,  6,  2,  0, 10,  6,  0, 11, 10,  0,  5, 11, -1, -1, -1, -1},  //  29
    {11,  0,  9, 11,  4,  0, 11, 10,  4,  2,  8,  6, -1, -1, -1, -1},  //  30
    {11,  2,  9, 11,  6,  2, 11, 10,  6, -1, -1, -1, -1, -1, -1, -1},  //  31
    { 2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  32
    { 0,  4,  8,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  33
    { 0,  7,  5,  0,  2,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  34
    { 5,  2,  7,  5,  8,  2,  5,  4,  8, -1, -1, -1, -1, -1, -1, -1},  //  35
    { 1, 10,  4,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  36
    { 0, 10,  8,  0,  1, 10,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1},  //  37
    { 0,  7,  5,  0,  2,  7,  1, 10,  4, -1, -1, -1, -1, -1, -1, -1},  //  38
    { 5,  2,  7,  5,  8,  2,  5, 10,  8,  5,  1, 10, -1, -1, -1, -1},  //  39
    { 1,  5, 11,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  40
    { 0,  4,  8,  1,  5, 11,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1},  //  41
    { 0, 11,  1,  0,  7, 11,  0,  2,  7, -1, -1, -1, -1, -1, -1, -1},  //  42
    { 1,  7, 11,  1,  2,  7,  1,  8,  2,  1,  4,  8, -1, -1, -1, -1},  //  43
    { 2,  7,  9,  4, 11, 10,  4,  5, 11, -1, -1, -1, -1, -1, -1, -1},  //  44
    {10,  5, 11, 10,  0,  5, 10,  8,  0,  2,  7,  9, -1, -1, -1, -1},  //  45
    { 0, 10,  4,  0, 11, 10,  0,  7, 11,  0,  2,  7, -1, -1, -1, -1},  //  46
    {10,  7, 11, 10,  2,  7, 10,  8,  2, -1, -1, -1, -1, -1, -1, -1},  //  47
    { 6,  9,  8,  6,  7,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  48
    { 6,  0,  4,  6,  9,  0,  6,  7,  9, -1, -1, -1, -1, -1, -1, -1},  //  49
    { 7,  8,  6,  7,  0,  8,  7,  5,  0, -1, -1, -1, -1, -1, -1, -1},  //  50
    { 4,  7,  5,  4,  6,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  51
    { 1, 10,  4,  6,  9,  8,  6,  7,  9, -1, -1, -1, -1, -1, -1, -1},  //  52
    { 0,  7,  9,  0,  6,  7,  0, 10,  6,  0,  1, 10, -1, -1, -1, -1},  //  53
    { 7,  8,  6,  7,  0,  8,  7,  5,  0,  1, 10,  4, -1, -1, -1, -1},  //  54
    { 7, 10,  6,  7,  1, 10,  7,  5,  1, -1, -1, -1, -1, -1, -1, -1},  //  55
    { 1,  5, 11,  6,  9,  8,  6,  7,  9, -1, -1, -1, -1, -1, -1, -1},  //  56
    { 6,  0,  4,  6,  9,  0,  6,  7,  9,  1,  5, 11, -1, -1, -1, -1},  //  57
    { 0, 11,  1,  0,  7, 11,  0,  6,  7,  0,  8,  6, -1, -1, -1, -1},  //  58
    { 6,  1,  4,  6, 11,  1,  6,  7, 11, -1, -1, -1, -1, -1, -1, -1},  //  59
    { 4, 11, 10,  4,  5, 11,  6,  9,  8,  6,  7,  9, -1, -1, -1, -1},  //  60
    { 0,  7,  9,  0,  6,  7,  0, 10,  6,  0, 11, 10,  0,  5, 11, -1},  //  61
    { 0, 10,  4,  0, 11, 10,  0,  7, 11,  0,  6,  7,  0,  8,  6, -1},  //  62
    { 6, 11, 10,  6,  7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  63
    { 3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  64
    { 0,  4,  8,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  65
    { 0,  9,  5,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  66
    { 3,  6, 10,  4,  9,  5,  4,  8,  9, -1, -1, -1, -1, -1, -1, -1},  //  67
    { 1,  6,  4,  1,  3,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  68
    { 1,  8,  0,  1,  6,  8,  1,  3,  6, -1, -1, -1, -1, -1, -1, -1},  //  69
    { 0,  9,  5,  1,  6,  4,  1,  3,  6, -1, -1, -1, -1, -1, -1, -1},  //  70
    { 1,  9,  5,  1,  8,  9,  1,  6,  8,  1,  3,  6, -1, -1, -1, -1},  //  71
    { 1,  5, 11,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  72
    { 0,  4,  8,  1,  5, 11,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},  //  73
    { 0, 11,  1,  0,  9, 11,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},  //  74
    { 9,  4,  8,  9,  1,  4,  9, 11,  1,  3,  6, 10, -1, -1, -1, -1},  //  75
    { 4,  3,  6,  4, 11,  3,  4,  5, 11, -1, -1, -1, -1, -1, -1, -1},  //  76
    { 0,  6,  8,  0,  3,  6,  0, 11,  3,  0,  5, 11, -1, -1, -1, -1},  //  77
    { 4,  3,  6,  4, 11,  3,  4,  9, 11,  4,  0,  9, -1, -1, -1, -1},  //  78
    { 9,  6,  8,  9,  3,  6,  9, 11,  3, -1, -1, -1, -1, -1, -1, -1},  //  79
    { 2, 10,  3,  2,  8, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  80
    { 2, 10,  3,  2,  4, 10,  2,  0,  4, -1, -1, -1, -1, -1, -1, -1},  //  81
    { 0,  9,  5,  2, 10,  3,  2,  8, 10, -1, -1, -1, -1, -1, -1, -1},  //  82
    { 2, 10,  3,  2,  4, 10,  2,  5,  4,  2,  9,  5, -1, -1, -1, -1},  //  83
    { 3,  4,  1,  3,  8,  4,  3,  2,  8, -1, -1, -1, -1, -1, -1, -1},  //  84
    { 0,  3,  2,  0,  1,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  85
    { 0,  9,  5,  3,  4,  1,  3,  8,  4,  3,  2,  8, -1, -1, -1, -1},  //  86
    { 3,  5,  1,  3,  9,  5,  3,  2,  9, -1, -1, -1, -1, -1, -1, -1},  //  87
    { 1,  5, 11,  2, 10,  3,  2,  8, 10, -1, -1, -1, -1, -1, -1, -1},  //  88
    { 2, 10,  3,  2,  4, 10,  2,  0,  4,  1,  5, 11, -1, -1, -1, -1},  //  89
    { 0, 11,  1,  0,  9, 11,  2, 10,  3,  2,  8, 10, -1, -1, -1, -1},  //  90
    { 4, 11,  1,  4,  9, 11,  4,  2,  9,  4,  3,  2,  4, 10,  3, -1},  //  91
    { 2, 11,  3,  2,  5, 11,  2,  4,  5,  2,  8,  4, -1, -1, -1, -1},  //  92
    { 2, 11,  3,  2,  5, 11,  2,  0,  5, -1, -1, -1, -1, -1, -1, -1},  //  93
    { 4,  2,  8,  4,  3,  2,  4, 11,  3,  4,  9, 11,  4,  0,  9, -1},  //  94
    { 2, 11,  3,  2,  9, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  95
    { 2,  7,  9,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  //  96
    { 0,  4,  8,  2,  7,  9,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},  //  97
    { 0,  7,  5,  0,  2,  7,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},  //  98
    { 5,  2,  7,  5,  8,  2,  5,  4,  8,  3,  6, 10, -1, -1, -1, -1},  //  99
    { 1,  6,  4,  1,  3,  6,  2,  7,  9, -1, -1, -1, -1, -1, -1, -1},  // 100
    { 1,  8,  0,  1,  6,  8,  1,  3,  6,  2,  7,  9, -1, -1, -1, -1},  // 101
    { 0,  7,  5,  0,  2,  7,  1,  6,  4,  1,  3,  6, -1, -1, -1, -1},  // 102
    { 8,  3,  6,  8,  1,  3,  8,  5,  1,  8,  7,  5,  8,  2,  7, -1},  // 103
    { 1,  5, 11,  2,  7,  9,  3,  6, 10, -1, -1, -1, -1, -1, -1, -1},  // 104
    { 0,  4,  8,  1,  5, 11,  2,  7,  9,  3,  6, 10, -1, -1, -1, -1},  // 105
    { 0, 11,  1,  0,  7, 11,  0,  2,  7,  3,  6, 10, -1, -1, -1, -1},  // 106
    { 1,  7, 11,  1,  2,  7,  1,  8,  2,  1,  4,  8,  3,  6, 10, -1},  // 107
    { 2,  7,  9,  4,  3,  6,  4, 11,  3,  4,  5, 11, -1, -1, -1, -1},  // 108
    { 0,  6,  8,  0,  3,  6,  0, 11,  3,  0,  5, 11,  2,  7,  9, -1},  // 109
    {11,  2,  7, 11,  0,  2, 11,  4,  0, 11,  6,  4, 11,  3,  6, -1},  // 110
    { 8,  3,  6,  8, 11,  3,  8,  7, 11,  8,  2,  7, -1, -1, -1, -1},  // 111
    { 8,  7,  9,  8,  3,  7,  8, 10,  3, -1, -1, -1, -1, -1, -1, -1},  // 112
    { 0,  7,  9,  0,  3,  7,  0, 10,  3,  0,  4, 10, -1, -1, -1, -1},  // 113
    { 5,  3,  7,  5, 10,  3,  5,  8, 10,  5,  0,  8, -1, -1, -1, -1},  // 114
    { 5,  3,  7,  5, 10,  3,  5,  4, 10, -1, -1, -1, -1, -1, -1, -1},  // 115
    { 1,  8,  4,  1,  9,  8,  1,  7,  9,  1,  3,  7, -1, -1, -1, -1},  // 116
    { 1,  9,  0,  1,  7,  9,  1,  3,  7, -1, -1, -1, -1, -1, -1, -1},  // 117
    { 8,  5,  0,  8,  7,  5,  8,  3,  7,  8,  1,  3,  8,  4,  1, -1},  // 118
    { 1,  7,  5,  1,  3,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 119
    { 1,  5, 11,  8,  7,  9,  8,  3,  7,  8, 10,  3, -1, -1, -1, -1},  // 120
    { 0,  7,  9,  0,  3,  7,  0, 10,  3,  0,  4, 10,  1,  5, 11, -1},  // 121
    { 7, 10,  3,  7,  8, 10,  7,  0,  8,  7,  1,  0,  7, 11,  1, -1},  // 122
    { 7, 10,  3,  7,  4, 10,  7,  1,  4,  7, 11,  1, -1, -1, -1, -1},  // 123
    { 3,  5, 11,  3,  4,  5,  3,  8,  4,  3,  9,  8,  3,  7,  9, -1},  // 124
    { 0,  7,  9,  0,  3,  7,  0, 11,  3,  0,  5, 11, -1, -1, -1, -1},  // 125
    { 0,  8,  4,  3,  7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 126
    { 3,  7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 127
    { 3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 128
    { 0,  4,  8,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 129
    { 0,  9,  5,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 130
    { 3, 11,  7,  4,  9,  5,  4,  8,  9, -1, -1, -1, -1, -1, -1, -1},  // 131
    { 1, 10,  4,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 132
    { 0, 10,  8,  0,  1, 10,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},  // 133
    { 0,  9,  5,  1, 10,  4,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},  // 134
    { 8,  1, 10,  8,  5,  1,  8,  9,  5,  3, 11,  7, -1, -1, -1, -1},  // 135
    { 1,  7,  3,  1,  5,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 136
    { 0,  4,  8,  1,  7,  3,  1,  5,  7, -1, -1, -1, -1, -1, -1, -1},  // 137
    { 1,  7,  3,  1,  9,  7,  1,  0,  9, -1, -1, -1, -1, -1, -1, -1},  // 138
    { 1,  7,  3,  1,  9,  7,  1,  8,  9,  1,  4,  8, -1, -1, -1, -1},  // 139
    { 5, 10,  4,  5,  3, 10,  5,  7,  3, -1, -1, -1, -1, -1, -1, -1},  // 140
    { 8,  3, 10,  8,  7,  3,  8,  5,  7,  8,  0,  5, -1, -1, -1, -1},  // 141
    { 0, 10,  4,  0,  3, 10,  0,  7,  3,  0,  9,  7, -1, -1, -1, -1},  // 142
    { 8,  3, 10,  8,  7,  3,  8,  9,  7, -1, -1, -1, -1, -1, -1, -1},  // 143
    { 2,  8,  6,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 144
    { 0,  6,  2,  0,  4,  6,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},  // 145
    { 0,  9,  5,  2,  8,  6,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},  // 146
    { 4,  9,  5,  4,  2,  9,  4,  6,  2,  3, 11,  7, -1, -1, -1, -1},  // 147
    { 1, 10,  4,  2,  8,  6,  3, 11,  7, -1, -1, -1, -1, -1, -1, -1},  // 148
    { 0,  6,  2,  0, 10,  6,  0,  1, 10,  3, 11,  7, -1, -1, -1, -1},  // 149
    { 0,  9,  5,  1, 10,  4,  2,  8,  6,  3, 11,  7, -1, -1, -1, -1},  // 150
    { 1,  9,  5,  1,  2,  9,  1,  6,  2,  1, 10,  6,  3, 11,  7, -1},  // 151
    { 1,  7,  3,  1,  5,  7,  2,  8,  6, -1, -1, -1, -1, -1, -1, -1},  // 152
    { 0,  6,  2,  0,  4,  6,  1,  7,  3,  1,  5,  7, -1, -1, -1, -1},  // 153
    { 1,  7,  3,  1,  9,  7,  1,  0,  9,  2,  8,  6, -1, -1, -1, -1},  // 154
    { 9,  6,  2,  9,  4,  6,  9,  1,  4,  9,  3,  1,  9,  7,  3, -1},  // 155
    { 2,  8,  6,  5, 10,  4,  5,  3, 10,  5,  7,  3, -1, -1, -1, -1},  // 156
    {10,  7,  3, 10,  5,  7, 10,  0,  5, 10,  2,  0, 10,  6,  2, -1},  // 157
    { 0, 10,  4,  0,  3, 10,  0,  7,  3,  0,  9,  7,  2,  8,  6, -1},  // 158
    {10,  7,  3, 10,  9,  7, 10,  2,  9, 10,  6,  2, -1, -1, -1, -1},  // 159
    { 2, 11,  9,  2,  3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 160
    { 0,  4,  8,  2, 11,  9,  2,  3, 11, -1, -1, -1, -1, -1, -1, -1},  // 161
    { 2,  5,  0,  2, 11,  5,  2,  3, 11, -1, -1, -1, -1, -1, -1, -1},  // 162
    { 2,  4,  8,  2,  5,  4,  2, 11,  5,  2,  3, 11, -1, -1, -1, -1},  // 163
    { 1, 10,  4,  2, 11,  9,  2,  3, 11, -1, -1, -1, -1, -1, -1, -1},  // 164
    { 0, 10,  8,  0,  1, 10,  2, 11,  9,  2,  3, 11, -1, -1, -1, -1},  // 165
    { 2,  5,  0,  2, 11,  5,  2,  3, 11,  1, 10,  4, -1, -1, -1, -1},  // 166
    { 5,  3, 11,  5,  2,  3,  5,  8,  2,  5, 10,  8,  5,  1, 10, -1},  // 167
    { 3,  9,  2,  3,  5,  9,  3,  1,  5, -1, -1, -1, -1, -1, -1, -1},  // 168
    { 0,  4,  8,  3,  9,  2,  3,  5,  9,  3,  1,  5, -1, -1, -1, -1},  // 169
    { 0,  3,  1,  0,  2,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 170
    { 3,  8,  2,  3,  4,  8,  3,  1,  4, -1, -1, -1, -1, -1, -1, -1},  // 171
    { 2,  5,  9,  2,  4,  5,  2, 10,  4,  2,  3, 10, -1, -1, -1, -1},  // 172
    { 5,  8,  0,  5, 10,  8,  5,  3, 10,  5,  2,  3,  5,  9,  2, -1},  // 173
    { 2,  4,  0,  2, 10,  4,  2,  3, 10, -1, -1, -1, -1, -1, -1, -1},  // 174
    { 2, 10,  8,  2,  3, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 175
    { 9,  3, 11,  9,  6,  3,  9,  8,  6, -1, -1, -1, -1, -1, -1, -1},  // 176
    { 9,  3, 11,  9,  6,  3,  9,  4,  6,  9,  0,  4, -1, -1, -1, -1},  // 177
    { 0, 11,  5,  0,  3, 11,  0,  6,  3,  0,  8,  6, -1, -1, -1, -1},  // 178
    { 4, 11,  5,  4,  3, 11,  4,  6,  3, -1, -1, -1, -1, -1, -1, -1},  // 179
    { 1, 10,  4,  9,  3, 11,  9,  6,  3,  9,  8,  6, -1, -1, -1, -1},  // 180
    { 6,  1, 10,  6,  0,  1,  6,  9,  0,  6, 11,  9,  6,  3, 11, -1},  // 181
    { 0, 11,  5,  0,  3, 11,  0,  6,  3,  0,  8,  6,  1, 10,  4, -1},  // 182
    { 5,  3, 11,  5,  6,  3,  5, 10,  6,  5,  1, 10, -1, -1, -1, -1},  // 183
    { 1,  6,  3,  1,  8,  6,  1,  9,  8,  1,  5,  9, -1, -1, -1, -1},  // 184
    { 9,  1,  5,  9,  3,  1,  9,  6,  3,  9,  4,  6,  9,  0,  4, -1},  // 185
    { 1,  6,  3,  1,  8,  6,  1,  0,  8, -1, -1, -1, -1, -1, -1, -1},  // 186
    { 1,  6,  3,  1,  4,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 187
    { 3,  8,  6,  3,  9,  8,  3,  5,  9,  3,  4,  5,  3, 10,  4, -1},  // 188
    { 0,  5,  9,  3, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 189
    { 0, 10,  4,  0,  3, 10,  0,  6,  3,  0,  8,  6, -1, -1, -1, -1},  // 190
    { 3, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 191
    { 6, 11,  7,  6, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 192
    { 0,  4,  8,  6, 11,  7,  6, 10, 11, -1, -1, -1, -1, -1, -1, -1},  // 193
    { 0,  9,  5,  6, 11,  7,  6, 10, 11, -1, -1, -1, -1, -1, -1, -1},  // 194
    { 4,  9,  5,  4,  8,  9,  6, 11,  7,  6, 10, 11, -1, -1, -1, -1},  // 195
    { 6, 11,  7,  6,  1, 11,  6,  4,  1, -1, -1, -1, -1, -1, -1, -1},  // 196
    { 0,  6,  8,  0,  7,  6,  0, 11,  7,  0,  1, 11, -1, -1, -1, -1},  // 197
    { 0,  9,  5,  6, 11,  7,  6,  1, 11,  6,  4,  1, -1, -1, -1, -1},  // 198
    { 1,  9,  5,  1,  8,  9,  1,  6,  8,  1,  7,  6,  1, 11,  7, -1},  // 199
    { 7,  1,  5,  7, 10,  1,  7,  6, 10, -1, -1, -1, -1, -1, -1, -1},  // 200
    { 0,  4,  8,  7,  1,  5,  7, 10,  1,  7,  6, 10, -1, -1, -1, -1},  // 201
    { 0, 10,  1,  0,  6, 10,  0,  7,  6,  0,  9,  7, -1, -1, -1, -1},  // 202
    { 1,  6, 10,  1,  7,  6,  1,  9,  7,  1,  8,  9,  1,  4,  8, -1},  // 203
    { 4,  7,  6,  4,  5,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 204
    { 7,  0,  5,  7,  8,  0,  7,  6,  8, -1, -1, -1, -1, -1, -1, -1},  // 205
    { 6,  9,  7,  6,  0,  9,  6,  4,  0, -1, -1, -1, -1, -1, -1, -1},  // 206
    { 6,  9,  7,  6,  8,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 207
    {10,  2,  8, 10,  7,  2, 10, 11,  7, -1, -1, -1, -1, -1, -1, -1},  // 208
    { 0,  7,  2,  0, 11,  7,  0, 10, 11,  0,  4, 10, -1, -1, -1, -1},  // 209
    { 0,  9,  5, 10,  2,  8, 10,  7,  2, 10, 11,  7, -1, -1, -1, -1},  // 210
    { 2, 11,  7,  2, 10, 11,  2,  4, 10,  2,  5,  4,  2,  9,  5, -1},  // 211
    { 1,  8,  4,  1,  2,  8,  1,  7,  2,  1, 11,  7, -1, -1, -1, -1},  // 212
    { 0,  7,  2,  0, 11,  7,  0,  1, 11, -1, -1, -1, -1, -1, -1, -1},  // 213
    { 0,  9,  5,  1,  8,  4,  1,  2,  8,  1,  7,  2,  1, 11,  7, -1},  // 214
    { 1,  9,  5,  1,  2,  9,  1,  7,  2,  1, 11,  7, -1, -1, -1, -1},  // 215
    {10,  2,  8, 10,  7,  2, 10,  5,  7, 10,  1,  5, -1, -1, -1, -1},  // 216
    {10,  0,  4, 10,  2,  0, 10,  7,  2, 10,  5,  7, 10,  1,  5, -1},  // 217
    { 7,  0,  9,  7,  1,  0,  7, 10,  1,  7,  8, 10,  7,  2,  8, -1},  // 218
    { 1,  4, 10,  2,  9,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 219
    { 5,  8,  4,  5,  2,  8,  5,  7,  2, -1, -1, -1, -1, -1, -1, -1},  // 220
    { 0,  7,  2,  0,  5,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 221
    { 4,  2,  8,  4,  7,  2,  4,  9,  7,  4,  0,  9, -1, -1, -1, -1},  // 222
    { 2,  9,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 223
    {11,  6, 10, 11,  2,  6, 11,  9,  2, -1, -1, -1, -1, -1, -1, -1},  // 224
    { 0,  4,  8, 11,  6, 10, 11,  2,  6, 11,  9,  2, -1, -1, -1, -1},  // 225
    { 0, 11,  5,  0, 10, 11,  0,  6, 10,  0,  2,  6, -1, -1, -1, -1},  // 226
    { 2,  4,  8,  2,  5,  4,  2, 11,  5,  2, 10, 11,  2,  6, 10, -1},  // 227
    { 4,  2,  6,  4,  9,  2,  4, 11,  9,  4,  1, 11, -1, -1, -1, -1},  // 228
    { 6,  9,  2,  6, 11,  9,  6,  1, 11,  6,  0,  1,  6,  8,  0, -1},  // 229
    {11,  4,  1, 11,  6,  4, 11,  2,  6, 11,  0,  2, 11,  5,  0, -1},  // 230
    { 1, 11,  5,  2,  6,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 231
    { 1,  6, 10,  1,  2,  6,  1,  9,  2,  1,  5,  9, -1, -1, -1, -1},  // 232
    { 0,  4,  8,  1,  6, 10,  1,  2,  6,  1,  9,  2,  1,  5,  9, -1},  // 233
    { 0, 10,  1,  0,  6, 10,  0,  2,  6, -1, -1, -1, -1, -1, -1, -1},  // 234
    { 1,  6, 10,  1,  2,  6,  1,  8,  2,  1,  4,  8, -1, -1, -1, -1},  // 235
    { 4,  2,  6,  4,  9,  2,  4,  5,  9, -1, -1, -1, -1, -1, -1, -1},  // 236
    { 6,  9,  2,  6,  5,  9,  6,  0,  5,  6,  8,  0, -1, -1, -1, -1},  // 237
    { 0,  6,  4,  0,  2,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 238
    { 2,  6,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 239
    { 8, 11,  9,  8, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 240
    {11,  4, 10, 11,  0,  4, 11,  9,  0, -1, -1, -1, -1, -1, -1, -1},  // 241
    {10,  0,  8, 10,  5,  0, 10, 11,  5, -1, -1, -1, -1, -1, -1, -1},  // 242
    { 4, 11,  5,  4, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 243
    { 9,  1, 11,  9,  4,  1,  9,  8,  4, -1, -1, -1, -1, -1, -1, -1},  // 244
    { 0, 11,  9,  0,  1, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 245
    {11,  4,  1, 11,  8,  4, 11,  0,  8, 11,  5,  0, -1, -1, -1, -1},  // 246
    { 1, 11,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 247
    { 8,  5,  9,  8,  1,  5,  8, 10,  1, -1, -1, -1, -1, -1, -1, -1},  // 248
    { 9,  1,  5,  9, 10,  1,  9,  4, 10,  9,  0,  4, -1, -1, -1, -1},  // 249
    { 0, 10,  1,  0,  8, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 250
    { 1,  4, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 251
    { 4,  9,  8,  4,  5,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 252
    { 0,  5,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 253
    { 0,  8,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 254
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},  // 255
};

__host__ __device__ __forceinline__ int tsdf_tri_count(int cs)
{
    int n = 0;
    while (n < 5 && TSDF_MC_TRI[cs][3 * n] >= 0) ++n;
    return n;
}

__device__ __forceinline__ uint32_t tsdf_hash(int64_t key, int bits)
{
    return (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}

__device__ __forceinline__ int64_t tsdf_pack(int bx, int by, int bz)
{
    return (int64_t)(bx + TSDF_BIAS) | ((int64_t)(by + TSDF_BIAS) << IBGS_TSDF_COORD_BITS) | ((int64_t)(bz + TSDF_BIAS) << (2 * IBGS_TSDF_COORD_BITS));
}

__device__ __forceinline__ bool tsdf_packable(int bx, int by, int bz)
{
    return bx >= -TSDF_BIAS && bx < TSDF_BIAS && by >= -TSDF_BIAS && by < TSDF_BIAS && bz >= -TSDF_BIAS && bz < TSDF_BIAS;
}

__device__ __forceinline__ void tsdf_unpack(int64_t key, int& bx, int& by, int& bz)
{
    bx = (int)(key & TSDF_CMASK) - TSDF_BIAS;
    by = (int)((key >> IBGS_TSDF_COORD_BITS) & TSDF_CMASK) - TSDF_BIAS;
    bz = (int)((key >> (2 * IBGS_TSDF_COORD_BITS)) & TSDF_CMASK) - TSDF_BIAS;
}

// ---- allocation ----------------------------------------------------------------------------------------------------------------------------

// the slot of `key` in the global hash, inserting it (and handing it a block) if new; -1 when the table has no room
__device__ int tsdf_insert(const ibgs_tsdf_volume& vol, int64_t key)
{
    const uint32_t mask = (1u << vol.slot_bits) - 1u;
    uint32_t s = tsdf_hash(key, vol.slot_bits);
    for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
        const int64_t seen = __hip_atomic_load(&vol.slot_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == key) return (int)s;
        if (seen != TSDF_EMPTY) continue;
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(&vol.slot_key[s]), (unsigned long long)TSDF_EMPTY,
                                                  (unsigned long long)key);
        if (prev == (unsigned long long)TSDF_EMPTY) {          // this thread inserted the key: hand it a block
            const uint32_t id = atomicAdd(&vol.state[IBGS_TSDF_ALLOCATED], 1u);
            if (id < (uint32_t)vol.capacity) {
                vol.block_key[id] = key;
                vol.slot_block[s] = (int32_t)id;
            } else {
                atomicAdd(&vol.state[IBGS_TSDF_FAILED], 1u);     // slot_block stays -1
            }
            return (int)s;
        }
        if ((int64_t)prev == key) return (int)s;
    }
    atomicAdd(&vol.state[IBGS_TSDF_TABLE_FULL], 1u);          // (every slot holds another key: only after >= capacity blocks failed)
    return -1;
}

// mark the slot active for this view; the first marker appends it to the active list
__device__ __forceinline__ void tsdf_activate(const ibgs_tsdf_volume& vol, int s)
{
    if (s < 0 || __hip_atomic_load(&vol.slot_mark[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
    if (atomicExch(&vol.slot_mark[s], 1u) == 0u) {
        const uint32_t i = atomicAdd(&vol.state[IBGS_TSDF_ACTIVE], 1u);
        if (i < (1u << vol.slot_bits)) vol.active[i] = s;
    }
}

constexpr int AL_TW = 16, AL_TH = 16, AL_THREADS = AL_TW * AL_TH;
constexpr int AL_LDS_BITS = 10, AL_LDS = 1 << AL_LDS_BITS, AL_LDS_PROBES = 32;

__global__ void __launch_bounds__(AL_THREADS) tsdf_alloc_kernel(ibgs_tsdf_volume vol, ibgs_tsdf_view view, const float* __restrict__ depth, int dedup)
{
    __shared__ int64_t s_keys[AL_LDS];
    const int tid = threadIdx.x;
    if (dedup) {
        for (int j = tid; j < AL_LDS; j += AL_THREADS) s_keys[j] = TSDF_EMPTY;
        __syncthreads();
    }
    const int u = blockIdx.x * AL_TW + (tid % AL_TW), v = blockIdx.y * AL_TH + (tid / AL_TW);
    if (u < view.W && v < view.H) {
        const float d = depth[(size_t)v * view.W + u];
        if (d > 0.f && d <= view.depth_trunc) {
            const float xc = (((float)u - view.cx) / view.fx) * d, yc = (((float)v - view.cy) / view.fy) * d;
            const float* M = view.camera_to_world;
            const float p[3] = {((M[0] * xc + M[1] * yc) + M[2] * d) + M[3], ((M[4] * xc + M[5] * yc) + M[6] * d) + M[7],
                                ((M[8] * xc + M[9] * yc) + M[10] * d) + M[11]};
            const float B = vol.voxel_length * (float)TB, tau = vol.sdf_trunc;
            float lo[3], hi[3];
            bool ok = true;
            for (int a = 0; a < 3; ++a) {
                lo[a] = floorf((p[a] - tau) / B); hi[a] = floorf((p[a] + tau) / B);
                ok = ok && lo[a] >= (float)-TSDF_BIAS && hi[a] <= (float)(TSDF_BIAS - 1);          // (false for NaN)
            }
            if (!ok) {
                atomicAdd(&vol.state[IBGS_TSDF_IGNORED], 1u);
            } else {
                for (int bz = (int)lo[2]; bz <= (int)hi[2]; ++bz)
                    for (int by = (int)lo[1]; by <= (int)hi[1]; ++by)
                        for (int bx = (int)lo[0]; bx <= (int)hi[0]; ++bx) {
                            const int64_t key = tsdf_pack(bx, by, bz);
                            bool merged = false;
                            if (dedup) {
                                uint32_t h = tsdf_hash(key, AL_LDS_BITS);
                                for (int probe = 0; probe < AL_LDS_PROBES && !merged; ++probe, h = (h + 1u) & (AL_LDS - 1)) {
                                    const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(&s_keys[h]),
                                                                              (unsigned long long)TSDF_EMPTY, (unsigned long long)key);
                                    merged = prev == (unsigned long long)TSDF_EMPTY || (int64_t)prev == key;
                                }
                            }
                            if (!merged) tsdf_activate(vol, tsdf_insert(vol, key));          // no dedup, or the LDS table is crowded
                        }
            }
        }
    }
    if (dedup) {
        __syncthreads();
        for (int j = tid; j < AL_LDS; j += AL_THREADS) {
            const int64_t key = s_keys[j];
            if (key != TSDF_EMPTY) tsdf_activate(vol, tsdf_insert(vol, key));
        }
    }
}

// ---- update ------------------------------------------------------------------------------------------------------------------------------

constexpr int IG_GRID = 1024;          // 4 resident 512-thread workgroups per CU

__global__ void __launch_bounds__(TVOX) tsdf_integrate_kernel(ibgs_tsdf_volume vol, ibgs_tsdf_view view, const float* __restrict__ depth,
                                                              const float* __restrict__ color)
{
    const int l = threadIdx.x, li = l & 7, lj = (l >> 3) & 7, lk = l >> 6;
    const uint32_t n_active = min(vol.state[IBGS_TSDF_ACTIVE], 1u << vol.slot_bits);
    const float vl = vol.voxel_length, tau = vol.sdf_trunc;
    const float* M = view.world_to_camera;
    const size_t HW = (size_t)view.W * view.H, plane = (size_t)vol.capacity * TVOX;
    for (uint32_t b = blockIdx.x; b < n_active; b += gridDim.x) {
        const int s = vol.active[b];
        const int id = vol.slot_block[s];
        if (l == 0) vol.slot_mark[s] = 0u;          // (nothing else reads the marks in this launch)
        if (id < 0) continue;
        int bx, by, bz;
        tsdf_unpack(vol.block_key[id], bx, by, bz);
        const float X = ((float)(bx * TB + li) + 0.5f) * vl, Y = ((float)(by * TB + lj) + 0.5f) * vl, Z = ((float)(bz * TB + lk) + 0.5f) * vl;
        const float x = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[3];
        const float y = ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7];
        const float z = ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11];
        if (!(z > 0.f)) continue;
        const float fu = floorf(((view.fx * x) / z + view.cx) + 0.5f), fv = floorf(((view.fy * y) / z + view.cy) + 0.5f);
        if (!(fu >= 0.f && fu < (float)view.W && fv >= 0.f && fv < (float)view.H)) continue;
        const size_t pix = (size_t)fv * view.W + (size_t)fu;
        const float d = depth[pix];
        if (!(d > 0.f && d <= view.depth_trunc)) continue;
        const float ra = (fu - view.cx) / view.fx, rb = (fv - view.cy) / view.fy;
        const float sdf = (d - z) * sqrtf((1.f + ra * ra) + rb * rb);
        if (!(sdf > -tau)) continue;
        const float t = fminf(1.f, sdf / tau);
        const size_t o = (size_t)id * TVOX + l;
        const float w = vol.weight[o], w1 = w + 1.f;
        vol.tsdf[o] = (vol.tsdf[o] * w + t) / w1;
        if (color) {
            for (int c = 0; c < 3; ++c) vol.color[c * plane + o] = (vol.color[c * plane + o] * w + color[c * HW + pix]) / w1;
        }
        vol.weight[o] = w1;
    }
}

// ---- marching cubes ------------------------------------------------------------------------------------------------------------------------

constexpr int NB = TB + 2, NB3 = NB * NB * NB;          // a block and a one-voxel halo on every side
constexpr int MC_GRID = 1024;

__device__ __forceinline__ int nbi(int x, int y, int z) { return (x + 1) + NB * ((y + 1) + NB * (z + 1)); }

__device__ int tsdf_lookup(const ibgs_tsdf_volume& vol, int64_t key)
{
    const uint32_t mask = (1u << vol.slot_bits) - 1u;
    uint32_t s = tsdf_hash(key, vol.slot_bits);
    for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
        const int64_t k = vol.slot_key[s];
        if (k == key) return vol.slot_block[s];
        if (k == TSDF_EMPTY) return -1;
    }
    return -1;
}

struct McLds {
    float t[NB3];
    float c[3][NB3];
    uint8_t ok[NB3];          // weight > 0
    int nb[27];               // block index of neighbour (ox + 1) + 3 (oy + 1) + 9 (oz + 1), -1 = none
    int wsum[2][TVOX / 64];          // two rows: a vertex scan and a face scan (block_exclusive_scan) are in flight together
};

// the 27 blocks around block `id` and its 10^3 voxels (colours too when `with_color`) into LDS; ends with a barrier
__device__ void mc_load(const ibgs_tsdf_volume& vol, McLds& L, int id, int bx, int by, int bz, bool with_color)
{
    const int tid = threadIdx.x;
    if (tid < 27) {
        const int ox = tid % 3 - 1, oy = (tid / 3) % 3 - 1, oz = tid / 9 - 1;
        int nid = id;
        if (tid != 13) nid = tsdf_packable(bx + ox, by + oy, bz + oz) ? tsdf_lookup(vol, tsdf_pack(bx + ox, by + oy, bz + oz)) : -1;
        L.nb[tid] = nid < vol.capacity ? nid : -1;
    }
    __syncthreads();
    const size_t plane = (size_t)vol.capacity * TVOX;
    for (int h = tid; h < NB3; h += TVOX) {
        const int hx = h % NB - 1, hy = (h / NB) % NB - 1, hz = h / (NB * NB) - 1;
        const int ox = hx < 0 ? -1 : (hx >= TB ? 1 : 0), oy = hy < 0 ? -1 : (hy >= TB ? 1 : 0), oz = hz < 0 ? -1 : (hz >= TB ? 1 : 0);
        const int nid = L.nb[(ox + 1) + 3 * (oy + 1) + 9 * (oz + 1)];
        float t = 0.f, w = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (nid >= 0) {
            const size_t o = (size_t)nid * TVOX + (hx - TB * ox) + TB * (hy - TB * oy) + TB * TB * (hz - TB * oz);
            t = vol.tsdf[o]; w = vol.weight[o];
            if (with_color) { c0 = vol.color[o]; c1 = vol.color[plane + o]; c2 = vol.color[2 * plane + o]; }
        }
        L.t[h] = t; L.ok[h] = w > 0.f;
        if (with_color) { L.c[0][h] = c0; L.c[1][h] = c1; L.c[2][h] = c2; }
    }
    __syncthreads();
}

// case of the cell with min corner (x, y, z) (-1 .. 7 on each axis), -1 unless all 8 weights are > 0
__device__ int mc_case(const McLds& L, int x, int y, int z)
{
    int cs = 0;
    for (int n = 0; n < 8; ++n) {
        const int q = nbi(x + (n & 1), y + ((n >> 1) & 1), z + (n >> 2));
        if (!L.ok[q]) return -1;
        if (L.t[q] < 0.f) cs |= 1 << n;
    }
    return cs;
}

__device__ __forceinline__ void other_axes(int a, int& b, int& c) { b = a == 0 ? 1 : 0; c = a == 2 ? 1 : 2; }

// bits a = 0..2: the edge (p, p + e_a) carries a vertex (it crosses and one of the <= 4 cells around it is emitted)
__device__ int mc_edge_mask(const McLds& L, int px, int py, int pz)
{
    const int q0 = nbi(px, py, pz);
    int mask = 0;
    for (int a = 0; a < 3; ++a) {
        int e[3] = {0, 0, 0}; e[a] = 1;
        const int q1 = nbi(px + e[0], py + e[1], pz + e[2]);
        if (!L.ok[q0] || !L.ok[q1] || ((L.t[q0] < 0.f) == (L.t[q1] < 0.f))) continue;
        int b, c; other_axes(a, b, c);
        for (int k = 0; k < 4; ++k) {
            int m[3] = {px, py, pz}; m[b] -= k & 1; m[c] -= k >> 1;
            if (mc_case(L, m[0], m[1], m[2]) >= 0) { mask |= 1 << a; break; }
        }
    }
    return mask;
}

struct McGeom { int gx, gy, gz; float vl; };          // global voxel coordinates of LDS voxel (0, 0, 0), voxel length

// vertex of the cell-edge `e` of the cell with min corner m (LDS coordinates): position and interpolation parameter
__device__ void mc_edge_point(const McLds& L, const McGeom& G, int mx, int my, int mz, int e, float pos[3], float& t, int& q0, int& q1)
{
    const int a = e >> 2, k = e & 3;
    int b, c; other_axes(a, b, c);
    int o[3] = {mx, my, mz}; o[b] += k & 1; o[c] += k >> 1;
    int o1[3] = {o[0], o[1], o[2]}; o1[a] += 1;
    q0 = nbi(o[0], o[1], o[2]); q1 = nbi(o1[0], o1[1], o1[2]);
    const float f0 = L.t[q0], f1 = L.t[q1];
    t = f0 / (f0 - f1);
    const int g[3] = {G.gx, G.gy, G.gz};
    for (int r = 0; r < 3; ++r) {
        const float x0 = ((float)(g[r] + o[r]) + 0.5f) * G.vl, x1 = ((float)(g[r] + o1[r]) + 0.5f) * G.vl;
        pos[r] = x0 + t * (x1 - x0);
    }
}

__global__ void __launch_bounds__(TVOX) tsdf_mc_count_kernel(ibgs_tsdf_volume vol, ibgs_tsdf_mesh_scratch sc)
{
    __shared__ McLds L;
    const int tid = threadIdx.x, px = tid & 7, py = (tid >> 3) & 7, pz = tid >> 6;
    const uint32_t N = min(vol.state[IBGS_TSDF_ALLOCATED], (uint32_t)vol.capacity);
    for (uint32_t r = blockIdx.x; r < N; r += gridDim.x) {
        const int id = (int)sc.order[r];
        if (tid == 0) sc.rank[id] = (int)r;
        int bx, by, bz;
        tsdf_unpack(vol.block_key[id], bx, by, bz);
        mc_load(vol, L, id, bx, by, bz, false);
        const int emask = mc_edge_mask(L, px, py, pz);
        const int cs = mc_case(L, px, py, pz);
        int vtot, ftot;
        const int vex = block_exclusive_scan<TVOX>((int)__popc(emask), &vtot, L.wsum[0]);
        (void)block_exclusive_scan<TVOX>(cs >= 0 ? tsdf_tri_count(cs) : 0, &ftot, L.wsum[1]);
        sc.vinfo[(size_t)id * TVOX + tid] = (uint16_t)(emask | (vex << 3));
        if (tid == 0) { sc.vcount[r] = vtot; sc.fcount[r] = ftot; }
        __syncthreads();          // LDS reused by the next block
    }
}

constexpr int SC_PER = 4;          // counts per thread per round of the scan

__global__ void __launch_bounds__(TVOX) tsdf_mc_scan_kernel(ibgs_tsdf_volume vol, ibgs_tsdf_mesh_scratch sc)
{
    __shared__ McLds L;          // (only wsum)
    const int tid = threadIdx.x;
    const uint32_t N = min(vol.state[IBGS_TSDF_ALLOCATED], (uint32_t)vol.capacity);
    int carry_v = 0, carry_f = 0;
    for (uint32_t base = 0; base < N; base += TVOX * SC_PER) {
        int v[SC_PER], f[SC_PER], sv = 0, sf = 0;
        for (int q = 0; q < SC_PER; ++q) {
            const uint32_t r = base + tid * SC_PER + q;
            v[q] = r < N ? sc.vcount[r] : 0; f[q] = r < N ? sc.fcount[r] : 0;
            sv += v[q]; sf += f[q];
        }
        int tv, tf;
        int ov = block_exclusive_scan<TVOX>(sv, &tv, L.wsum[0]) + carry_v, of = block_exclusive_scan<TVOX>(sf, &tf, L.wsum[1]) + carry_f;
        for (int q = 0; q < SC_PER; ++q) {
            const uint32_t r = base + tid * SC_PER + q;
            if (r < N) { sc.vcount[r] = ov; sc.fcount[r] = of; }
            ov += v[q]; of += f[q];
        }
        carry_v += tv; carry_f += tf;
        __syncthreads();
    }
    if (tid == 0) {
        sc.vcount[N] = carry_v; sc.fcount[N] = carry_f;
        vol.state[IBGS_TSDF_VERTICES] = (uint32_t)carry_v; vol.state[IBGS_TSDF_FACES] = (uint32_t)carry_f;
    }
}

__global__ void __launch_bounds__(TVOX) tsdf_mc_emit_kernel(ibgs_tsdf_volume vol, ibgs_tsdf_mesh_scratch sc, int V, int F, float* __restrict__ vert,
                                                            float* __restrict__ nrm, float* __restrict__ col, int32_t* __restrict__ faces)
{
    __shared__ McLds L;
    const int tid = threadIdx.x, px = tid & 7, py = (tid >> 3) & 7, pz = tid >> 6;
    const uint32_t N = min(vol.state[IBGS_TSDF_ALLOCATED], (uint32_t)vol.capacity);
    for (uint32_t r = blockIdx.x; r < N; r += gridDim.x) {
        const int id = (int)sc.order[r];
        int bx, by, bz;
        tsdf_unpack(vol.block_key[id], bx, by, bz);
        mc_load(vol, L, id, bx, by, bz, true);
        const McGeom G = {bx * TB, by * TB, bz * TB, vol.voxel_length};
        const int emask = mc_edge_mask(L, px, py, pz);
        const int cs = mc_case(L, px, py, pz);
        const int nf = cs >= 0 ? tsdf_tri_count(cs) : 0;
        int vtot, ftot;
        int vi = sc.vcount[r] + block_exclusive_scan<TVOX>((int)__popc(emask), &vtot, L.wsum[0]);
        int fi = sc.fcount[r] + block_exclusive_scan<TVOX>(nf, &ftot, L.wsum[1]);
        for (int a = 0; a < 3; ++a) {
            if (!(emask >> a & 1)) continue;
            const int e = 4 * a;          // the edge owned by p is edge 4 a of the cell whose min corner is p
            float pos[3], t;
            int q0, q1;
            mc_edge_point(L, G, px, py, pz, e, pos, t, q0, q1);
            float n[3] = {0.f, 0.f, 0.f};
            int b, c; other_axes(a, b, c);
            for (int k = 0; k < 4; ++k) {          // the cells around the edge, in the order k = ob | oc << 1
                int m[3] = {px, py, pz}; m[b] -= k & 1; m[c] -= k >> 1;
                const int mcs = mc_case(L, m[0], m[1], m[2]);
                if (mcs < 0) continue;
                const int me = 4 * a + k;          // the same edge as seen from that cell
                for (int tr = 0; tr < 5; ++tr) {
                    const int e0 = TSDF_MC_TRI[mcs][3 * tr], e1 = TSDF_MC_TRI[mcs][3 * tr + 1], e2 = TSDF_MC_TRI[mcs][3 * tr + 2];
                    if (e0 < 0) break;
                    if (e0 != me && e1 != me && e2 != me) continue;
                    float p0[3], p1[3], p2[3], tt;
                    int r0, r1;
                    mc_edge_point(L, G, m[0], m[1], m[2], e0, p0, tt, r0, r1);
                    mc_edge_point(L, G, m[0], m[1], m[2], e1, p1, tt, r0, r1);
                    mc_edge_point(L, G, m[0], m[1], m[2], e2, p2, tt, r0, r1);
                    const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
                    const float wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
                    n[0] = n[0] + (uy * wz - uz * wy);
                    n[1] = n[1] + (uz * wx - ux * wz);
                    n[2] = n[2] + (ux * wy - uy * wx);
                }
            }
            const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            if (len > 0.f) { n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len; }
            if (vi >= 0 && vi < V) {
                const size_t o = (size_t)vi * 3;
                for (int q = 0; q < 3; ++q) {
                    vert[o + q] = pos[q];
                    nrm[o + q] = n[q];
                    col[o + q] = L.c[q][q0] + t * (L.c[q][q1] - L.c[q][q0]);
                }
            } else {
                atomicAdd(&vol.state[IBGS_TSDF_OVERRUN], 1u);
            }
            ++vi;
        }
        for (int tr = 0; tr < nf; ++tr, ++fi) {
            int32_t idx[3];
            for (int m = 0; m < 3; ++m) {
                const int e = TSDF_MC_TRI[cs][3 * tr + m], a = e >> 2, k = e & 3;
                int b, c; other_axes(a, b, c);
                int q[3] = {px, py, pz}; q[b] += k & 1; q[c] += k >> 1;          // the edge's owner voxel (0 .. 8 on each axis)
                const int ox = q[0] >> 3, oy = q[1] >> 3, oz = q[2] >> 3;
                const int nid = L.nb[(ox + 1) + 3 * (oy + 1) + 9 * (oz + 1)];
                idx[m] = -1;
                if (nid >= 0) {
                    const uint16_t info = sc.vinfo[(size_t)nid * TVOX + (q[0] & 7) + TB * (q[1] & 7) + TB * TB * (q[2] & 7)];
                    if (info >> a & 1)
                        idx[m] = sc.vcount[sc.rank[nid]] + (info >> 3) + __popc(info & 7u & ((1u << a) - 1u));
                }
            }
            if (fi >= 0 && fi < F && idx[0] >= 0 && idx[1] >= 0 && idx[2] >= 0 && idx[0] < V && idx[1] < V && idx[2] < V) {
                faces[(size_t)fi * 3] = idx[0]; faces[(size_t)fi * 3 + 1] = idx[1]; faces[(size_t)fi * 3 + 2] = idx[2];
            } else {
                atomicAdd(&vol.state[IBGS_TSDF_OVERRUN], 1u);
            }
        }
        __syncthreads();          // LDS reused by the next block
    }
}

static bool tsdf_volume_ok(const ibgs_tsdf_volume* v)
{
    if (!v) { set_error("tsdf: null volume"); return false; }
    if (!(v->voxel_length > 0.f) || !(v->sdf_trunc > 0.f) || !std::isfinite(v->voxel_length) || !std::isfinite(v->sdf_trunc)) {
        set_error("tsdf: voxel_length and sdf_trunc must be finite and > 0"); return false;
    }
    if (v->capacity <= 0 || v->slot_bits < 1 || v->slot_bits > 30 || (int64_t(1) << v->slot_bits) < v->capacity) {
        set_error("tsdf: capacity %d / slot_bits %d", v->capacity, v->slot_bits); return false;
    }
    if (!v->slot_key || !v->slot_block || !v->slot_mark || !v->active || !v->block_key || !v->tsdf || !v->weight || !v->color || !v->state) {
        set_error("tsdf: null volume array"); return false;
    }
    return true;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_tsdf_sizeof_volume(void) { return sizeof(ibgs_tsdf_volume); }
size_t ibgs_tsdf_sizeof_view(void) { return sizeof(ibgs_tsdf_view); }
size_t ibgs_tsdf_sizeof_mesh_scratch(void) { return sizeof(ibgs_tsdf_mesh_scratch); }

int32_t ibgs_tsdf_mc_table(int32_t* host_out)
{
    if (!host_out) { set_error("tsdf_mc_table: null output"); return -IBGS_ERR_INVALID; }
    for (int c = 0; c < 256; ++c)
        for (int j = 0; j < 16; ++j) host_out[c * 16 + j] = TSDF_MC_TRI[c][j];
    return 0;
}

int32_t ibgs_tsdf_integrate(void* stream, const ibgs_tsdf_volume* vol, const ibgs_tsdf_view* view, const float* depth, const float* color, uint32_t flags)
{
    if (!tsdf_volume_ok(vol)) return -IBGS_ERR_INVALID;
    if (!view || !depth || view->W <= 0 || view->H <= 0 || !(view->fx != 0.f) || !(view->fy != 0.f) || !std::isfinite(view->fx) || !std::isfinite(view->fy)
        || !std::isfinite(view->cx) || !std::isfinite(view->cy) || std::isnan(view->depth_trunc)) {
        set_error("tsdf_integrate: bad view (sizes, intrinsics) or null depth"); return -IBGS_ERR_INVALID;
    }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(view->world_to_camera[i]) || !std::isfinite(view->camera_to_world[i])) { set_error("tsdf_integrate: non-finite pose"); return -IBGS_ERR_INVALID; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IBGS_HIP(hipMemsetAsync(vol->state + IBGS_TSDF_ACTIVE, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(tsdf_alloc_kernel, dim3((view->W + AL_TW - 1) / AL_TW, (view->H + AL_TH - 1) / AL_TH), dim3(AL_THREADS), 0, s, *vol, *view, depth,
                       (flags & IBGS_TSDF_FLAG_NO_DEDUP) ? 0 : 1);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(IG_GRID), dim3(TVOX), 0, s, *vol, *view, depth, color);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_tsdf_mesh_count(void* stream, const ibgs_tsdf_volume* vol, const ibgs_tsdf_mesh_scratch* sc)
{
    if (!tsdf_volume_ok(vol)) return -IBGS_ERR_INVALID;
    if (!sc || !sc->order || !sc->rank || !sc->vinfo || !sc->vcount || !sc->fcount) { set_error("tsdf_mesh_count: null scratch array"); return -IBGS_ERR_INVALID; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tsdf_mc_count_kernel, dim3(MC_GRID), dim3(TVOX), 0, s, *vol, *sc);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(tsdf_mc_scan_kernel, dim3(1), dim3(TVOX), 0, s, *vol, *sc);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_tsdf_mesh_emit(void* stream, const ibgs_tsdf_volume* vol, const ibgs_tsdf_mesh_scratch* sc, int32_t V, int32_t F,
                            float* vertices, float* normals, float* colors, int32_t* faces)
{
    if (!tsdf_volume_ok(vol)) return -IBGS_ERR_INVALID;
    if (!sc || !sc->order || !sc->rank || !sc->vinfo || !sc->vcount || !sc->fcount) { set_error("tsdf_mesh_emit: null scratch array"); return -IBGS_ERR_INVALID; }
    if (V < 0 || F < 0 || (V > 0 && (!vertices || !normals || !colors)) || (F > 0 && !faces)) { set_error("tsdf_mesh_emit: bad V / F or null output"); return -IBGS_ERR_INVALID; }
    if (V == 0 && F == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tsdf_mc_emit_kernel, dim3(MC_GRID), dim3(TVOX), 0, s, *vol, *sc, V, F, vertices, normals, colors, faces);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
