// The 16 x 16-tile implicit GEMM on v_mfma_f32_16x16x4_f32, stated once for the three kernels that run it: hg_conv3_kernel (hourglass.hip), hgb_conv_kernel
// (hgtrain.hip) and lpips_conv3_kernel (lpips.hip); and the rule by which a layer reads its source (plain, the 2 x 2 maximum, the nearest upsample), which
// hgb_wgrad_kernel (hgtrain.hip), hgh_conv3_kernel (hghalf.hip) and the kernels of hghtrain.hip follow too.  Device code and constants only.  A kernel keeps what is its own: its chunk
// loop with the two barriers, its loads of a chunk, its table of tap offsets and the k-steps that read it, its epilogue.
//
// THE TILE  256 threads = 4 waves per 16 x 16 output tile; a wave owns four rows of it and MT result tiles of 16 output channels.  Output channels are M, 16
// pixels of one row N, K runs over k = TAPS (input channel) + tap, four consecutive k per instruction.  LANE MAP: lane l = (col = l & 15, kq = l >> 4) holds
// A[row col][k = kq] and B[k = kq][column col]; register r of result tile mt is channel 16 mt + 4 kq + r of pixel col.  The helpers take wave, col and kq
// from the kernel, which derives them once.
// THE STAGED CHUNK  per input channel the window of the tile and its halo (18 x 18 for 3 x 3 taps), CT_PLANE floats apart (= 16 mod 32), and the weights
// k-major, WROW = padded Cout + 1 floats per k: the lanes of a half-wave read disjoint banks but for one.
// THE STAGING DISCIPLINE (tests/test_gpu_dirty_buffers.py)  coordinates are clamped INTO the frame before an offset is formed, every
// load is unconditional and from a valid address (so the loads of a chunk are all in flight together), and what lies outside the frame or past the last
// channel is replaced by zero afterwards.
// ibgs_amd/_build.py lists this header under the five units (UNIT_HEADERS) and no other; conv_tile_f16.h, next to this file, is the f16 tile of the two half units.
#pragma once
#include "../common.h"

namespace ibgs {

typedef float ct_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) float ct_lds;          // a float in LDS: what the helpers below take the staged chunk as (a generic pointer costs registers)

constexpr int CT_TILE = 16;                          // side of a workgroup's output tile
constexpr int CT_THREADS = 256;
constexpr int CT_WAVES = CT_THREADS / 64;
constexpr int CT_ROWS = CT_TILE / CT_WAVES;          // rows of the tile per wave
constexpr int CT_WIN = CT_TILE + 2;                  // the staged window of a 3 x 3 layer: tile and halo
constexpr int CT_PLANE = 336;                        // floats per staged channel (18 x 18 = 324, padded to 16 mod 32)
constexpr int CT_NPOS = (CT_WIN * CT_WIN + CT_THREADS - 1) / CT_THREADS;          // window positions per thread
static_assert(CT_ROWS == 4 && CT_WIN * CT_WIN <= CT_PLANE && CT_PLANE % 32 == 16, "the lane maps and the bank argument above");

enum { CT_PLAIN = 0, CT_POOL = 1, CT_UP = 2 };          // how a layer reads its (first) input: a kernel's MODE

__device__ __forceinline__ ct_f32x4 ct_mfma(float a, float b, ct_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The source of output position (y, x) of an h x w frame, as an offset into a plane of hs x ws: (h, w) itself (plain), >= (2 h, 2 w) (pool: the first of the
// four of the 2 x 2 maximum; an odd last row or column is never read) or (h / 2, w / 2) (up).  (y, x) may lie outside the frame (a halo): it is clamped into
// it first, so the offset is always a valid one.
template <int MODE>
__device__ __forceinline__ int ct_source_offset(int y, int x, int h, int w, int hs, int ws)
{
    const int yc = min(max(y, 0), h - 1), xc = min(max(x, 0), w - 1);
    if (MODE == CT_PLAIN) return yc * ws + xc;
    if (MODE == CT_POOL) return 2 * yc * ws + 2 * xc;          // 2 yc + 1 <= 2 h - 1 <= hs - 1, and the columns alike
    return min(yc * hs / h, hs - 1) * ws + min(xc * ws / w, ws - 1);          // (yc hs < 2^26)
}
// the value at q = plane + ct_source_offset<MODE>(..)
template <int MODE>
__device__ __forceinline__ float ct_read(const float* q, int ws)
{
    float v = q[0];
    if (MODE == CT_POOL) v = fmaxf(fmaxf(v, q[1]), fmaxf(q[ws], q[ws + 1]));
    return v;
}

// the accumulator tiles started from the bias of COUT channels; a null bias and the channels past COUT give 0
template <int COUT, int MT>
__device__ __forceinline__ void ct_start(ct_f32x4 (&acc)[MT][CT_ROWS], const float* bias, int kq)
{
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        ct_f32x4 start;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = mt * 16 + kq * 4 + r;
            start[r] = (bias && ch < COUT) ? bias[min(ch, COUT - 1)] : 0.0f;
        }
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt) acc[mt][nt] = start;
    }
}

// What a thread stages of an 18 x 18 window does not depend on the chunk: positions tid and tid + 256 (of 324) of each of the chunk's channels.  pos_off: the
// position's ct_source_offset; pos_lds: its place in a staged plane, or -1 for none; pos_in: whether it lies in the frame.
template <int MODE>
__device__ __forceinline__ void ct_window_positions(int (&pos_off)[CT_NPOS], int (&pos_lds)[CT_NPOS], bool (&pos_in)[CT_NPOS], int tx0, int ty0, int h, int w, int hs,
                                                    int ws)
{
#pragma unroll
    for (int r = 0; r < CT_NPOS; ++r) {
        const int p = (int)threadIdx.x + r * CT_THREADS, pc = p < CT_WIN * CT_WIN ? p : 0;
        const int yy = pc / CT_WIN, xx = pc - yy * CT_WIN, y = ty0 + yy - 1, x = tx0 + xx - 1;
        pos_in[r] = p < CT_WIN * CT_WIN && y >= 0 && y < h && x >= 0 && x < w;
        pos_lds[r] = p < CT_WIN * CT_WIN ? p : -1;
        pos_off[r] = ct_source_offset<MODE>(y, x, h, w, hs, ws);
    }
}

// a chunk's window values, as ct_window_positions dealt them, into LDS
template <int CHUNK_C>
__device__ __forceinline__ void ct_store_window(ct_lds* s_in, const float (&iv)[CHUNK_C][CT_NPOS], const int (&pos_lds)[CT_NPOS])
{
#pragma unroll
    for (int cl = 0; cl < CHUNK_C; ++cl)
#pragma unroll
        for (int r = 0; r < CT_NPOS; ++r)
            if (pos_lds[r] >= 0) s_in[cl * CT_PLANE + pos_lds[r]] = iv[cl][r];
}
// A chunk's weights into LDS, k-major (the instruction's A layout).  Element n of a thread is i = tid + 256 n of COUTP runs of RUN consecutive k (an output
// channel's row of the nn.Conv2d layout): m = i / RUN, k = i - m RUN.
template <int COUTP, int RUN, int WROW, int NW>
__device__ __forceinline__ void ct_store_weights(ct_lds* s_w, const float (&wv)[NW])
{
#pragma unroll
    for (int n = 0; n < NW; ++n) {
        const int i = (int)threadIdx.x + n * CT_THREADS, m = i / RUN, j = i - m * RUN;
        if (NW * CT_THREADS == COUTP * RUN || i < COUTP * RUN) s_w[j * WROW + m] = wv[n];          // (a guard only where the last round is partial)
    }
}

// f(ch, y, x, value) for every element this lane holds of the workgroup's output tile (in or outside the frame, below or past Cout: f decides).  f captures
// by value: with captures by reference lpips_conv3_kernel grows by a fifth (the stores' addresses are no longer formed from one base).
template <int MT, typename F>
__device__ __forceinline__ void ct_for_each_output(const ct_f32x4 (&acc)[MT][CT_ROWS], int tx0, int ty0, int wave, int col, int kq, F f)
{
    const int x = tx0 + col;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt) {
            const int y = ty0 + wave * CT_ROWS + nt;
#pragma unroll
            for (int r = 0; r < 4; ++r) f(mt * 16 + kq * 4 + r, y, x, acc[mt][nt][r]);
        }
}

}  // namespace ibgs
