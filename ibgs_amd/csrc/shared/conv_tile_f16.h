// The 16 x 16-tile implicit GEMM on v_mfma_f32_16x16x32_f16, stated once for the two half-precision hourglass units: hgh_conv3_kernel (hghalf.hip, the
// forward) and hght_conv3_kernel (hghtrain.hip, the backward, whose head runs the forward's last launch again); the read of an octet as a layer's MODE says,
// which hght_wgrad_kernel follows too; and the order of an operand fragment's elements, which both packing kernels lay the weights out in.  Device code and
// constants only.  The tile (CT_TILE, CT_THREADS, CT_ROWS, CT_WIN), ct_f32x4, the MODE enum and ct_source_offset are conv_tile.h's.  A kernel keeps what is
// its own: its launch bounds, how its accumulators start, its epilogue.
//
// THE PRODUCTS  Output channels are M (38 -> 48, 19 -> 32, 9 -> 16), 16 pixels of one row are N.  LANE MAP: lane l = (col = l & 15, kq = l >> 4) holds
// A[row col][k = 8 kq + j] and B[k = 8 kq + j][column col], j = 0 .. 7; register r of result tile mt is channel 16 mt + 4 kq + r of pixel col.
// A STAGE IN MEMORY is pixel-major binary16 with the channels innermost, padded with zeros to a multiple of 8 ("octets": 38 -> 5, 19 -> 3, 9 -> 2), so a lane's
// eight k are ONE 16-byte read.  The k order: the input [a | b] is a row of octets, taken four at a time (a CHUNK, 32 channels); inside a chunk one k-step
// is one tap, and kq is the octet.
// THE STAGED CHUNK  the 18 x 18 window of four octets, 80 bytes per pixel in LDS (an odd number of 16-byte units, so the sixteen pixels of a quarter-wave
// read disjoint banks), and the chunk's weights, copied as they lie in the arena: fragment (tap, M tile, lane), which a wave reads back as consecutive 16
// bytes per lane.  The loads of chunk c + 1 are issued before the products of chunk c.
// THE STAGING DISCIPLINE is conv_tile.h's: coordinates are clamped INTO the frame before an offset is formed, every load is unconditional and from a valid
// address, and zeros are selected afterwards for what lies outside the frame or past the last octet.  The arena may hold anything before the call.
// AN ACCUMULATOR TILE AS AN OPERAND  a row of result tiles, rounded, is the next product's B operand as it stands: k-step s takes the M tiles 2 s and 2 s + 1,
// element j of a lane being channel cth_acc_channel(s, kq, j), and the packing kernels lay a 1 x 1 layer's weights out in that order.
// ibgs_amd/_build.py lists this header under hghalf and hghtrain (UNIT_HEADERS) and no other unit.
#pragma once
#include "conv_tile.h"
#include "hg_net.h"

namespace ibgs {

typedef _Float16 cth_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 cth_h4 __attribute__((ext_vector_type(4)));

constexpr int CTH_NPIX = CT_WIN * CT_WIN;
constexpr int CTH_PSTRIDE = 5;                       // 16-byte units per staged pixel: four octets and one of padding (odd)
constexpr int CTH_XO = (HG_C + 7) / 8;               // octets of x
static_assert(CT_ROWS == 4 && CTH_PSTRIDE % 2 == 1 && CT_THREADS % 4 == 0, "the lane maps and the bank argument above");

constexpr int cth_octets(int c) { return (c + 7) / 8; }
// fragments (eight binary16 each) of a packed 3 x 3 layer of `octets` of input and `rows` of output: chunks x 9 taps x M tiles x 64 lanes
constexpr int cth_frags3(int octets, int rows) { return ((octets + 3) / 4) * 9 * ((rows + 15) / 16) * 64; }
constexpr int CTH_FUSE_STEPS = 2 + (CTH_XO + 3) / 4;          // k-steps of fuse_input (d1: 2, x: 2)

__device__ __forceinline__ ct_f32x4 cth_mfma(cth_h8 a, cth_h8 b, ct_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float cth_round(float v) { return (float)(_Float16)v; }          // to binary16, to nearest even, and back

// ---- the order of a fragment's elements (the packing kernels) ----------------------------------------------------------------------------------------------
// element j of octet o of a 3 x 3 layer's input [ca | cb]: its channel along Cin, or -1 for padding
__device__ __forceinline__ int cth_frag3_channel(int o, int j, int ca, int cb)
{
    const int noa = cth_octets(ca), nob = cth_octets(cb);
    if (o < noa) return 8 * o + j < ca ? 8 * o + j : -1;
    if (o < noa + nob) return 8 * (o - noa) + j < cb ? ca + 8 * (o - noa) + j : -1;
    return -1;
}
// element j of a lane of k-step s where the B operand is a row of accumulator tiles: the channel that tile holds there
__device__ __forceinline__ int cth_acc_channel(int s, int kq, int j) { return (2 * s + (j >> 2)) * 16 + 4 * kq + (j & 3); }
// the same of a 1 x 1 layer on [accumulator tiles of ca channels (k-steps 0, 1) | octets of cb channels (k-steps 2 ..)]
__device__ __forceinline__ int cth_frag1_channel(int s, int kq, int j, int ca, int cb)
{
    if (s < 2) return cth_acc_channel(s, kq, j) < ca ? cth_acc_channel(s, kq, j) : -1;
    const int ch = 8 * (4 * (s - 2) + kq) + j;
    return ch < cb ? ca + ch : -1;
}

// ---- the read of an octet ------------------------------------------------------------------------------------------------------------------------------
// The octet at q = stage + (size_t)ct_source_offset<MODE>(..) * cp + 8 * octet, cp binary16 per pixel of a stage ws pixels wide: itself, or the maximum of
// its 2 x 2 window (CT_POOL); zeros where `in` is false.
template <int MODE>
__device__ __forceinline__ cth_h8 cth_read(const _Float16* q, size_t cp, int ws, bool in)
{
    cth_h8 v = *reinterpret_cast<const cth_h8*>(q);
    if (MODE == CT_POOL) {
        const cth_h8 v1 = *reinterpret_cast<const cth_h8*>(q + cp), v2 = *reinterpret_cast<const cth_h8*>(q + (size_t)ws * cp),
                     v3 = *reinterpret_cast<const cth_h8*>(q + ((size_t)ws + 1) * cp);
        v = __builtin_elementwise_max(__builtin_elementwise_max(v, v1), __builtin_elementwise_max(v2, v3));
    }
    const cth_h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    return in ? v : zero;
}

// ---- the convolution -------------------------------------------------------------------------------------------------------------------------------------
// the accumulator tiles started from the rounded bias of COUT channels; the channels past COUT give 0
template <int COUT, int MT>
__device__ __forceinline__ void cth_start(ct_f32x4 (&acc)[MT][CT_ROWS], const float* bias, int kq)
{
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        ct_f32x4 start;
#pragma unroll
        for (int r = 0; r < 4; ++r) start[r] = mt * 16 + kq * 4 + r < COUT ? cth_round(bias[mt * 16 + kq * 4 + r]) : 0.0f;
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt) acc[mt][nt] = start;
    }
}

// acc += the 3 x 3 convolution of [a | b] (CA and CB channels; a holds hs x ws pixels and is read as MODE says, b h x w and plain) with the packed weights
// wfrag, on this workgroup's tile of the h x w output.  Every thread of the workgroup calls it (it holds the barriers).
template <int CA, int CB, int COUT, int MODE>
__device__ __forceinline__ void cth_conv3(ct_f32x4 (&acc)[(COUT + 15) / 16][CT_ROWS], const _Float16* a, const _Float16* b, const cth_h8* wfrag, int h, int w, int hs, int ws)
{
    constexpr int NOA = cth_octets(CA), NOB = cth_octets(CB), NO = NOA + NOB, NC = (NO + 3) / 4, MT = (COUT + 15) / 16;
    constexpr int NWF = 9 * MT * 64;          // weight fragments of a chunk
    constexpr int NPOS = (CTH_NPIX * 4 + CT_THREADS - 1) / CT_THREADS, NW = (NWF + CT_THREADS - 1) / CT_THREADS;
    static_assert(CB == 0 || MODE == CT_PLAIN, "a second input is read plain, at the first one's resolution");
    __shared__ cth_h8 s_in[CTH_NPIX * CTH_PSTRIDE];
    __shared__ cth_h8 s_w[NWF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int tx0 = blockIdx.x * CT_TILE, ty0 = blockIdx.y * CT_TILE;

    // What a thread stages does not depend on the chunk but for the octet: octet tid & 3 of the window pixels (tid >> 2) + 64 r, and NW weight fragments.  A
    // pixel's index into a stage is formed once, from coordinates clamped INTO the frame.
    const int o4 = tid & 3;
    int pos[NPOS];          // pixel index into a (and into b: read plain at the same resolution)
    bool pos_in[NPOS];
#pragma unroll
    for (int r = 0; r < NPOS; ++r) {
        const int p = (tid >> 2) + r * (CT_THREADS / 4), pc = p < CTH_NPIX ? p : 0;
        const int yy = pc / CT_WIN, xx = pc - yy * CT_WIN, y = ty0 + yy - 1, x = tx0 + xx - 1;
        pos_in[r] = p < CTH_NPIX && y >= 0 && y < h && x >= 0 && x < w;
        pos[r] = ct_source_offset<MODE>(y, x, h, w, hs, ws);
    }
    cth_h8 iv[NPOS], wv[NW];
    auto load_chunk = [&](const int c) {
        const int oc = 4 * c + o4, occ = oc < NO ? oc : NO - 1;          // this thread's octet of [a | b], clamped to the last one
        const bool from_a = CB == 0 || occ < NOA;
        const _Float16* const base = from_a ? a + occ * 8 : b + (occ - NOA) * 8;
        const size_t cp = from_a ? NOA * 8 : NOB * 8;          // binary16 per pixel of that input
#pragma unroll
        for (int r = 0; r < NPOS; ++r) iv[r] = cth_read<MODE>(base + (size_t)pos[r] * cp, cp, ws, oc < NO && pos_in[r]);
#pragma unroll
        for (int n = 0; n < NW; ++n) wv[n] = wfrag[c * NWF + min(tid + n * CT_THREADS, NWF - 1)];
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int r = 0; r < NPOS; ++r) {
            const int p = (tid >> 2) + r * (CT_THREADS / 4);
            if (p < CTH_NPIX) s_in[p * CTH_PSTRIDE + o4] = iv[r];
        }
#pragma unroll
        for (int n = 0; n < NW; ++n)
            if (tid + n * CT_THREADS < NWF) s_w[tid + n * CT_THREADS] = wv[n];
    };
    const int window_at = (wave * CT_ROWS * CT_WIN + col) * CTH_PSTRIDE + kq;
    auto run_taps = [&]() {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            cth_h8 av[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = s_w[(t * MT + mt) * 64 + lane];
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) {
                const cth_h8 bv = s_in[window_at + ((nt + t / 3) * CT_WIN + t % 3) * CTH_PSTRIDE];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = cth_mfma(av[mt], bv, acc[mt][nt]);
            }
        }
    };
    load_chunk(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) {          // (uniform over the workgroup: every thread reaches the barriers)
        __syncthreads();          // the chunk before has been read
        store_chunk();
        __syncthreads();
        if (c + 1 < NC) load_chunk(c + 1);          // in flight during this chunk's products
        run_taps();
    }
}

// ---- the head: an accumulator tile as the next product's operand, and fuse_input ---------------------------------------------------------------------------
// M tiles 2 s and 2 s + 1 of a row of accumulator tiles as the B fragment of k-step s, rounded; RELU: clamped at zero first (values that are already clamped
// and rounded pass unchanged either way)
template <int MT, bool RELU>
__device__ __forceinline__ cth_h8 cth_as_operand(const ct_f32x4 (&t)[MT][CT_ROWS], int nt, int s)
{
    cth_h8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int tile = 2 * s + (j >> 2);
        float f = 0.0f;
        if (tile < MT) f = t[tile][nt][j & 3];
        v[j] = (_Float16)(RELU ? (f > 0.0f ? f : 0.0f) : f);
    }
    return v;
}

// f = fuse_input on [d1 | h(x)] before its ReLU and rounding, on this workgroup's tile of the h x w frame: the rounded bias, then the k-steps in the order of
// the packed weights fuse_frag.  d1 is dec1's row of accumulator tiles, padding channels exact zeros; RELU: given before its ReLU and rounding.  xh is h(x),
// pixel-major octets.  The forward's last launch and the backward's head both run THIS: the same k order, the same bits.
template <bool RELU>
__device__ __forceinline__ void cth_fuse_input(ct_f32x4 (&f)[3][CT_ROWS], const ct_f32x4 (&d1)[3][CT_ROWS], const cth_h8* fuse_frag, const float* fuse_b, const _Float16* xh, int h,
                                               int w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int xc = min((int)blockIdx.x * CT_TILE + col, w - 1), ty0 = blockIdx.y * CT_TILE;
    cth_start<HG_C>(f, fuse_b, kq);
#pragma unroll
    for (int s = 0; s < CTH_FUSE_STEPS; ++s) {
        cth_h8 av[3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) av[mt] = fuse_frag[(s * 3 + mt) * 64 + lane];
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt) {
            cth_h8 bv;
            if (s < 2) bv = cth_as_operand<3, RELU>(d1, nt, s);
            else {
                const int o = 4 * (s - 2) + kq, yc = min(ty0 + wave * CT_ROWS + nt, h - 1);
                bv = cth_read<CT_PLAIN>(xh + ((size_t)yc * w + xc) * (CTH_XO * 8) + min(o, CTH_XO - 1) * 8, CTH_XO * 8, w, o < CTH_XO);
            }
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) f[mt][nt] = cth_mfma(av[mt], bv, f[mt][nt]);
        }
    }
}

}  // namespace ibgs
