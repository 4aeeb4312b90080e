// The half-precision backward of the hourglass CNN (C ABI: include/ibgs_hg_half_train.h, which holds the operation line by line; Python:
// ibgs_amd/hourglass.py `hourglass_backward` / `hourglass_train` with precision="float16").  The forward of a training step is ibgs_hgh_forward (hghalf.hip)
// on an arena the caller keeps; this unit reads its h(x) and its six binary16 stages and never writes them.
//
// CONTRACT  A tolerance against a float64 restatement on the device's own decisions, with torch's autocast backward as the yardstick (DESIGN.md section 15,
// "Half-precision training"; tests/hghalf_bwd_ref.py).  The same arguments give the same bits on every call and stream: a weight gradient is one float32
// partial per workgroup, summed by a last pass in the order of the workgroups; the only atomics are INTEGER ones (the maximum of the upstream's magnitude as
// bits, the count of non-finite values, the reduction's ticket), whose results do not depend on their order.
//
// THE PRODUCTS are v_mfma_f32_16x16x32_f16 with the lane map of csrc/shared/conv_tile_f16.h, which states the tile, the chunk loop, the octet read and the
// forward's fuse_input once for this unit and hghalf.hip.  Every tensor between two launches is PIXEL-MAJOR with
// the channels innermost and padded with zeros to a multiple of 8, binary16 (the G_*, d1, f, gS, h(x)) or float32 (an input gradient before its gather).
//   hght_conv3_kernel<CA, CB, COUT, EPI>  cth_conv3, the 3 x 3 implicit GEMM hgh_conv3_kernel runs too, on the 16 x 16 tile (M = COUT rows of the packed weight,
//     N = 16 pixels of a row, K = (octet of [a | b], tap)), the input read plain.  With the weight packed transposed and flipped it is a layer's input gradient from its G;
//     its epilogue stores the float32 accumulation (EPI_F32), masks by a stage, rounds and stores binary16 (EPI_MASK), or adds 2^-k times it to grad_x's planes
//     (EPI_GRADX).  EPI_HEAD is the last launch of the forward again -- dec1 from its rounded bias, then cth_fuse_input on [d1, h(x)]: the definition the forward
//     runs, so the same k order and bits -- followed by the head of the backward in registers: gS, G_f, G_d1 and the head's share of grad_x.
//   hght_wgrad_kernel<CA, CB, COUT, MODE, TAPS>  a GEMM whose K is the pixels, 32 of them per instruction: M = output channels (rows: G), N = 16 input channels
//     of a slice for each tap, and one column of ones (the bias gradient).  A workgroup owns a slice and a strip of 8 x 16 tiles; G and the input window are
//     staged CHANNEL-major in LDS (the window in three copies shifted by one column, so that every operand is one aligned 16-byte read); each wave takes two
//     rows of a tile; the four waves' float32 sums are added in wave order through LDS and written as one partial.  hght_wsum_kernel adds a layer's partials
//     in strip order, in double, and scales by 2^-k.
//   hght_scale_kernel, hght_pack_kernel, hght_unpool_kernel, hght_unup_kernel, hght_status_kernel  the scale, the operand fragments, the routing.
// STAGING keeps the forward's discipline: coordinates are clamped into the frame before an offset is formed, every load is unconditional and from a valid
// address, and what lies outside the frame or past the last octet is replaced by zero afterwards.  The arena may be uninitialised memory.
#include "common.h"
#include "shared/hg_net.h"
#include "shared/conv_tile.h"
#include "shared/conv_tile_f16.h"
#include "../../include/ibgs_hourglass.h"
#include "../../include/ibgs_hg_half.h"
#include "../../include/ibgs_hg_half_train.h"

namespace ibgs {

constexpr int HGHT_WT_H = 8;                         // hght_wgrad_kernel: rows of a tile of its strip
constexpr int HGHT_WT_W = 16;                        // ... and columns
constexpr int HGHT_MAX_STRIPS = 128;                 // strips (partials) per weight gradient, at most
constexpr int HGHT_MIN_STRIP_TILES = 2;              // tiles of a strip, at least
constexpr int HGHT_SLICE = 16;                       // input channels (two octets) of a weight-gradient slice
constexpr int HGHT_GROW = HGHT_WT_H * HGHT_WT_W + 8; // binary16 per staged channel of G (a multiple of 8: operands stay 16-byte aligned)
constexpr int HGHT_E_TARGET = IBGS_HGHT_E_TARGET;
constexpr int HGHT_SCALE_BLOCKS = 256;
static_assert(HGHT_WT_H * HGHT_WT_W == 32 * (CT_THREADS / 64), "the lane maps");

// the control words at the head of the arena
struct HghtCtrl { unsigned m_bits; int k; int nonfinite; unsigned ticket; };

__device__ __forceinline__ bool hght_bad(_Float16 v) { return !(__builtin_fabsf((float)v) <= 65504.0f); }          // inf or NaN
// floor(log2 m) of a positive finite float32 given as bits (subnormals included)
__device__ __forceinline__ int hght_floor_log2(unsigned bits)
{
    const int e = (int)(bits >> 23);
    return e ? e - 127 : (31 - __clz((int)bits)) - 149;
}

// ---- the scale ---------------------------------------------------------------------------------------------------------------------------------------------
// AUTO: the maximum of |g_res + g_ip| as bits (non-negative floats order as their bits; a NaN's bits lie above infinity's); the last workgroup to finish writes k.
__global__ void __launch_bounds__(CT_THREADS) hght_scale_kernel(const float* __restrict__ g_res, const float* __restrict__ g_ip, size_t n, int fixed, int fixed_k,
                                                                HghtCtrl* ctrl)
{
    if (fixed) {
        if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->k = fixed_k;
        return;
    }
    __shared__ unsigned s_max[CT_THREADS / 64];
    unsigned best = 0;
    for (size_t i = (size_t)blockIdx.x * CT_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * CT_THREADS) {
        const float g = (g_res ? g_res[i] : 0.0f) + (g_ip ? g_ip[i] : 0.0f);
        best = max(best, __float_as_uint(g) & 0x7fffffffu);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, d, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        atomicMax(&ctrl->m_bits, best);
        __threadfence();
        if (atomicAdd(&ctrl->ticket, 1u) == gridDim.x - 1) {
            __threadfence();
            const unsigned m = atomicMax(&ctrl->m_bits, 0u);
            ctrl->k = (m == 0u || m >= 0x7f800000u) ? 0 : HGHT_E_TARGET - hght_floor_log2(m);
        }
    }
}

__global__ void hght_status_kernel(const HghtCtrl* ctrl, int* status)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { status[0] = ctrl->k; status[1] = ctrl->nonfinite; }
}

// ---- the packing launch: the operand fragments ----------------------------------------------------------------------------------------
enum { HGHT_P3_FWD, HGHT_P3_T, HGHT_P1_FWD, HGHT_P1_T_ACC, HGHT_P1_T_PLAIN };
struct HghtPackItem {
    const float* w;
    int kind;
    int rows;                  // rows of the operand (M) that are not padding
    int ca, cb;                // channels along K: of the two inputs ([a | b]); for the transposed kinds ca = the layer's output channels, cb = 0
    int wcin, m0;              // transposed kinds: the weight's second dimension, and the first of its input channels this operand holds
    int first;                 // its first fragment
};
constexpr int HGHT_ITEMS = 14;
struct HghtPackArgs {
    cth_h8* packed; int frags;
    HghtPackItem item[HGHT_ITEMS];
};

__global__ void __launch_bounds__(CT_THREADS) hght_pack_kernel(const HghtPackArgs a)
{
    const int i = (int)blockIdx.x * CT_THREADS + (int)threadIdx.x;
    if (i >= a.frags) return;
    HghtPackItem L = a.item[0];
#pragma unroll
    for (int n = 1; n < HGHT_ITEMS; ++n)
        if (i >= a.item[n].first) L = a.item[n];          // (selects: the table is never indexed by a register)
    const int local = i - L.first, lane = local & 63, rest = local >> 6, kq = lane >> 4;
    const int mtn = (L.rows + 15) / 16;
    cth_h8 v;
    if (L.kind == HGHT_P3_FWD || L.kind == HGHT_P3_T) {
        const int mt = rest % mtn, t = (rest / mtn) % 9, c = rest / (mtn * 9), m = mt * 16 + (lane & 15), o = 4 * c + kq;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = cth_frag3_channel(o, j, L.ca, L.cb);
            float f = 0.0f;
            if (m < L.rows && idx >= 0)
                f = L.kind == HGHT_P3_FWD ? L.w[((size_t)m * (L.ca + L.cb) + idx) * 9 + t] : L.w[((size_t)idx * L.wcin + L.m0 + m) * 9 + (8 - t)];
            v[j] = (_Float16)f;
        }
    } else {
        const int mt = rest % mtn, s = rest / mtn, m = mt * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int acc_ch = cth_acc_channel(s, kq, j);
            float f = 0.0f;
            if (L.kind == HGHT_P1_FWD) {
                const int idx = cth_frag1_channel(s, kq, j, L.ca, L.cb);
                if (m < L.rows && idx >= 0) f = L.w[(size_t)m * (L.ca + L.cb) + idx];
            } else if (L.kind == HGHT_P1_T_ACC) {
                if (m < L.rows && acc_ch < L.ca) f = L.w[(size_t)acc_ch * L.wcin + L.m0 + m];
            } else {
                const int ch = 8 * kq + j;
                if (m < L.rows && s == 0 && ch < L.ca) f = L.w[(size_t)ch * L.wcin + L.m0 + m];
            }
            v[j] = (_Float16)f;
        }
    }
    a.packed[i] = v;
}

// ---- the convolution --------------------------------------------------------------------------------------------------------------------------------------
enum { HGHT_EPI_F32, HGHT_EPI_MASK, HGHT_EPI_GRADX, HGHT_EPI_HEAD };
struct HghtConv {
    const _Float16* a; const _Float16* b;          // the two inputs ([a | b] along the channels), pixel-major, at h x w
    const cth_h8* wfrag;
    int h, w;
    HghtCtrl* ctrl;
    float* out32;                                  // EPI_F32: h x w pixels of CPOUT float32
    const _Float16* mask; _Float16* out16;         // EPI_MASK: the stage whose ReLU masks, the rounded result (both CPOUT per pixel)
    float* grad_x;                                 // EPI_GRADX and EPI_HEAD: 38 planes (EPI_HEAD: may be null)
    // EPI_HEAD
    const float* bias; const _Float16* xh; const cth_h8* fuse_frag; const float* fuse_b;
    const cth_h8* finalT_frag; const cth_h8* fuseT_lo; const cth_h8* fuseT_hi;
    const float* g_res; const float* g_ip; float burned;
    _Float16 *d1, *f, *Gf, *Gd1, *gs;
};

// a row of three accumulator tiles (38 channels, padding rows exact zeros) as pixel-major binary16: 40 per pixel
__device__ __forceinline__ void hght_store40(_Float16* out, const ct_f32x4 (&t)[3][CT_ROWS], int nt, size_t p, int kq, bool in)
{
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        const int c0 = mt * 16 + kq * 4;
        if (c0 < 40 && in) {
            cth_h4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (_Float16)t[mt][nt][r];
            *reinterpret_cast<cth_h4*>(out + p * 40 + c0) = v;
        }
    }
}

template <int CA, int CB, int COUT, int EPI>
__global__ void __launch_bounds__(CT_THREADS, EPI == HGHT_EPI_HEAD ? 1 : 2) hght_conv3_kernel(const HghtConv a)
{
    constexpr int MT = (COUT + 15) / 16, CPOUT = 8 * cth_octets(COUT);
    static_assert(EPI != HGHT_EPI_HEAD || (COUT == HG_C && MT == 3), "the head is dec1");
    static_assert(EPI != HGHT_EPI_GRADX || COUT == HG_C, "grad_x has 38 planes");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int tx0 = blockIdx.x * CT_TILE, ty0 = blockIdx.y * CT_TILE;
    const int h = a.h, w = a.w;

    ct_f32x4 acc[MT][CT_ROWS] = {};
    if constexpr (EPI == HGHT_EPI_HEAD) cth_start<COUT>(acc, a.bias, kq);          // only the head is a forward layer
    cth_conv3<CA, CB, COUT, CT_PLAIN>(acc, a.a, a.b, a.wfrag, h, w, h, w);

    const int x = tx0 + col, xc = min(x, w - 1);
    const size_t plane = (size_t)h * (size_t)w;
    const int k = a.ctrl->k;
    int bad = 0;
    if constexpr (EPI == HGHT_EPI_F32 || EPI == HGHT_EPI_MASK) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int c0 = mt * 16 + kq * 4;
            if (c0 < CPOUT) {          // (whole groups of four: CPOUT is a multiple of 8; rows past COUT are exact zeros)
#pragma unroll
                for (int nt = 0; nt < CT_ROWS; ++nt) {
                    const int y = ty0 + wave * CT_ROWS + nt, yc = min(y, h - 1);
                    const size_t at = ((size_t)yc * w + xc) * CPOUT + c0;
                    const bool in = y < h && x < w;
                    if constexpr (EPI == HGHT_EPI_F32) {
                        if (in) *reinterpret_cast<ct_f32x4*>(a.out32 + at) = acc[mt][nt];
                    } else {
                        const cth_h4 m = *reinterpret_cast<const cth_h4*>(a.mask + at);
                        cth_h4 v;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            v[r] = m[r] > (_Float16)0.0f ? (_Float16)acc[mt][nt][r] : (_Float16)0.0f;
                            bad += (in && hght_bad(v[r])) ? 1 : 0;
                        }
                        if (in) *reinterpret_cast<cth_h4*>(a.out16 + at) = v;
                    }
                }
            }
        }
    } else if constexpr (EPI == HGHT_EPI_GRADX) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) {
                const int y = ty0 + wave * CT_ROWS + nt;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = mt * 16 + kq * 4 + r;
                    if (ch < COUT && y < h && x < w) {
                        const size_t at = (size_t)ch * plane + (size_t)y * w + x;
                        a.grad_x[at] += ldexpf(acc[mt][nt][r], -k);
                    }
                }
            }
    } else {
        // acc is d1 before its ReLU and rounding.  d1 and f as the forward forms them (cth_fuse_input is its last launch's too); then the head of the backward.
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[mt][nt][r] = cth_round(acc[mt][nt][r] > 0.0f ? acc[mt][nt][r] : 0.0f);
        ct_f32x4 f[3][CT_ROWS];
        cth_fuse_input<false>(f, acc, a.fuse_frag, a.fuse_b, a.xh, h, w);
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) f[mt][nt][r] = cth_round(f[mt][nt][r] > 0.0f ? f[mt][nt][r] : 0.0f);

        cth_h8 fin_t[3], lo_t[2][3], hi_t[2][3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            fin_t[mt] = a.finalT_frag[mt * 64 + lane];
#pragma unroll
            for (int s = 0; s < 2; ++s) { lo_t[s][mt] = a.fuseT_lo[(s * 3 + mt) * 64 + lane]; hi_t[s][mt] = a.fuseT_hi[(s * 3 + mt) * 64 + lane]; }
        }
        ct_f32x4 gf[3][CT_ROWS];
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt) {
            const int y = ty0 + wave * CT_ROWS + nt, yc = min(y, h - 1);
            const bool in = y < h && x < w;
            const size_t p = (size_t)yc * w + xc;
            hght_store40(a.d1, acc, nt, p, kq, in);
            hght_store40(a.f, f, nt, p, kq, in);
            // gS: the three channels of the scaled upstream, rounded, as rows k = 0 .. 2 of the B operand (lanes kq == 0)
            cth_h8 gv = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float g = (a.g_res ? a.g_res[(size_t)c * plane + p] : 0.0f) + (a.g_ip ? a.g_ip[(size_t)c * plane + p] : 0.0f);
                const _Float16 s = (_Float16)ldexpf(g, k);
                gv[c] = (kq == 0 && in) ? s : (_Float16)0.0f;
                bad += (kq == 0 && in && hght_bad(s)) ? 1 : 0;
            }
            if (kq == 0 && in) *reinterpret_cast<cth_h8*>(a.gs + p * 8) = gv;
            const ct_f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) {
                gf[mt][nt] = cth_mfma(fin_t[mt], gv, z4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const _Float16 v = f[mt][nt][r] > 0.0f ? (_Float16)gf[mt][nt][r] : (_Float16)0.0f;
                    bad += (in && hght_bad(v)) ? 1 : 0;
                    gf[mt][nt][r] = (float)v;
                }
            }
            hght_store40(a.Gf, gf, nt, p, kq, in);
        }
        // g_cat = fuse_input^T G_f: rows 0 .. 37 masked by d1 (G_d1), rows 38 .. 75 the head's share of grad_x
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt) {
            const int y = ty0 + wave * CT_ROWS + nt, yc = min(y, h - 1);
            const bool in = y < h && x < w;
            const size_t p = (size_t)yc * w + xc;
            const cth_h8 b0 = cth_as_operand<3, false>(gf, nt, 0), b1 = cth_as_operand<3, false>(gf, nt, 1);
            const ct_f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) {
                ct_f32x4 lo = cth_mfma(lo_t[1][mt], b1, cth_mfma(lo_t[0][mt], b0, z4));
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const _Float16 v = acc[mt][nt][r] > 0.0f ? (_Float16)lo[r] : (_Float16)0.0f;
                    bad += (in && hght_bad(v)) ? 1 : 0;
                    f[mt][nt][r] = (float)v;          // (f has been stored: its registers carry G_d1 to the store)
                }
            }
            hght_store40(a.Gd1, f, nt, p, kq, in);
            if (a.grad_x) {
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) {
                    const ct_f32x4 hi = cth_mfma(hi_t[1][mt], b1, cth_mfma(hi_t[0][mt], b0, z4));
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = mt * 16 + kq * 4 + r;
                        if (ch < HG_C && in) {
                            float v = ldexpf(hi[r], -k);
                            if (a.g_ip && ch >= HG_C - 3) v = fmaf(a.burned, a.g_ip[(size_t)(ch - (HG_C - 3)) * plane + p], v);
                            a.grad_x[(size_t)ch * plane + p] = v;
                        }
                    }
                }
            }
        }
    }
    if (EPI != HGHT_EPI_F32 && EPI != HGHT_EPI_GRADX && bad) atomicAdd(&a.ctrl->nonfinite, bad);
}

// ---- the weight gradients ----------------------------------------------------------------------------------------------------------------------------------
struct HghtWgrad {
    const _Float16* g;                             // the layer's pre-activation gradient: h x w pixels of 8 octets(COUT)
    const _Float16* a; const _Float16* b;          // the layer's input [a | b]; a holds hs x ws pixels, read as MODE says
    float* partial;                                // (strips, slices, COUT padded, (TAPS + 1) x 16)
    int h, w, hs, ws;
    int tiles_x, ntiles, strip_tiles;
};

template <int CA, int CB, int COUT, int MODE, int TAPS>
__global__ void __launch_bounds__(CT_THREADS, 2) hght_wgrad_kernel(const HghtWgrad a)
{
    constexpr int NOA = cth_octets(CA), NOB = cth_octets(CB), NO = NOA + NOB, NOG = cth_octets(COUT), MT = (COUT + 15) / 16, COUTP = MT * 16;
    constexpr int PAD = TAPS == 9 ? 1 : 0, COPIES = TAPS == 9 ? 3 : 1, WINH = HGHT_WT_H + 2 * PAD, WINW = HGHT_WT_W + 2 * PAD;
    constexpr int ICH = WINH * HGHT_WT_W + 8;          // binary16 per staged channel of one copy (a multiple of 8; 84 or 68 dwords: the sixteen channels of a read fall into disjoint banks)
    constexpr int NTT = TAPS + 1, NCOLS = NTT * 16;
    constexpr int G_HALVES = COUTP * HGHT_GROW, I_HALVES = COPIES * HGHT_SLICE * ICH, RED_FLOATS = 4 * NTT * 256;
    constexpr int BYTES = 2 * (G_HALVES + I_HALVES) > 4 * RED_FLOATS ? 2 * (G_HALVES + I_HALVES) : 4 * RED_FLOATS;
    static_assert(CB == 0 || MODE == CT_PLAIN, "a second input is read plain, at the first one's resolution");
    static_assert(TAPS == 9 || TAPS == 1, "3 x 3 or 1 x 1");
    __shared__ __attribute__((aligned(16))) char s_mem[BYTES];
    _Float16* const s_g = reinterpret_cast<_Float16*>(s_mem);
    _Float16* const s_i = s_g + G_HALVES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int slice = blockIdx.x;
    const int h = a.h, w = a.w;

    for (int i = tid; i < (COUTP - 8 * NOG) * HGHT_GROW; i += CT_THREADS) s_g[8 * NOG * HGHT_GROW + i] = (_Float16)0.0f;          // the rows past the last octet, once

    ct_f32x4 acc[MT][NTT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < NTT; ++t) acc[mt][t] = ct_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    cth_h8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = col == 0 ? (_Float16)1.0f : (_Float16)0.0f;

    const int row = 2 * wave + (kq >> 1), xo = 8 * (kq & 1);          // this lane's eight pixels of the tile: (row, xo .. xo + 7)
    const int first = blockIdx.y * a.strip_tiles, last = min(first + a.strip_tiles, a.ntiles);
    for (int tile = first; tile < last; ++tile) {          // (uniform over the workgroup)
        const int tyi = tile / a.tiles_x, ty0 = tyi * HGHT_WT_H, tx0 = (tile - tyi * a.tiles_x) * HGHT_WT_W;
        __syncthreads();          // the tile before has been read
        for (int i = tid; i < HGHT_WT_H * HGHT_WT_W * NOG; i += CT_THREADS) {
            const int p = i / NOG, o = i - p * NOG, yy = p / HGHT_WT_W, xx = p - yy * HGHT_WT_W, y = ty0 + yy, x = tx0 + xx;
            const cth_h8 v = cth_read<CT_PLAIN>(a.g + ((size_t)min(y, h - 1) * w + min(x, w - 1)) * (8 * NOG) + 8 * o, 8 * NOG, w, y < h && x < w);
#pragma unroll
            for (int j = 0; j < 8; ++j) s_g[(8 * o + j) * HGHT_GROW + p] = v[j];
        }
        for (int i = tid; i < WINH * WINW * 2; i += CT_THREADS) {
            const int p = i >> 1, o2 = i & 1, yy = p / WINW, xx = p - yy * WINW, y = ty0 + yy - PAD, x = tx0 + xx - PAD;
            const int oc = 2 * slice + o2, occ = min(oc, NO - 1);
            const bool from_a = CB == 0 || occ < NOA;
            const bool in = oc < NO && y >= 0 && y < h && x >= 0 && x < w;
            constexpr size_t CPA = 8 * NOA, CPB = 8 * (NOB > 0 ? NOB : 1);          // binary16 per pixel of the two inputs
            const cth_h8 v = from_a ? cth_read<MODE>(a.a + (size_t)ct_source_offset<MODE>(y, x, h, w, a.hs, a.ws) * CPA + 8 * occ, CPA, a.ws, in)
                                    : cth_read<CT_PLAIN>(a.b + (size_t)ct_source_offset<CT_PLAIN>(y, x, h, w, h, w) * CPB + 8 * (occ - NOA), CPB, w, in);
#pragma unroll
            for (int d = 0; d < COPIES; ++d) {          // copy d holds the window shifted by d columns: every tap's eight pixels start at a multiple of 8
                const int xs = xx - d;
                if (xs >= 0 && xs < HGHT_WT_W) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) s_i[(d * HGHT_SLICE + 8 * o2 + j) * ICH + yy * HGHT_WT_W + xs] = v[j];
                }
            }
        }
        __syncthreads();
        cth_h8 av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = *reinterpret_cast<const cth_h8*>(s_g + (mt * 16 + col) * HGHT_GROW + 32 * wave + 8 * kq);
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int dy = TAPS == 9 ? t / 3 : 0, dx = TAPS == 9 ? t % 3 : 0;
            const cth_h8 bv = *reinterpret_cast<const cth_h8*>(s_i + (dx * HGHT_SLICE + col) * ICH + (row + dy) * HGHT_WT_W + xo);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][t] = cth_mfma(av[mt], bv, acc[mt][t]);
        }
        if (slice == 0) {          // (uniform over the workgroup) the bias gradient is read from the first slice's partial
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][TAPS] = cth_mfma(av[mt], ones, acc[mt][TAPS]);
        }
    }
    // the four waves' sums are added in wave order through LDS, one row of result tiles at a time: the workgroup's partial
    float* const out = a.partial + ((size_t)blockIdx.y * gridDim.x + slice) * (size_t)(COUTP * NCOLS);
    float* const s_red = reinterpret_cast<float*>(s_mem);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        __syncthreads();          // the last tile, or the row before, has been read
#pragma unroll
        for (int t = 0; t < NTT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_red[((wave * NTT + t) * 4 + r) * 64 + lane] = acc[mt][t][r];
        __syncthreads();
        for (int i = tid; i < NTT * 256; i += CT_THREADS) {
            const float sum = ((s_red[i] + s_red[NTT * 256 + i]) + s_red[2 * NTT * 256 + i]) + s_red[3 * NTT * 256 + i];
            const int l = i & 63, r = (i >> 6) & 3, t = i >> 8;
            out[(mt * 16 + (l >> 4) * 4 + r) * NCOLS + t * 16 + (l & 15)] = sum;
        }
    }
}

// dW[o, i, t] and db[o]: the partials of the strips, in strip order, in double; times 2^-k
__global__ void __launch_bounds__(CT_THREADS) hght_wsum_kernel(const float* __restrict__ partial, int strips, int slices, int coutp, int taps, int cout, int ca, int cb,
                                                               const HghtCtrl* ctrl, float* __restrict__ dw, float* __restrict__ db)
{
    const int cin = ca + cb, e = blockIdx.x * CT_THREADS + threadIdx.x, nw = cout * cin * taps, ncols = (taps + 1) * 16;
    if (e >= nw + cout) return;
    int o, slice, n;
    if (e < nw) {
        o = e / (cin * taps);
        const int rest = e - o * (cin * taps), i = rest / taps, t = rest - i * taps;
        const int oc = i < ca ? i / 8 : (ca + 7) / 8 + (i - ca) / 8, j = i < ca ? i % 8 : (i - ca) % 8;
        slice = oc >> 1;
        n = t * 16 + (oc & 1) * 8 + j;
    } else {
        o = e - nw; slice = 0; n = taps * 16;
    }
    const size_t block = (size_t)coutp * ncols;
    const float* q = partial + (size_t)slice * block + (size_t)o * ncols + n;
    double sum = 0.0;
    for (int s = 0; s < strips; ++s) sum += (double)q[(size_t)s * slices * block];
    const float v = (float)ldexp(sum, -ctrl->k);
    if (e < nw) dw[e] = v;
    else db[o] = v;
}

// ---- routing -----------------------------------------------------------------------------------------------------------------------------------------------
// out[y, x, c] = h((add[y, x, c] + (g_pool[y / 2, x / 2, c] if (y, x) is the first maximum of its window of t, else 0)) [t[y, x, c] > 0]), four channels per
// thread.  t, out: binary16, add, g_pool: float32, all pixel-major with cp channels; t, add, out at h x w, g_pool at h2 x w2 = (h / 2) x (w / 2).
__global__ void __launch_bounds__(CT_THREADS) hght_unpool_kernel(const float* __restrict__ g_pool, const _Float16* __restrict__ t, const float* __restrict__ add,
                                                                 _Float16* __restrict__ out, int cp, int h, int w, int h2, int w2, HghtCtrl* ctrl)
{
    const int groups = cp >> 2;
    const size_t i = (size_t)blockIdx.x * CT_THREADS + threadIdx.x, n = (size_t)h * w * groups;
    if (i >= n) return;
    const int c0 = 4 * (int)(i % groups), p = (int)(i / groups), y = p / w, x = p - y * w;
    const int py = y >> 1, px = x >> 1, pyc = min(py, h2 - 1), pxc = min(px, w2 - 1);
    const _Float16* const q = t + ((size_t)(2 * pyc) * w + 2 * pxc) * cp + c0;          // 2 pyc + 1 <= 2 h2 - 1 <= h - 1
    const cth_h4 v0 = *reinterpret_cast<const cth_h4*>(q), v1 = *reinterpret_cast<const cth_h4*>(q + cp),
                  v2 = *reinterpret_cast<const cth_h4*>(q + (size_t)w * cp), v3 = *reinterpret_cast<const cth_h4*>(q + ((size_t)w + 1) * cp);
    const ct_f32x4 routed = *reinterpret_cast<const ct_f32x4*>(g_pool + ((size_t)pyc * w2 + pxc) * cp + c0);
    const ct_f32x4 skip = *reinterpret_cast<const ct_f32x4*>(add + (size_t)p * cp + c0);
    const cth_h4 me = *reinterpret_cast<const cth_h4*>(t + (size_t)p * cp + c0);
    const int mine_k = 2 * (y & 1) + (x & 1);
    cth_h4 res;
    int bad = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const _Float16 v[4] = {v0[r], v1[r], v2[r], v3[r]};
        int best = 0;
#pragma unroll
        for (int kk = 1; kk < 4; ++kk)
            if (v[kk] > v[best]) best = kk;
        const bool mine = py < h2 && px < w2 && best == mine_k;
        const float sum = skip[r] + (mine ? routed[r] : 0.0f);
        res[r] = me[r] > (_Float16)0.0f ? (_Float16)sum : (_Float16)0.0f;
        bad += hght_bad(res[r]) ? 1 : 0;
    }
    *reinterpret_cast<cth_h4*>(out + (size_t)p * cp + c0) = res;
    if (bad) atomicAdd(&ctrl->nonfinite, bad);
}

// out[Y, X, c] = h((the sum of g[y, x, c] over the (y, x) of the h x w frame whose nearest source is (Y, X), rows then columns) [t[Y, X, c] > 0]).  t, out: hl x wl.
__global__ void __launch_bounds__(CT_THREADS) hght_unup_kernel(const float* __restrict__ g, const _Float16* __restrict__ t, _Float16* __restrict__ out, int cp, int h, int w,
                                                               int hl, int wl, HghtCtrl* ctrl)
{
    const int groups = cp >> 2;
    const size_t i = (size_t)blockIdx.x * CT_THREADS + threadIdx.x, n = (size_t)hl * wl * groups;
    if (i >= n) return;
    const int c0 = 4 * (int)(i % groups), p = (int)(i / groups), Y = p / wl, X = p - Y * wl;
    const int y0 = (int)(((int64_t)Y * h + hl - 1) / hl), y1 = min((int)(((int64_t)(Y + 1) * h + hl - 1) / hl), h);
    const int x0 = (int)(((int64_t)X * w + wl - 1) / wl), x1 = min((int)(((int64_t)(X + 1) * w + wl - 1) / wl), w);
    ct_f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) sum += *reinterpret_cast<const ct_f32x4*>(g + ((size_t)y * w + x) * cp + c0);
    const cth_h4 me = *reinterpret_cast<const cth_h4*>(t + (size_t)p * cp + c0);
    cth_h4 res;
    int bad = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        res[r] = me[r] > (_Float16)0.0f ? (_Float16)sum[r] : (_Float16)0.0f;
        bad += hght_bad(res[r]) ? 1 : 0;
    }
    *reinterpret_cast<cth_h4*>(out + (size_t)p * cp + c0) = res;
    if (bad) atomicAdd(&ctrl->nonfinite, bad);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
struct HghtStrips {          // how a frame of h x w is cut into strips of tiles
    int tiles_x, ntiles, strip_tiles, strips;
    HghtStrips(int h, int w)
    {
        tiles_x = (w + HGHT_WT_W - 1) / HGHT_WT_W;
        ntiles = tiles_x * ((h + HGHT_WT_H - 1) / HGHT_WT_H);
        strip_tiles = (ntiles + HGHT_MAX_STRIPS - 1) / HGHT_MAX_STRIPS;
        if (strip_tiles < HGHT_MIN_STRIP_TILES) strip_tiles = HGHT_MIN_STRIP_TILES;
        strips = (ntiles + strip_tiles - 1) / strip_tiles;
    }
};

constexpr int hght_slices(int ca, int cb) { return (cth_octets(ca) + cth_octets(cb) + 1) / 2; }

// the floats of the partials of the weight gradients of layers I .. of HG_LAYERS, each at its own resolution: the most any of them takes
template <int I = 0>
static size_t hght_partial_floats(const int (&h)[3], const int (&w)[3])
{
    if constexpr (I == HG_LAYER_COUNT) return 0;
    else {
        constexpr HgLayer L = HG_LAYERS[I];
        const size_t mine = (size_t)HghtStrips(h[L.level], w[L.level]).strips * hght_slices(L.ca, L.cb) * (size_t)(((L.cout + 15) / 16) * 16 * (L.side * L.side + 1) * 16);
        const size_t rest = hght_partial_floats<I + 1>(h, w);
        return mine > rest ? mine : rest;
    }
}

// the operand fragments, in the order of the packing launch's table
enum { HGHT_W_DEC1, HGHT_W_FUSE, HGHT_W_FINAL_T, HGHT_W_FUSE_T_LO, HGHT_W_FUSE_T_HI, HGHT_W_DEC1_T_A, HGHT_W_DEC1_T_B, HGHT_W_UP1_T, HGHT_W_DEC2_T_A,
       HGHT_W_DEC2_T_B, HGHT_W_UP2_T, HGHT_W_ENC3_T, HGHT_W_ENC2_T, HGHT_W_ENC1_T };
constexpr int HGHT_ITEM_FRAGS[HGHT_ITEMS] = {cth_frags3(10, 38), CTH_FUSE_STEPS * 3 * 64, 3 * 64, 2 * 3 * 64, 2 * 3 * 64, cth_frags3(5, 38), cth_frags3(5, 38),
                                             cth_frags3(5, 19), cth_frags3(3, 19), cth_frags3(3, 19), cth_frags3(3, 9), cth_frags3(2, 19), cth_frags3(3, 38), cth_frags3(5, 38)};
constexpr int hght_at(int i) { return i == 0 ? 0 : hght_at(i - 1) + HGHT_ITEM_FRAGS[i - 1]; }
constexpr int HGHT_FRAGS = hght_at(HGHT_ITEMS);
static_assert((size_t)HGHT_FRAGS * 16 == IBGS_HGHT_PACKED_WEIGHT_BYTES, "the header's size of the packed weights");

struct HghtScratch {          // the arena of the header, in its order
    HghtCtrl* ctrl;
    _Float16 *d1, *f, *Gf, *Gd1, *gs, *Gd2, *Gu2, *Ge2, *Gb;
    float *e1a, *Iup1, *e2a, *Iup2, *Ienc2, *Ienc3, *partial;
    cth_h8* packed;
    size_t bytes;
    HghtScratch(char* base, int H, int W)
    {
        const int h[3] = {H, H / 2, H / 2 / 2}, w[3] = {W, W / 2, W / 2 / 2};
        const size_t p1 = (size_t)H * W, p2 = (size_t)h[1] * w[1], p4 = (size_t)h[2] * w[2];
        Carver c(base);
        ctrl = reinterpret_cast<HghtCtrl*>(c.take<char>(128));
        d1 = c.take<_Float16>(40 * p1);
        f = c.take<_Float16>(40 * p1);
        Gf = c.take<_Float16>(40 * p1);
        Gd1 = c.take<_Float16>(40 * p1);
        gs = c.take<_Float16>(8 * p1);
        e1a = c.take<float>(40 * p1);
        Iup1 = c.take<float>(24 * p1);
        Gd2 = c.take<_Float16>(24 * p2);
        Gu2 = c.take<_Float16>(24 * p2);
        Ge2 = c.take<_Float16>(24 * p2);
        e2a = c.take<float>(24 * p2);
        Iup2 = c.take<float>(16 * p2);
        Ienc2 = c.take<float>(40 * p2);
        Gb = c.take<_Float16>(16 * p4);
        Ienc3 = c.take<float>(24 * p4);
        packed = c.take<cth_h8>(HGHT_FRAGS);
        partial = c.take<float>(hght_partial_floats(h, w));
        bytes = hg_carved_bytes(c, base);
    }
};

template <int CA, int CB, int COUT, int EPI>
static void hght_conv(hipStream_t st, const HghtConv& a)
{
    const dim3 grid((unsigned)((a.w + CT_TILE - 1) / CT_TILE), (unsigned)((a.h + CT_TILE - 1) / CT_TILE));
    hipLaunchKernelGGL((hght_conv3_kernel<CA, CB, COUT, EPI>), grid, dim3(CT_THREADS), 0, st, a);
}

// the input gradient of a 3 x 3 layer from its G (CL channels): COUT rows of the transposed weight
static HghtConv hght_dgrad(const _Float16* G, const cth_h8* wfrag, HghtCtrl* ctrl, int h, int w)
{
    HghtConv a = {};
    a.a = G; a.wfrag = wfrag; a.ctrl = ctrl; a.h = h; a.w = w;
    return a;
}
static HghtConv hght_dgrad_f32(const _Float16* G, const cth_h8* wfrag, HghtCtrl* ctrl, int h, int w, float* out)
{
    HghtConv a = hght_dgrad(G, wfrag, ctrl, h, w);
    a.out32 = out;
    return a;
}
static HghtConv hght_dgrad_mask(const _Float16* G, const cth_h8* wfrag, HghtCtrl* ctrl, int h, int w, const _Float16* mask, _Float16* out)
{
    HghtConv a = hght_dgrad(G, wfrag, ctrl, h, w);
    a.mask = mask; a.out16 = out;
    return a;
}

template <int CA, int CB, int COUT, int MODE, int TAPS>
static void hght_wgrad(hipStream_t st, const _Float16* G, const _Float16* in_a, const _Float16* in_b, const HghtScratch& sc, float* dw, float* db, int h, int w, int hs, int ws)
{
    const HghtStrips strips(h, w);
    constexpr int SLICES = hght_slices(CA, CB);
    HghtWgrad a = {};
    a.g = G; a.a = in_a; a.b = in_b; a.partial = sc.partial; a.h = h; a.w = w; a.hs = hs; a.ws = ws;
    a.tiles_x = strips.tiles_x; a.ntiles = strips.ntiles; a.strip_tiles = strips.strip_tiles;
    hipLaunchKernelGGL((hght_wgrad_kernel<CA, CB, COUT, MODE, TAPS>), dim3(SLICES, (unsigned)strips.strips), dim3(CT_THREADS), 0, st, a);
    const int n = COUT * (CA + CB) * TAPS + COUT;
    hipLaunchKernelGGL(hght_wsum_kernel, dim3(grid_for((size_t)n, CT_THREADS)), dim3(CT_THREADS), 0, st, sc.partial, strips.strips, SLICES, ((COUT + 15) / 16) * 16, TAPS, COUT,
                       CA, CB, sc.ctrl, dw, db);
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_hgh_train_required_scratch(int64_t H, int64_t W)
{
    return hg_shape_ok(nullptr, H, W) ? HghtScratch(nullptr, (int)H, (int)W).bytes : 0;
}

int32_t ibgs_hgh_train_backward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                                const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                                const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                                const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                                float burned_in_gauss, const void* forward_arena, const float* grad_residual, const float* grad_image_pred, int32_t scale_mode,
                                int32_t grad_scale_log2, int32_t* status, float* grad_x, float* grad_enc1_w, float* grad_enc1_b, float* grad_enc2_w,
                                float* grad_enc2_b, float* grad_enc3_w, float* grad_enc3_b, float* grad_up2_conv_w, float* grad_up2_conv_b, float* grad_dec2_w,
                                float* grad_dec2_b, float* grad_up1_conv_w, float* grad_up1_conv_b, float* grad_dec1_w, float* grad_dec1_b,
                                float* grad_fuse_input_w, float* grad_fuse_input_b, float* grad_final_w, float* grad_final_b, void* scratch, size_t scratch_bytes)
{
    const char* const who = "hgh_train_backward";
    if (!hg_shape_ok(who, H, W)) return -IBGS_ERR_INVALID;
    if (!x) { set_error("%s: null input", who); return -IBGS_ERR_INVALID; }
    const float* const params[18] = {enc1_w, enc1_b, enc2_w, enc2_b, enc3_w, enc3_b, up2_conv_w, up2_conv_b, dec2_w, dec2_b, up1_conv_w, up1_conv_b, dec1_w, dec1_b,
                                     fuse_input_w, fuse_input_b, final_w, final_b};
    float* const grads[18] = {grad_enc1_w, grad_enc1_b, grad_enc2_w, grad_enc2_b, grad_enc3_w, grad_enc3_b, grad_up2_conv_w, grad_up2_conv_b, grad_dec2_w, grad_dec2_b,
                              grad_up1_conv_w, grad_up1_conv_b, grad_dec1_w, grad_dec1_b, grad_fuse_input_w, grad_fuse_input_b, grad_final_w, grad_final_b};
    if (!hg_params_ok(who, params)) return -IBGS_ERR_INVALID;
    if (!forward_arena) { set_error("%s: null stages arena", who); return -IBGS_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(forward_arena) & 127) { set_error("%s: stages arena is not 128-byte aligned", who); return -IBGS_ERR_INVALID; }
    if (!grad_residual && !grad_image_pred) { set_error("%s: null upstream: grad_residual and grad_image_pred are both null", who); return -IBGS_ERR_INVALID; }
    if (scale_mode != IBGS_HGHT_SCALE_AUTO && scale_mode != IBGS_HGHT_SCALE_FIXED) { set_error("%s: scale_mode %d is neither automatic (0) nor fixed (1)", who, (int)scale_mode); return -IBGS_ERR_INVALID; }
    if (scale_mode == IBGS_HGHT_SCALE_FIXED && (grad_scale_log2 < -300 || grad_scale_log2 > 300)) { set_error("%s: grad_scale_log2 %d is out of range (-300 .. 300)", who, (int)grad_scale_log2); return -IBGS_ERR_INVALID; }
    int given = 0;
    for (int i = 0; i < 18; ++i) given += grads[i] != nullptr;
    if (given != 0 && given != 18) {
        const int i = hg_first_null(grads);
        set_error("%s: null gradients: %s's %s (the eighteen are given together or not at all)", who, HG_LAYERS[i / 2].name, hg_part(i));
        return -IBGS_ERR_INVALID;
    }
    const bool want_params = given == 18, want_x = grad_x != nullptr;
    if (!want_params && !want_x) { set_error("%s: null outputs: neither grad_x nor the parameter gradients are asked for", who); return -IBGS_ERR_INVALID; }
    const HghtScratch sc(static_cast<char*>(scratch), H, W);
    if (!arena_ok(who, "scratch", scratch, scratch_bytes, sc.bytes)) return -IBGS_ERR_INVALID;
    Carver fa(static_cast<char*>(const_cast<void*>(forward_arena)));          // the arena of ibgs_hgh_forward, read only: h(x), then the six stages
    const _Float16* const xh = fa.take<_Float16>(8 * CTH_XO * (size_t)H * (size_t)W);
    const HgStages<const _Float16> sg = hg_carve_stages<const _Float16>(fa, (size_t)H, (size_t)W, 8);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2;
    const size_t p1 = (size_t)H * W, p2 = (size_t)H2 * W2, p4 = (size_t)H4 * W4;
    HghtCtrl* const ctrl = sc.ctrl;
    auto frag = [&](int i) { return sc.packed + hght_at(i); };

    // the control words, the scale, the operands
    IBGS_HIP(hipMemsetAsync(ctrl, 0, sizeof(HghtCtrl), st));
    const bool fixed = scale_mode == IBGS_HGHT_SCALE_FIXED;
    hipLaunchKernelGGL(hght_scale_kernel, dim3(fixed ? 1u : (grid_for(3 * p1, CT_THREADS) < (unsigned)HGHT_SCALE_BLOCKS ? grid_for(3 * p1, CT_THREADS) : (unsigned)HGHT_SCALE_BLOCKS)), dim3(CT_THREADS), 0, st, grad_residual,
                       grad_image_pred, 3 * p1, fixed ? 1 : 0, (int)grad_scale_log2, ctrl);
    HghtPackArgs pk = {};
    pk.packed = sc.packed; pk.frags = HGHT_FRAGS;
    const HghtPackItem items[HGHT_ITEMS] = {
        {dec1_w, HGHT_P3_FWD, 38, 38, 38, 0, 0, 0},          {fuse_input_w, HGHT_P1_FWD, 38, 38, 38, 0, 0, 0},
        {final_w, HGHT_P1_T_PLAIN, 38, 3, 0, 38, 0, 0},      {fuse_input_w, HGHT_P1_T_ACC, 38, 38, 0, 76, 0, 0}, {fuse_input_w, HGHT_P1_T_ACC, 38, 38, 0, 76, 38, 0},
        {dec1_w, HGHT_P3_T, 38, 38, 0, 76, 0, 0},            {dec1_w, HGHT_P3_T, 38, 38, 0, 76, 38, 0},          {up1_conv_w, HGHT_P3_T, 19, 38, 0, 19, 0, 0},
        {dec2_w, HGHT_P3_T, 19, 19, 0, 38, 0, 0},            {dec2_w, HGHT_P3_T, 19, 19, 0, 38, 19, 0},          {up2_conv_w, HGHT_P3_T, 9, 19, 0, 9, 0, 0},
        {enc3_w, HGHT_P3_T, 19, 9, 0, 19, 0, 0},             {enc2_w, HGHT_P3_T, 38, 19, 0, 38, 0, 0},           {enc1_w, HGHT_P3_T, 38, 38, 0, 38, 0, 0}};
    for (int i = 0; i < HGHT_ITEMS; ++i) { pk.item[i] = items[i]; pk.item[i].first = hght_at(i); }
    hipLaunchKernelGGL(hght_pack_kernel, dim3(grid_for(HGHT_FRAGS, CT_THREADS)), dim3(CT_THREADS), 0, st, pk);

    // the head: d1, f, gS, G_f, G_d1 and the head's share of grad_x
    HghtConv head = {};
    head.a = sg.u1; head.b = sg.e1; head.wfrag = frag(HGHT_W_DEC1); head.h = H; head.w = W; head.ctrl = ctrl; head.grad_x = grad_x;
    head.bias = dec1_b; head.xh = xh; head.fuse_frag = frag(HGHT_W_FUSE); head.fuse_b = fuse_input_b; head.finalT_frag = frag(HGHT_W_FINAL_T);
    head.fuseT_lo = frag(HGHT_W_FUSE_T_LO); head.fuseT_hi = frag(HGHT_W_FUSE_T_HI); head.g_res = grad_residual; head.g_ip = grad_image_pred; head.burned = burned_in_gauss;
    head.d1 = sc.d1; head.f = sc.f; head.Gf = sc.Gf; head.Gd1 = sc.Gd1; head.gs = sc.gs;
    hght_conv<38, 38, 38, HGHT_EPI_HEAD>(st, head);
    if (want_params) {
        hght_wgrad<38, 0, 3, CT_PLAIN, 1>(st, sc.gs, sc.f, nullptr, sc, grad_final_w, grad_final_b, H, W, H, W);
        hght_wgrad<38, 38, 38, CT_PLAIN, 1>(st, sc.Gf, sc.d1, xh, sc, grad_fuse_input_w, grad_fuse_input_b, H, W, H, W);
        hght_wgrad<38, 38, 38, CT_PLAIN, 9>(st, sc.Gd1, sg.u1, sg.e1, sc, grad_dec1_w, grad_dec1_b, H, W, H, W);
    }
    // dec1: G_u1 (in G_f's place), g_e1a
    _Float16* const Gu1 = sc.Gf;
    hght_conv<38, 0, 38, HGHT_EPI_MASK>(st, hght_dgrad_mask(sc.Gd1, frag(HGHT_W_DEC1_T_A), ctrl, H, W, sg.u1, Gu1));
    hght_conv<38, 0, 38, HGHT_EPI_F32>(st, hght_dgrad_f32(sc.Gd1, frag(HGHT_W_DEC1_T_B), ctrl, H, W, sc.e1a));
    // up1_conv: G_d2
    if (want_params) hght_wgrad<19, 0, 38, CT_UP, 9>(st, Gu1, sg.d2, nullptr, sc, grad_up1_conv_w, grad_up1_conv_b, H, W, H2, W2);
    hght_conv<38, 0, 19, HGHT_EPI_F32>(st, hght_dgrad_f32(Gu1, frag(HGHT_W_UP1_T), ctrl, H, W, sc.Iup1));
    hipLaunchKernelGGL(hght_unup_kernel, dim3(grid_for(6 * p2, CT_THREADS)), dim3(CT_THREADS), 0, st, sc.Iup1, sg.d2, sc.Gd2, 24, H, W, H2, W2, ctrl);
    // dec2: G_u2, g_e2a
    if (want_params) hght_wgrad<19, 19, 19, CT_PLAIN, 9>(st, sc.Gd2, sg.u2, sg.e2, sc, grad_dec2_w, grad_dec2_b, H2, W2, H2, W2);
    hght_conv<19, 0, 19, HGHT_EPI_MASK>(st, hght_dgrad_mask(sc.Gd2, frag(HGHT_W_DEC2_T_A), ctrl, H2, W2, sg.u2, sc.Gu2));
    hght_conv<19, 0, 19, HGHT_EPI_F32>(st, hght_dgrad_f32(sc.Gd2, frag(HGHT_W_DEC2_T_B), ctrl, H2, W2, sc.e2a));
    // up2_conv: G_b
    if (want_params) hght_wgrad<9, 0, 19, CT_UP, 9>(st, sc.Gu2, sg.b, nullptr, sc, grad_up2_conv_w, grad_up2_conv_b, H2, W2, H4, W4);
    hght_conv<19, 0, 9, HGHT_EPI_F32>(st, hght_dgrad_f32(sc.Gu2, frag(HGHT_W_UP2_T), ctrl, H2, W2, sc.Iup2));
    hipLaunchKernelGGL(hght_unup_kernel, dim3(grid_for(4 * p4, CT_THREADS)), dim3(CT_THREADS), 0, st, sc.Iup2, sg.b, sc.Gb, 16, H2, W2, H4, W4, ctrl);
    // enc3: G_e2
    if (want_params) hght_wgrad<19, 0, 9, CT_POOL, 9>(st, sc.Gb, sg.e2, nullptr, sc, grad_enc3_w, grad_enc3_b, H4, W4, H2, W2);
    hght_conv<9, 0, 19, HGHT_EPI_F32>(st, hght_dgrad_f32(sc.Gb, frag(HGHT_W_ENC3_T), ctrl, H4, W4, sc.Ienc3));
    hipLaunchKernelGGL(hght_unpool_kernel, dim3(grid_for(6 * p2, CT_THREADS)), dim3(CT_THREADS), 0, st, sc.Ienc3, sg.e2, sc.e2a, sc.Ge2, 24, H2, W2, H4, W4, ctrl);
    // enc2: G_e1 (in G_d1's place)
    _Float16* const Ge1 = sc.Gd1;
    if (want_params) hght_wgrad<38, 0, 19, CT_POOL, 9>(st, sc.Ge2, sg.e1, nullptr, sc, grad_enc2_w, grad_enc2_b, H2, W2, H, W);
    hght_conv<19, 0, 38, HGHT_EPI_F32>(st, hght_dgrad_f32(sc.Ge2, frag(HGHT_W_ENC2_T), ctrl, H2, W2, sc.Ienc2));
    hipLaunchKernelGGL(hght_unpool_kernel, dim3(grid_for(10 * p1, CT_THREADS)), dim3(CT_THREADS), 0, st, sc.Ienc2, sg.e1, sc.e1a, Ge1, 40, H, W, H2, W2, ctrl);
    // enc1
    if (want_params) hght_wgrad<38, 0, 38, CT_PLAIN, 9>(st, Ge1, xh, nullptr, sc, grad_enc1_w, grad_enc1_b, H, W, H, W);
    if (want_x) {
        HghtConv last = hght_dgrad(Ge1, frag(HGHT_W_ENC1_T), ctrl, H, W);
        last.grad_x = grad_x;
        hght_conv<38, 0, 38, HGHT_EPI_GRADX>(st, last);
    }
    if (status) hipLaunchKernelGGL(hght_status_kernel, dim3(1), dim3(64), 0, st, ctrl, status);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
