// The half-precision forward of the hourglass CNN (C ABI: include/ibgs_hg_half.h; Python: ibgs_amd/hourglass.py, precision="float16"): the network of
// hourglass.hip with the roundings of the reference's test-time run under torch.autocast(float16) -- x, weights, biases and the eight ReLU stages rounded to
// binary16 (to nearest even), every convolution a float32 accumulation of exact binary16 products on the matrix cores, `final` left in float32.  One packing
// launch (x and the weights into the arena), then seven launches of ONE templated 3 x 3 implicit-GEMM kernel; the last one carries the two 1 x 1
// convolutions and image_pred: d1 and f never reach memory.  The float32 boundary, the limits and the messages are those of ibgs_hg_forward.
//
// THE PRODUCTS are v_mfma_f32_16x16x32_f16.  Output channels are M (38 -> 48, 19 -> 32, 9 -> 16), 16 pixels of one row are N, and lane l = (column l & 15,
// kq = l >> 4) holds A[row l & 15][k = 8 kq + j] and B[k = 8 kq + j][column l & 15], j = 0 .. 7; register r of a result tile is channel 4 kq + r of pixel
// l & 15.  A STAGE IN MEMORY is pixel-major binary16 with the channels innermost, padded with zeros to a multiple of 8 ("octets": 38 -> 5, 19 -> 3, 9 -> 2), so
// a lane's eight k are ONE 16-byte read.  The k order (free: the contract is a tolerance): the input [A | B] is a row of octets, taken four at a time (a
// CHUNK, 32 channels); inside a chunk one k-step is one tap, and kq is the octet.  Padding costs products, which are cheap here: 38 channels run as 64,
// [38 | 38] as 96, 19 and 9 as 32 (DESIGN.md section 15 has the shares).
//
// KERNEL  hgh_conv3_kernel<CA, CB, COUT, MODE, FUSE>: 256 threads = 4 waves per 16 x 16 output tile on a 2-D uncapped grid; a wave owns four rows of the tile
// and all output channels.  Per chunk the workgroup stages the 18 x 18 window of four octets (pooled, upsampled or plain as MODE says; 80 bytes per pixel in
// LDS: an odd number of 16-byte units, so the sixteen pixels of a quarter-wave read disjoint banks) and the chunk's weights (copied as they lie in the arena:
// fragment (tap, M tile, lane), which a wave reads back as consecutive 16 bytes per lane), then runs 9 k-steps.  The loads of chunk c + 1 are issued before
// the products of chunk c.  Coordinates are clamped INTO the frame before an offset is formed, every load is unconditional, and zeros are selected afterwards
// for what lies outside the frame or past the last octet: the arena may hold anything before the call, and no byte that was not written by this call reaches a
// product.  In the last launch the accumulator tile, rounded, is the next product's B operand as it stands: k-step s takes the M tiles 2 s and 2 s + 1, element
// j of a lane being channel 16 (2 s + (j >> 2)) + 4 kq + (j & 3), and hgh_pack_kernel lays the 1 x 1 weights out in that order.
#include "common.h"
#include "shared/hg_net.h"
#include "shared/conv_tile.h"
#include "../../include/ibgs_hourglass.h"
#include "../../include/ibgs_hg_half.h"

namespace ibgs {

typedef float hgh_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 hgh_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 hgh_h4 __attribute__((ext_vector_type(4)));

constexpr int HGH_TILE = 16;                         // side of a workgroup's output tile
constexpr int HGH_THREADS = 256;
constexpr int HGH_ROWS = HGH_TILE / (HGH_THREADS / 64);          // rows of the tile per wave
constexpr int HGH_WIN = HGH_TILE + 2;                // the staged window: tile and halo
constexpr int HGH_NPIX = HGH_WIN * HGH_WIN;
constexpr int HGH_PSTRIDE = 5;                       // 16-byte units per staged pixel: four octets and one of padding (odd)
constexpr int HGH_XO = (HG_C + 7) / 8;               // octets of x
static_assert(HGH_ROWS == 4 && HGH_PSTRIDE % 2 == 1 && HGH_THREADS % 4 == 0, "the lane maps and the bank argument above");

constexpr int hgh_octets(int c) { return (c + 7) / 8; }
// fragments (eight binary16 each) of a packed 3 x 3 layer: chunks x 9 taps x M tiles x 64 lanes
constexpr int hgh_frags(int ca, int cb, int cout) { return ((hgh_octets(ca) + hgh_octets(cb) + 3) / 4) * 9 * ((cout + 15) / 16) * 64; }
constexpr int HGH_FUSE_STEPS = 2 + (HGH_XO + 3) / 4, HGH_FIN_STEPS = 2;          // k-steps of fuse_input (d1: 2, x: 2) and final
// layer i of HG_LAYERS in the packed weights, which hold the nine in the order of the C ABI: its kind (0: 3 x 3; 1: fuse_input; 2: final), its fragments, its first one
constexpr int hgh_kind(int i) { return HG_LAYERS[i].side == 3 ? 0 : (i == HG_FINAL ? 2 : 1); }
constexpr int hgh_layer_frags(int i)
{
    const HgLayer& l = HG_LAYERS[i];
    return hgh_kind(i) == 0 ? hgh_frags(l.ca, l.cb, l.cout) : (hgh_kind(i) == 1 ? HGH_FUSE_STEPS : HGH_FIN_STEPS) * ((l.cout + 15) / 16) * 64;
}
constexpr int hgh_at(int i) { return i == 0 ? 0 : hgh_at(i - 1) + hgh_layer_frags(i - 1); }
constexpr int HGH_FRAGS = hgh_at(HG_LAYER_COUNT);
static_assert((size_t)HGH_FRAGS * 16 == IBGS_HGH_PACKED_WEIGHT_BYTES, "the header's size of the packed weights");

__device__ __forceinline__ hgh_f32x4 hgh_mfma(hgh_h8 a, hgh_h8 b, hgh_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float hgh_round(float v) { return (float)(_Float16)v; }          // to binary16, to nearest even, and back

// ---- the packing launch: h(x) pixel-major, and the nine layers' weights as operand fragments ---------------------------------------------------------------
struct HghPackLayer {
    const float* w;
    int cout, ca, cb;          // rows; channels of the two inputs ([a | b] along Cin)
    int first;                 // its first fragment
    int kind;                  // 0: 3 x 3; 1: fuse_input; 2: final
};
struct HghPackArgs {
    const float* x; hgh_h8* xh; size_t pixels; unsigned x_blocks;
    hgh_h8* packed;
    HghPackLayer layer[9];
};

__global__ void __launch_bounds__(HGH_THREADS) hgh_pack_kernel(const HghPackArgs a)
{
    if (blockIdx.x < a.x_blocks) {          // (uniform over the workgroup)
        const size_t p = (size_t)blockIdx.x * HGH_THREADS + threadIdx.x;
        if (p >= a.pixels) return;
#pragma unroll
        for (int o = 0; o < HGH_XO; ++o) {
            hgh_h8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 8 * o + j < HG_C ? (_Float16)a.x[(size_t)(8 * o + j) * a.pixels + p] : (_Float16)0.0f;
            a.xh[p * HGH_XO + o] = v;
        }
        return;
    }
    const int i = (int)(blockIdx.x - a.x_blocks) * HGH_THREADS + (int)threadIdx.x;
    if (i >= HGH_FRAGS) return;
    HghPackLayer L = a.layer[0];
#pragma unroll
    for (int n = 1; n < 9; ++n)
        if (i >= a.layer[n].first) L = a.layer[n];          // (selects: the table is never indexed by a register)
    const int local = i - L.first, lane = local & 63, rest = local >> 6, kq = lane >> 4;
    hgh_h8 v;
    if (L.kind == 0) {
        const int noa = hgh_octets(L.ca), nob = hgh_octets(L.cb), mtn = (L.cout + 15) / 16;
        const int mt = rest % mtn, t = (rest / mtn) % 9, c = rest / (mtn * 9), m = mt * 16 + (lane & 15), o = 4 * c + kq;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int idx = -1;
            if (o < noa) { if (8 * o + j < L.ca) idx = 8 * o + j; }
            else if (o < noa + nob) { if (8 * (o - noa) + j < L.cb) idx = L.ca + 8 * (o - noa) + j; }
            v[j] = (m < L.cout && idx >= 0) ? (_Float16)L.w[((size_t)m * (L.ca + L.cb) + idx) * 9 + t] : (_Float16)0.0f;
        }
    } else {
        const int mtn = L.kind == 1 ? 3 : 1, mt = rest % mtn, s = rest / mtn, m = mt * 16 + (lane & 15), cin = L.ca + L.cb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int idx = -1;
            if (s < 2) { const int ch = (2 * s + (j >> 2)) * 16 + 4 * kq + (j & 3); if (ch < L.ca) idx = ch; }          // the order an accumulator tile gives
            else { const int ch = 8 * (4 * (s - 2) + kq) + j; if (ch < L.cb) idx = L.ca + ch; }
            v[j] = (m < L.cout && idx >= 0) ? (_Float16)L.w[(size_t)m * cin + idx] : (_Float16)0.0f;
        }
    }
    a.packed[i] = v;
}

// ---- the convolution ------------------------------------------------------------------------------------------------------------------------------------
struct HghArgs {
    const _Float16* a; const _Float16* b;          // the two inputs ([a | b] along the channels), pixel-major; b may be null when CB == 0
    const hgh_h8* wfrag; const float* bias;        // the layer's packed weights; its float32 bias (COUT), rounded here
    _Float16* out;                                 // h x w pixels of CPOUT channels (null in the last launch)
    int h, w, hs, ws;                              // the output's resolution, and a's
    // the last launch: h(x) pixel-major, x (38 float32 planes), the packed fuse_input and final, the two outputs
    const _Float16* xh; const float* x; const hgh_h8* fuse_frag; const float* fuse_b; const hgh_h8* final_frag; const float* final_b;
    float burned; float* residual; float* image_pred;
};

// ReLU, rounded: M tiles 2 s and 2 s + 1 of a row of accumulator tiles as the B fragment of k-step s
template <int MT>
__device__ __forceinline__ hgh_h8 hgh_as_operand(const hgh_f32x4 (&t)[MT][HGH_ROWS], int nt, int s)
{
    hgh_h8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int tile = 2 * s + (j >> 2);
        float f = 0.0f;
        if (tile < MT) f = t[tile][nt][j & 3];
        v[j] = (_Float16)(f > 0.0f ? f : 0.0f);
    }
    return v;
}

template <int CA, int CB, int COUT, int MODE, bool FUSE>
__global__ void __launch_bounds__(HGH_THREADS, 2) hgh_conv3_kernel(const HghArgs a)
{
    constexpr int NOA = hgh_octets(CA), NOB = hgh_octets(CB), NO = NOA + NOB, NC = (NO + 3) / 4, MT = (COUT + 15) / 16, CPOUT = 8 * hgh_octets(COUT);
    constexpr int NWF = 9 * MT * 64;          // weight fragments of a chunk
    constexpr int NPOS = (HGH_NPIX * 4 + HGH_THREADS - 1) / HGH_THREADS, NW = (NWF + HGH_THREADS - 1) / HGH_THREADS;
    static_assert(CB == 0 || MODE == CT_PLAIN, "a second input is read plain, at the first one's resolution");
    static_assert(!FUSE || (COUT == HG_C && MT == 3), "the last launch is dec1");
    __shared__ hgh_h8 s_in[HGH_NPIX * HGH_PSTRIDE];
    __shared__ hgh_h8 s_w[NWF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int tx0 = blockIdx.x * HGH_TILE, ty0 = blockIdx.y * HGH_TILE;
    const int h = a.h, w = a.w;

    hgh_f32x4 acc[MT][HGH_ROWS];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        hgh_f32x4 start;
#pragma unroll
        for (int r = 0; r < 4; ++r) start[r] = mt * 16 + kq * 4 + r < COUT ? hgh_round(a.bias[mt * 16 + kq * 4 + r]) : 0.0f;
#pragma unroll
        for (int nt = 0; nt < HGH_ROWS; ++nt) acc[mt][nt] = start;
    }

    // What a thread stages does not depend on the chunk but for the octet: octet tid & 3 of the window pixels (tid >> 2) + 64 r, and NW weight fragments.  A
    // pixel's index into a stage is formed once, from coordinates clamped INTO the frame.
    const int o4 = tid & 3;
    int pos[NPOS];          // pixel index into a (and into b: read plain at the same resolution)
    bool pos_in[NPOS];
#pragma unroll
    for (int r = 0; r < NPOS; ++r) {
        const int p = (tid >> 2) + r * (HGH_THREADS / 4), pc = p < HGH_NPIX ? p : 0;
        const int yy = pc / HGH_WIN, xx = pc - yy * HGH_WIN, y = ty0 + yy - 1, x = tx0 + xx - 1;
        pos_in[r] = p < HGH_NPIX && y >= 0 && y < h && x >= 0 && x < w;
        pos[r] = ct_source_offset<MODE>(y, x, h, w, a.hs, a.ws);          // a holds hs x ws pixels, read as MODE says
    }
    hgh_h8 iv[NPOS], wv[NW];
    const hgh_h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    auto load_chunk = [&](const int c) {
        const int oc = 4 * c + o4, occ = oc < NO ? oc : NO - 1;          // this thread's octet of [a | b], clamped to the last one
        const bool from_a = CB == 0 || occ < NOA;
        const _Float16* const base = from_a ? a.a + occ * 8 : a.b + (occ - NOA) * 8;
        const size_t cp = from_a ? NOA * 8 : NOB * 8;          // binary16 per pixel of that input
#pragma unroll
        for (int r = 0; r < NPOS; ++r) {
            const _Float16* const q = base + (size_t)pos[r] * cp;
            hgh_h8 v = *reinterpret_cast<const hgh_h8*>(q);
            if (MODE == CT_POOL) {
                const hgh_h8 v1 = *reinterpret_cast<const hgh_h8*>(q + cp), v2 = *reinterpret_cast<const hgh_h8*>(q + (size_t)a.ws * cp),
                             v3 = *reinterpret_cast<const hgh_h8*>(q + ((size_t)a.ws + 1) * cp);
                v = __builtin_elementwise_max(__builtin_elementwise_max(v, v1), __builtin_elementwise_max(v2, v3));
            }
            iv[r] = (oc < NO && pos_in[r]) ? v : zero;
        }
#pragma unroll
        for (int n = 0; n < NW; ++n) wv[n] = a.wfrag[c * NWF + min(tid + n * HGH_THREADS, NWF - 1)];
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int r = 0; r < NPOS; ++r) {
            const int p = (tid >> 2) + r * (HGH_THREADS / 4);
            if (p < HGH_NPIX) s_in[p * HGH_PSTRIDE + o4] = iv[r];
        }
#pragma unroll
        for (int n = 0; n < NW; ++n)
            if (tid + n * HGH_THREADS < NWF) s_w[tid + n * HGH_THREADS] = wv[n];
    };
    const int window_at = (wave * HGH_ROWS * HGH_WIN + col) * HGH_PSTRIDE + kq;
    auto run_taps = [&]() {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            hgh_h8 av[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = s_w[(t * MT + mt) * 64 + lane];
#pragma unroll
            for (int nt = 0; nt < HGH_ROWS; ++nt) {
                const hgh_h8 bv = s_in[window_at + ((nt + t / 3) * HGH_WIN + t % 3) * HGH_PSTRIDE];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = hgh_mfma(av[mt], bv, acc[mt][nt]);
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

    const int x = tx0 + col;
    const size_t plane = (size_t)h * (size_t)w;
    if constexpr (!FUSE) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int c0 = mt * 16 + kq * 4;
            if (c0 < CPOUT) {          // (whole groups of four: CPOUT is a multiple of 8)
#pragma unroll
                for (int nt = 0; nt < HGH_ROWS; ++nt) {
                    const int y = ty0 + wave * HGH_ROWS + nt;
                    hgh_h4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = (c0 + r < COUT && acc[mt][nt][r] > 0.0f) ? (_Float16)acc[mt][nt][r] : (_Float16)0.0f;          // padding channels: zeros
                    if (y < h && x < w) *reinterpret_cast<hgh_h4*>(a.out + ((size_t)y * w + x) * CPOUT + c0) = v;
                }
            }
        }
    } else {
        // acc is d1 before its ReLU and rounding (padding channels: exact zeros).  fuse_input on [d1, h(x)], then final on f, the weights in the k order the
        // registers give, read from the arena as fragments.
        hgh_f32x4 f[3][HGH_ROWS];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            hgh_f32x4 start;
#pragma unroll
            for (int r = 0; r < 4; ++r) start[r] = mt * 16 + kq * 4 + r < HG_C ? hgh_round(a.fuse_b[mt * 16 + kq * 4 + r]) : 0.0f;
#pragma unroll
            for (int nt = 0; nt < HGH_ROWS; ++nt) f[mt][nt] = start;
        }
        const int xc = min(x, w - 1);
#pragma unroll
        for (int s = 0; s < HGH_FUSE_STEPS; ++s) {
            hgh_h8 av[3];
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) av[mt] = a.fuse_frag[(s * 3 + mt) * 64 + lane];
#pragma unroll
            for (int nt = 0; nt < HGH_ROWS; ++nt) {
                hgh_h8 bv;
                if (s < 2) bv = hgh_as_operand<3>(acc, nt, s);
                else {
                    const int o = 4 * (s - 2) + kq, yc = min(ty0 + wave * HGH_ROWS + nt, h - 1);
                    const hgh_h8 v = *reinterpret_cast<const hgh_h8*>(a.xh + ((size_t)yc * w + xc) * (HGH_XO * 8) + min(o, HGH_XO - 1) * 8);
                    bv = o < HGH_XO ? v : zero;
                }
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) f[mt][nt] = hgh_mfma(av[mt], bv, f[mt][nt]);
            }
        }
        hgh_f32x4 res[HGH_ROWS];
        {
            hgh_f32x4 start;
#pragma unroll
            for (int r = 0; r < 4; ++r) start[r] = kq * 4 + r < 3 ? hgh_round(a.final_b[min(kq * 4 + r, 2)]) : 0.0f;
#pragma unroll
            for (int nt = 0; nt < HGH_ROWS; ++nt) res[nt] = start;
        }
#pragma unroll
        for (int s = 0; s < HGH_FIN_STEPS; ++s) {
            const hgh_h8 av = a.final_frag[s * 64 + lane];
#pragma unroll
            for (int nt = 0; nt < HGH_ROWS; ++nt) res[nt] = hgh_mfma(av, hgh_as_operand<3>(f, nt, s), res[nt]);
        }
        if (kq == 0) {          // rows 0 .. 2 of the result tile: the three colour channels, unrounded
#pragma unroll
            for (int nt = 0; nt < HGH_ROWS; ++nt) {
                const int y = ty0 + wave * HGH_ROWS + nt;
                if (y < h && x < w) {
                    const size_t p = (size_t)y * w + x;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        a.residual[(size_t)ch * plane + p] = res[nt][ch];
                        if (a.image_pred) a.image_pred[(size_t)ch * plane + p] = hg_blend(a.burned, a.x[(size_t)(HG_C - 3 + ch) * plane + p], res[nt][ch]);
                    }
                }
            }
        }
    }
}

struct HghScratch {          // the arena of the header, in its order: h(x), the six stages (both pixel-major octets), the packed weights
    _Float16* xh;
    HgStages<_Float16> s;
    hgh_h8* packed;
    size_t bytes;
    HghScratch(char* base, size_t H, size_t W)
    {
        Carver c(base);
        xh = c.take<_Float16>(8 * HGH_XO * H * W);
        s = hg_carve_stages<_Float16>(c, H, W, 8);
        packed = c.take<hgh_h8>(HGH_FRAGS);
        bytes = hg_carved_bytes(c, base);
    }
};

template <int CA, int CB, int COUT, int MODE, bool FUSE>
static void hgh_launch(hipStream_t st, const HghArgs& a)
{
    const dim3 grid((unsigned)((a.w + HGH_TILE - 1) / HGH_TILE), (unsigned)((a.h + HGH_TILE - 1) / HGH_TILE));
    hipLaunchKernelGGL((hgh_conv3_kernel<CA, CB, COUT, MODE, FUSE>), grid, dim3(HGH_THREADS), 0, st, a);
}

static HghArgs hgh_layer(const _Float16* in_a, const _Float16* in_b, const hgh_h8* wfrag, const float* bias, _Float16* out, int h, int w, int hs, int ws)
{
    HghArgs a = {};
    a.a = in_a; a.b = in_b; a.wfrag = wfrag; a.bias = bias; a.out = out; a.h = h; a.w = w; a.hs = hs; a.ws = ws;
    return a;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_hgh_required_scratch(int64_t H, int64_t W)
{
    return hg_shape_ok(nullptr, H, W) ? HghScratch(nullptr, (size_t)H, (size_t)W).bytes : 0;
}

int32_t ibgs_hgh_forward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                         const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                         const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                         const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                         float burned_in_gauss, float* residual, float* image_pred, void* scratch, size_t scratch_bytes)
{
    if (!hg_shape_ok("hgh_forward", H, W)) return -IBGS_ERR_INVALID;
    if (!x) { set_error("hgh_forward: null input"); return -IBGS_ERR_INVALID; }
    const float* const params[18] = {enc1_w, enc1_b, enc2_w, enc2_b, enc3_w, enc3_b, up2_conv_w, up2_conv_b, dec2_w, dec2_b, up1_conv_w, up1_conv_b, dec1_w, dec1_b,
                                     fuse_input_w, fuse_input_b, final_w, final_b};
    if (!hg_params_ok("hgh_forward", params)) return -IBGS_ERR_INVALID;
    if (!residual) { set_error("hgh_forward: null outputs: residual is required"); return -IBGS_ERR_INVALID; }
    const HghScratch sc(static_cast<char*>(scratch), (size_t)H, (size_t)W);
    if (!arena_ok("hgh_forward", "scratch", scratch, scratch_bytes, sc.bytes)) return -IBGS_ERR_INVALID;
    const HgStages<_Float16>& s = sc.s;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2;

    HghPackArgs pk = {};
    pk.x = x; pk.xh = reinterpret_cast<hgh_h8*>(sc.xh); pk.pixels = (size_t)H * (size_t)W; pk.x_blocks = grid_for(pk.pixels, HGH_THREADS); pk.packed = sc.packed;
    for (int i = 0; i < HG_LAYER_COUNT; ++i) pk.layer[i] = {params[2 * i], HG_LAYERS[i].cout, HG_LAYERS[i].ca, HG_LAYERS[i].cb, hgh_at(i), hgh_kind(i)};
    hipLaunchKernelGGL(hgh_pack_kernel, dim3(pk.x_blocks + grid_for(HGH_FRAGS, HGH_THREADS)), dim3(HGH_THREADS), 0, st, pk);

    hgh_launch<38, 0, 38, CT_PLAIN, false>(st, hgh_layer(sc.xh, nullptr, sc.packed + hgh_at(HG_ENC1), enc1_b, s.e1, H, W, H, W));
    hgh_launch<38, 0, 19, CT_POOL, false>(st, hgh_layer(s.e1, nullptr, sc.packed + hgh_at(HG_ENC2), enc2_b, s.e2, H2, W2, H, W));
    hgh_launch<19, 0, 9, CT_POOL, false>(st, hgh_layer(s.e2, nullptr, sc.packed + hgh_at(HG_ENC3), enc3_b, s.b, H4, W4, H2, W2));
    hgh_launch<9, 0, 19, CT_UP, false>(st, hgh_layer(s.b, nullptr, sc.packed + hgh_at(HG_UP2_CONV), up2_conv_b, s.u2, H2, W2, H4, W4));
    hgh_launch<19, 19, 19, CT_PLAIN, false>(st, hgh_layer(s.u2, s.e2, sc.packed + hgh_at(HG_DEC2), dec2_b, s.d2, H2, W2, H2, W2));
    hgh_launch<19, 0, 38, CT_UP, false>(st, hgh_layer(s.d2, nullptr, sc.packed + hgh_at(HG_UP1_CONV), up1_conv_b, s.u1, H, W, H2, W2));
    HghArgs last = hgh_layer(s.u1, s.e1, sc.packed + hgh_at(HG_DEC1), dec1_b, nullptr, H, W, H, W);
    last.xh = sc.xh; last.x = x; last.fuse_frag = sc.packed + hgh_at(HG_FUSE_INPUT); last.fuse_b = fuse_input_b; last.final_frag = sc.packed + hgh_at(HG_FINAL); last.final_b = final_b;
    last.burned = burned_in_gauss; last.residual = residual; last.image_pred = image_pred;
    hgh_launch<38, 38, 38, CT_PLAIN, true>(st, last);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
