// The backward of the hourglass CNN of the colour aggregation network (C ABI: include/ibgs_hg_train.h, which holds the definition; Python:
// ibgs_amd/hourglass.py `hourglass_backward` / `hourglass_train`).  The forward of a training step is ibgs_hg_forward (hourglass.hip) on an arena the
// caller keeps; this unit reads its six stages and never writes them.
//
// CONTRACT  Float32, a tolerance against a float64 restatement (tests/hourglass_bwd_ref.py).  The same arguments give the same bits on
// every call and stream: nothing is summed in an order that depends on scheduling -- a weight gradient is one partial per workgroup, summed by a last pass
// in the order of the workgroups -- and grad_x does not depend on whether parameter gradients are asked for.
//
// THE PRODUCTS are v_mfma_f32_16x16x4_f32, lane l = (column l & 15, kq = l >> 4): the lane map of shared/conv_tile.h.
//   hgb_conv_kernel<CA, CB, COUT, TAPS, TRANS>  the implicit GEMM of the forward on the 16 x 16 tile of that header (M = output channels, N = 16 pixels of a
//     row, K = (channel, tap)), for 3 x 3 and 1 x 1 layers.  TRANS reads the weight transposed and flipped: the staged input is G, k = TAPS (output channel
//     of the layer) + (TAPS - 1 - tap), M = the layer's input channels (a window [m0, m0 + COUT) of them: the two halves of a concatenation are two
//     launches), no bias.  It serves the recomputed dec1 and fuse_input (forward form), final^T, fuse_input^T and the seven 3 x 3 input gradients.  The
//     epilogue adds a plane (enc1: the head's g_x), the burned-in image gradient, and applies the destination's ReLU mask.
//   hgb_wgrad_kernel<CA, CB, COUT, MODE, TAPS>  a GEMM whose K is the pixels: M = output channels (rows: G), N = (input channel, tap) and one column of ones
//     (the bias gradient), four pixels of a row per instruction.  A workgroup owns a slice of N (8 input channels of a 3 x 3 layer, 4 where Cout is 38; 40 or 20 of a 1 x 1 one) and a
//     strip of 8 x 16 tiles; it walks the strip with the sums in registers (a wave takes two rows of each tile: a chain on the matrix cores runs over one row, 16 pixels, and is
//     then added to a sum in double), adds its four waves through LDS in wave order (in double, rounded once) and writes one partial.  hgb_wsum_kernel adds the partials of a layer in strip order, in double too.  The layer's input is read plain, pooled or
//     upsampled while it is staged, as the forward reads it: no concatenated, pooled or upsampled tensor exists.
//   hgb_unpool_kernel, hgb_unup_kernel, hgb_add_kernel  the routing (pool^T with the skip sum and mask, up^T with the mask, g = g_res + g_ip): plain VALU,
//     gathers in a fixed order.
// STAGING keeps the forward's discipline (shared/conv_tile.h states it, and the rule by which a layer's source is read): coordinates are clamped into the
// frame before an offset is formed, every load is unconditional and from a valid address, and what lies outside the frame or past the last channel is
// replaced by zero afterwards.
#include "common.h"
#include "shared/hg_net.h"
#include "shared/conv_tile.h"
#include "../../include/ibgs_hourglass.h"
#include "../../include/ibgs_hg_train.h"

namespace ibgs {

constexpr int HGB_THREADS = CT_THREADS;              // of every kernel here; hgb_conv_kernel's tile is conv_tile.h's
constexpr int HGB_CHUNK = 8;                         // input channels per staged chunk
constexpr int HGB_WT_H = 8;                          // hgb_wgrad_kernel: rows of a tile of its strip
constexpr int HGB_WT_W = 16;                         // ... and columns
constexpr int HGB_MAX_STRIPS = 128;                  // strips (partials) per weight gradient, at most
constexpr int HGB_MIN_STRIP_TILES = 2;               // tiles of a strip, at least
constexpr int HGB_GPLANE = HGB_WT_H * HGB_WT_W + 4;  // floats per staged channel of G: the 64 lanes of a read fall into 64 banks

// ---- the 16 x 16-tile implicit GEMM ----------------------------------------------------------------------------------------------------------------------
struct HgbConv {
    const float* a; const float* b;          // the input's planes ([a | b] along the channels) of h x w
    const float* weight; const float* bias;  // the layer's weight in nn.Conv2d layout; its bias (forward form) or null
    int wcin, m0;                            // TRANS: the weight's second dimension, and the first of its input channels this launch computes
    float* out;                              // COUT planes of h x w
    const float* add;                        // null, or COUT planes added to the product (may be `out`: an element is read and written by one thread)
    const float* tail; float tail_scale;     // null, or 3 planes: out[COUT - 3 + c] += tail_scale * tail[c]
    const float* mask;                       // null, or COUT planes: the result is zero where mask <= 0
    int relu;
    int h, w;
};

template <int CA, int CB, int COUT, int TAPS, bool TRANS>
__global__ void __launch_bounds__(HGB_THREADS, 2) hgb_conv_kernel(const HgbConv a)
{
    constexpr int CIN = CA + CB, MT = (COUT + 15) / 16, COUTP = MT * 16;
    constexpr int RUN = HGB_CHUNK * TAPS, STEPS = RUN / 4;
    constexpr int PAD = TAPS == 9 ? 1 : 0, WIN = CT_TILE + 2 * PAD, PLANE = TAPS == 9 ? CT_PLANE : 272;          // (both 16 mod 32)
    constexpr int WROW = COUTP + 1;
    static_assert(TAPS == 9 || TAPS == 1, "3 x 3 or 1 x 1");
    static_assert(WIN * WIN <= PLANE && PLANE % 32 == 16 && RUN % 4 == 0, "the staged window");
    __shared__ float s_in[HGB_CHUNK * PLANE];
    __shared__ float s_w[RUN * WROW];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int tx0 = blockIdx.x * CT_TILE, ty0 = blockIdx.y * CT_TILE;
    const int h = a.h, w = a.w;
    const size_t plane = (size_t)h * (size_t)w;

    // sum: the bias and the finished groups.  A multiply-add chain on the matrix cores runs over ONE group of two k-steps (eight products) from zero and is
    // then added to sum: a chain of 342 or 684 products in one accumulator loses about four times as much to rounding as these short ones and their sum
    ct_f32x4 sum[MT][CT_ROWS];
    ct_start<COUT>(sum, a.bias, kq);
    int off[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int kk = 4 * s + kq, cl = kk / TAPS, t = kk - TAPS * cl, dy = t / 3;
        off[s] = cl * PLANE + dy * WIN + (t - 3 * dy);
    }
    const int window_at = wave * CT_ROWS * WIN + col;

#pragma unroll 1
    for (int c0 = 0; c0 < CIN; c0 += HGB_CHUNK) {          // (uniform over the workgroup: every thread reaches the barriers)
        __syncthreads();          // the chunk before has been read
        for (int p = threadIdx.x; p < WIN * WIN; p += HGB_THREADS) {
            const int yy = p / WIN, xx = p - yy * WIN, y = ty0 + yy - PAD, x = tx0 + xx - PAD;
            const bool in = y >= 0 && y < h && x >= 0 && x < w;
            const int o = ct_source_offset<CT_PLAIN>(y, x, h, w, h, w);
#pragma unroll
            for (int cl = 0; cl < HGB_CHUNK; ++cl) {
                const int c = c0 + cl, cc = c < CIN ? c : CIN - 1;
                const float* const base = (CB == 0 || cc < CA) ? a.a + (size_t)cc * plane : a.b + (size_t)(cc - CA) * plane;
                const float v = base[o];
                s_in[cl * PLANE + p] = (c < CIN && in) ? v : 0.0f;
            }
        }
        for (int i = threadIdx.x; i < COUTP * RUN; i += HGB_THREADS) {
            const int m = i / RUN, j = i - m * RUN, cl = j / TAPS, t = j - cl * TAPS, c = c0 + cl;
            const int mc = min(m, COUT - 1), cc = min(c, CIN - 1);
            const size_t at = TRANS ? ((size_t)cc * a.wcin + a.m0 + mc) * TAPS + (TAPS - 1 - t) : ((size_t)mc * CIN + cc) * TAPS + t;
            const float v = a.weight[at];
            s_w[j * WROW + m] = (m < COUT && c < CIN) ? v : 0.0f;
        }
        __syncthreads();
        const int limit = (min(CIN - c0, HGB_CHUNK) * TAPS + 3) / 4;          // k-steps this chunk holds (what lies past them is zeros)
#pragma unroll
        for (int s0 = 0; s0 < STEPS; s0 += 2) {
            if (s0 < limit) {
                ct_f32x4 acc[MT][CT_ROWS];
#pragma unroll
                for (int s = s0; s < s0 + 2; ++s) {
                    {          // (a group's second step past `limit` multiplies staged zeros)
                        float av[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) av[mt] = s_w[(4 * s + kq) * WROW + mt * 16 + col];
#pragma unroll
                        for (int nt = 0; nt < CT_ROWS; ++nt) {
                            const float bv = s_in[window_at + nt * WIN + off[s]];
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = ct_mfma(av[mt], bv, s == s0 ? ct_f32x4{0.0f, 0.0f, 0.0f, 0.0f} : acc[mt][nt]);
                        }
                    }
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < CT_ROWS; ++nt) sum[mt][nt] += acc[mt][nt];
            }
        }
    }

    // (the output walk is written out, not ct_for_each_output: with the epilogue as its callback the 19 -> 9 input gradient takes 74 registers for 72 and
    // loses a wave per SIMD)
    const int x = tx0 + col;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt) {
            const int y = ty0 + wave * CT_ROWS + nt;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = mt * 16 + kq * 4 + r;
                if (ch < COUT && y < h && x < w) {
                    const size_t p = (size_t)y * w + x, at = (size_t)ch * plane + p;
                    float v = sum[mt][nt][r];
                    if (a.add) v += a.add[at];
                    if (a.tail && ch >= COUT - 3) v = fmaf(a.tail_scale, a.tail[(size_t)(ch - (COUT - 3)) * plane + p], v);
                    if (a.relu) v = v > 0.0f ? v : 0.0f;
                    if (a.mask) v = a.mask[at] > 0.0f ? v : 0.0f;
                    a.out[at] = v;
                }
            }
        }
}

// ---- the weight gradients ----------------------------------------------------------------------------------------------------------------------------------
struct HgbWgrad {
    const float* g;                          // COUT planes of h x w: the layer's pre-activation gradient
    const float* a; const float* b;          // the layer's input [a | b]; a holds planes of hs x ws, read as MODE says
    float* partial;                          // (strips, slices, COUT padded, columns padded)
    int h, w, hs, ws;
    int tiles_x, ntiles, strip_tiles;
};

template <int CIN, int COUT, int TAPS> struct HgbSlice {
    // input channels of a slice: with three rows of result tiles (Cout 38) three columns of them, 15 with fewer -- the sums are kept in double, and 15 x 3 spill
    static constexpr int CI = TAPS == 9 ? (COUT > 32 ? 4 : 8) : (COUT > 32 ? 20 : 40);
    static constexpr int SLICES = (CIN + CI - 1) / CI;
    static constexpr int COLS = CI * TAPS + 1;                           // the slice's (channel, tap) columns and the column of ones
    static constexpr int NT = (COLS + 15) / 16, COLSP = NT * 16;
};

template <int CA, int CB, int COUT, int MODE, int TAPS>
__global__ void __launch_bounds__(HGB_THREADS, 2) hgb_wgrad_kernel(const HgbWgrad a)
{
    using S = HgbSlice<CA + CB, COUT, TAPS>;
    constexpr int CIN = CA + CB, MT = (COUT + 15) / 16, COUTP = MT * 16, NT = S::NT, CI = S::CI;
    constexpr int PAD = TAPS == 9 ? 1 : 0, WINW = HGB_WT_W + 2 * PAD, WINH = HGB_WT_H + 2 * PAD, IPL = WINW * WINH;
    constexpr int ROWS = HGB_WT_H / 4;          // rows of a tile per wave
    static_assert(CB == 0 || MODE == CT_PLAIN, "a second input is read plain, at the first one's resolution");
    constexpr int G_WORDS = COUTP * HGB_GPLANE, I_WORDS = CI * IPL, RED_WORDS = 2 * 4 * NT * 256;          // the last: one row of result tiles of the four waves, in double
    __shared__ __attribute__((aligned(16))) float s_mem[G_WORDS + I_WORDS > RED_WORDS ? G_WORDS + I_WORDS : RED_WORDS];
    float* const s_g = s_mem;
    float* const s_i = s_mem + G_WORDS;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int slice = blockIdx.x, c0 = slice * CI;
    const int h = a.h, w = a.w;
    const size_t plane = (size_t)h * (size_t)w, plane_a = (size_t)a.hs * (size_t)a.ws;

    for (int i = threadIdx.x; i < (COUTP - COUT) * HGB_GPLANE; i += HGB_THREADS) s_g[COUT * HGB_GPLANE + i] = 0.0f;          // the padding rows, once

    // column n of this lane in tile nt: (channel of the slice, tap) as an offset into the staged window, the column of ones, or nothing
    int boff[NT], bkind[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = nt * 16 + col;
        bkind[nt] = n < CI * TAPS ? 0 : (n == CI * TAPS ? 1 : 2);
        const int nc = n < CI * TAPS ? n : 0, cl = nc / TAPS, t = nc - cl * TAPS, dy = t / 3;
        boff[nt] = cl * IPL + dy * WINW + (t - 3 * dy);
    }
    // tot: the sums over the strip, in double.  A multiply-add chain on the matrix cores runs over ONE row of a tile (16 pixels) from zero and is then added to
    // tot: a float32 chain over the strip's pixels loses several ulp of its largest partial sum, which for a bias gradient is many ulp of the result
    double tot[MT][NT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) tot[mt][nt][r] = 0.0;

    const int first = blockIdx.y * a.strip_tiles, last = min(first + a.strip_tiles, a.ntiles);
    for (int tile = first; tile < last; ++tile) {          // (uniform over the workgroup)
        const int tyi = tile / a.tiles_x, ty0 = tyi * HGB_WT_H, tx0 = (tile - tyi * a.tiles_x) * HGB_WT_W;
        __syncthreads();          // the tile before has been read
        for (int i = threadIdx.x; i < COUT * HGB_WT_H * HGB_WT_W; i += HGB_THREADS) {
            const int ch = i / (HGB_WT_H * HGB_WT_W), p = i - ch * (HGB_WT_H * HGB_WT_W), yy = p / HGB_WT_W, xx = p - yy * HGB_WT_W;
            const int y = ty0 + yy, x = tx0 + xx;
            const float v = a.g[(size_t)ch * plane + (size_t)min(y, h - 1) * w + min(x, w - 1)];
            s_g[ch * HGB_GPLANE + p] = (y < h && x < w) ? v : 0.0f;
        }
        for (int i = threadIdx.x; i < CI * IPL; i += HGB_THREADS) {
            const int cl = i / IPL, p = i - cl * IPL, yy = p / WINW, xx = p - yy * WINW;
            const int y = ty0 + yy - PAD, x = tx0 + xx - PAD, c = c0 + cl, cc = min(c, CIN - 1);
            const bool in = c < CIN && y >= 0 && y < h && x >= 0 && x < w;
            const float* const base = (CB == 0 || cc < CA) ? a.a + (size_t)cc * plane_a : a.b + (size_t)(cc - CA) * plane_a;
            const float v = ct_read<MODE>(base + ct_source_offset<MODE>(y, x, h, w, a.hs, a.ws), a.ws);
            s_i[i] = in ? v : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int yy = wave * ROWS + rr;
            ct_f32x4 acc[MT][NT];
#pragma unroll
            for (int gx = 0; gx < HGB_WT_W / 4; ++gx) {
                const int px = 4 * gx + kq;
                float av[MT], bv[NT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[mt] = s_g[(mt * 16 + col) * HGB_GPLANE + yy * HGB_WT_W + px];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float v = s_i[boff[nt] + yy * WINW + px];
                    bv[nt] = bkind[nt] == 0 ? v : (bkind[nt] == 1 ? 1.0f : 0.0f);
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = ct_mfma(av[mt], bv[nt], gx == 0 ? ct_f32x4{0.0f, 0.0f, 0.0f, 0.0f} : acc[mt][nt]);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tot[mt][nt][r] += (double)acc[mt][nt][r];
        }
    }
    // the four waves' sums are added in wave order through LDS, one row of result tiles at a time, and rounded once: the workgroup's partial
    float* const out = a.partial + ((size_t)blockIdx.y * S::SLICES + slice) * (size_t)(COUTP * S::COLSP);
    double* const s_red = reinterpret_cast<double*>(s_mem);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        __syncthreads();          // the last tile, or the row before, has been read
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_red[((wave * NT + nt) * 4 + r) * 64 + lane] = tot[mt][nt][r];
        __syncthreads();
        for (int i = threadIdx.x; i < NT * 256; i += HGB_THREADS) {
            const double sum = ((s_red[i] + s_red[NT * 256 + i]) + s_red[2 * NT * 256 + i]) + s_red[3 * NT * 256 + i];
            const int l = i & 63, r = (i >> 6) & 3, nt = i >> 8;
            out[(mt * 16 + (l >> 4) * 4 + r) * S::COLSP + nt * 16 + (l & 15)] = (float)sum;
        }
    }
}

// dW[o, i, t] and db[o]: the partials of the strips, in strip order
__global__ void __launch_bounds__(HGB_THREADS) hgb_wsum_kernel(const float* __restrict__ partial, int strips, int slices, int coutp, int colsp, int ci, int taps,
                                                               int cout, int cin, float* __restrict__ dw, float* __restrict__ db)
{
    const int e = blockIdx.x * HGB_THREADS + threadIdx.x, nw = cout * cin * taps;
    if (e >= nw + cout) return;
    int o, slice, n;
    if (e < nw) {
        o = e / (cin * taps);
        const int rest = e - o * (cin * taps), i = rest / taps, t = rest - i * taps;
        slice = i / ci;
        n = (i - slice * ci) * taps + t;
    } else {
        o = e - nw; slice = 0; n = ci * taps;
    }
    const size_t block = (size_t)coutp * colsp;
    const float* q = partial + (size_t)slice * block + (size_t)o * colsp + n;
    double sum = 0.0;          // (the strips' partials in double, rounded once)
    for (int s = 0; s < strips; ++s) sum += (double)q[(size_t)s * slices * block];
    if (e < nw) dw[e] = (float)sum;
    else db[o] = (float)sum;
}

// ---- routing -----------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HGB_THREADS) hgb_add_kernel(const float* __restrict__ p, const float* __restrict__ q, float* __restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * HGB_THREADS + threadIdx.x;
    if (i < n) out[i] = p[i] + q[i];
}

// out[c, y, x] = (add[c, y, x] + (g_pool[c, y / 2, x / 2] if (y, x) is the first maximum of its window of t, else 0)) [t[c, y, x] > 0].  t: planes of h x w,
// g_pool: planes of h2 x w2 = (h / 2) x (w / 2).  `out` may be `add`.
__global__ void __launch_bounds__(HGB_THREADS) hgb_unpool_kernel(const float* __restrict__ g_pool, const float* __restrict__ t, const float* add, float* out, int channels,
                                                                 int h, int w, int h2, int w2)
{
    const size_t plane = (size_t)h * (size_t)w, i = (size_t)blockIdx.x * HGB_THREADS + threadIdx.x;
    if (i >= plane * channels) return;
    const int c = (int)(i / plane), p = (int)(i - (size_t)c * plane), y = p / w, x = p - y * w;
    const int py = y >> 1, px = x >> 1, pyc = min(py, h2 - 1), pxc = min(px, w2 - 1);
    const float* const q = t + (size_t)c * plane + (size_t)(2 * pyc) * w + 2 * pxc;          // 2 pyc + 1 <= 2 h2 - 1 <= h - 1
    const float v[4] = {q[0], q[1], q[w], q[w + 1]};
    int best = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (v[k] > v[best]) best = k;
    const float routed = g_pool[(size_t)c * ((size_t)h2 * w2) + (size_t)pyc * w2 + pxc];
    const bool mine = py < h2 && px < w2 && best == 2 * (y & 1) + (x & 1);
    const float sum = add[i] + (mine ? routed : 0.0f);
    out[i] = t[i] > 0.0f ? sum : 0.0f;
}

// out[c, Y, X] = (the sum of g[c, y, x] over the (y, x) of the h x w frame whose nearest source is (Y, X), rows then columns) [t[c, Y, X] > 0].  t, out: planes of hl x wl.
__global__ void __launch_bounds__(HGB_THREADS) hgb_unup_kernel(const float* __restrict__ g, const float* __restrict__ t, float* __restrict__ out, int channels, int h, int w,
                                                               int hl, int wl)
{
    const size_t plane_l = (size_t)hl * (size_t)wl, i = (size_t)blockIdx.x * HGB_THREADS + threadIdx.x;
    if (i >= plane_l * channels) return;
    const int c = (int)(i / plane_l), p = (int)(i - (size_t)c * plane_l), Y = p / wl, X = p - Y * wl;
    // y hl div h == Y  <=>  ceil(Y h / hl) <= y < ceil((Y + 1) h / hl)   (y hl div h < hl: the rule's clamp never acts)
    const int y0 = (int)(((int64_t)Y * h + hl - 1) / hl), y1 = min((int)(((int64_t)(Y + 1) * h + hl - 1) / hl), h);
    const int x0 = (int)(((int64_t)X * w + wl - 1) / wl), x1 = min((int)(((int64_t)(X + 1) * w + wl - 1) / wl), w);
    const float* const q = g + (size_t)c * ((size_t)h * w);
    float sum = 0.0f;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) sum += q[(size_t)y * w + x];
    out[i] = t[i] > 0.0f ? sum : 0.0f;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
struct HgbStrips {          // how a frame of h x w is cut into strips of tiles
    int tiles_x, ntiles, strip_tiles, strips;
    HgbStrips(int h, int w)
    {
        tiles_x = (w + HGB_WT_W - 1) / HGB_WT_W;
        ntiles = tiles_x * ((h + HGB_WT_H - 1) / HGB_WT_H);
        strip_tiles = (ntiles + HGB_MAX_STRIPS - 1) / HGB_MAX_STRIPS;
        if (strip_tiles < HGB_MIN_STRIP_TILES) strip_tiles = HGB_MIN_STRIP_TILES;
        strips = (ntiles + strip_tiles - 1) / strip_tiles;
    }
};

// the floats of the partials of the weight gradients of layers I .. of HG_LAYERS, each at its own resolution: the most any of them takes
template <int I = 0>
static size_t hgb_partial_floats(const int (&h)[3], const int (&w)[3])
{
    if constexpr (I == HG_LAYER_COUNT) return 0;
    else {
        constexpr HgLayer L = HG_LAYERS[I];
        using S = HgbSlice<L.ca + L.cb, L.cout, L.side * L.side>;
        const size_t mine = (size_t)HgbStrips(h[L.level], w[L.level]).strips * S::SLICES * (size_t)(((L.cout + 15) / 16) * 16 * S::COLSP);
        const size_t rest = hgb_partial_floats<I + 1>(h, w);
        return mine > rest ? mine : rest;
    }
}

struct HgbScratch {          // the arena of the header, in its order
    float *A, *B, *C, *D, *g, *Gd2, *Gu2, *E2, *Iup2, *Ienc2, *Gb, *Ienc3, *partial;
    static HgbScratch carve(char* base, int H, int W, size_t* total)
    {
        const int h[3] = {H, H / 2, H / 2 / 2}, w[3] = {W, W / 2, W / 2 / 2};
        const size_t p1 = (size_t)H * W, p2 = (size_t)h[1] * w[1], p4 = (size_t)h[2] * w[2];
        HgbScratch s;
        Carver c(base);
        s.A = c.take<float>(38 * p1);
        s.B = c.take<float>(38 * p1);
        s.C = c.take<float>(38 * p1);
        s.D = c.take<float>(38 * p1);
        s.g = c.take<float>(3 * p1);
        s.Gd2 = c.take<float>(19 * p2);
        s.Gu2 = c.take<float>(19 * p2);
        s.E2 = c.take<float>(19 * p2);
        s.Iup2 = c.take<float>(9 * p2);
        s.Ienc2 = c.take<float>(38 * p2);
        s.Gb = c.take<float>(9 * p4);
        s.Ienc3 = c.take<float>(19 * p4);
        s.partial = c.take<float>(hgb_partial_floats(h, w));
        if (total) *total = hg_carved_bytes(c, base);
        return s;
    }
};

template <int CA, int CB, int COUT, int TAPS, bool TRANS>
static void hgb_conv(hipStream_t st, const float* in_a, const float* in_b, const float* weight, const float* bias, int wcin, int m0, float* out, const float* add,
                     const float* tail, float tail_scale, const float* mask, bool relu, int h, int w)
{
    HgbConv a = {};
    a.a = in_a; a.b = in_b; a.weight = weight; a.bias = bias; a.wcin = wcin; a.m0 = m0; a.out = out; a.add = add; a.tail = tail; a.tail_scale = tail_scale;
    a.mask = mask; a.relu = relu ? 1 : 0; a.h = h; a.w = w;
    const dim3 grid((unsigned)((w + CT_TILE - 1) / CT_TILE), (unsigned)((h + CT_TILE - 1) / CT_TILE));
    hipLaunchKernelGGL((hgb_conv_kernel<CA, CB, COUT, TAPS, TRANS>), grid, dim3(HGB_THREADS), 0, st, a);
}

// the input gradient of a 3 x 3 layer whose weight is (CL, wcin, 3, 3): channels [m0, m0 + COUT) of it, from G (CL planes)
template <int CL, int COUT>
static void hgb_dgrad(hipStream_t st, const float* G, const float* weight, int wcin, int m0, float* out, const float* add, const float* mask, int h, int w)
{
    hgb_conv<CL, 0, COUT, 9, true>(st, G, nullptr, weight, nullptr, wcin, m0, out, add, nullptr, 0.0f, mask, false, h, w);
}

template <int CA, int CB, int COUT, int MODE, int TAPS>
static void hgb_wgrad(hipStream_t st, const float* G, const float* in_a, const float* in_b, float* partial, float* dw, float* db, int h, int w, int hs, int ws)
{
    using S = HgbSlice<CA + CB, COUT, TAPS>;
    const HgbStrips strips(h, w);
    HgbWgrad a = {};
    a.g = G; a.a = in_a; a.b = in_b; a.partial = partial; a.h = h; a.w = w; a.hs = hs; a.ws = ws;
    a.tiles_x = strips.tiles_x; a.ntiles = strips.ntiles; a.strip_tiles = strips.strip_tiles;
    hipLaunchKernelGGL((hgb_wgrad_kernel<CA, CB, COUT, MODE, TAPS>), dim3(S::SLICES, (unsigned)strips.strips), dim3(HGB_THREADS), 0, st, a);
    const int n = COUT * (CA + CB) * TAPS + COUT;
    hipLaunchKernelGGL(hgb_wsum_kernel, dim3(grid_for((size_t)n, HGB_THREADS)), dim3(HGB_THREADS), 0, st, partial, strips.strips, S::SLICES, ((COUT + 15) / 16) * 16,
                       S::COLSP, S::CI, TAPS, COUT, CA + CB, dw, db);
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_hgb_required_scratch(int64_t H, int64_t W)
{
    size_t total = 0;
    if (!hg_shape_ok(nullptr, H, W)) return 0;
    HgbScratch::carve(nullptr, (int)H, (int)W, &total);
    return total;
}

int32_t ibgs_hgb_backward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                          const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                          const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                          const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                          float burned_in_gauss, const void* stages_arena, const float* grad_residual, const float* grad_image_pred, float* grad_x,
                          float* grad_enc1_w, float* grad_enc1_b, float* grad_enc2_w, float* grad_enc2_b, float* grad_enc3_w, float* grad_enc3_b,
                          float* grad_up2_conv_w, float* grad_up2_conv_b, float* grad_dec2_w, float* grad_dec2_b, float* grad_up1_conv_w,
                          float* grad_up1_conv_b, float* grad_dec1_w, float* grad_dec1_b, float* grad_fuse_input_w, float* grad_fuse_input_b,
                          float* grad_final_w, float* grad_final_b, void* scratch, size_t scratch_bytes)
{
    const char* const who = "hgb_backward";
    size_t need = 0;
    if (!hg_shape_ok(who, H, W)) return -IBGS_ERR_INVALID;
    if (!x) { set_error("%s: null input", who); return -IBGS_ERR_INVALID; }
    const float* const params[18] = {enc1_w, enc1_b, enc2_w, enc2_b, enc3_w, enc3_b, up2_conv_w, up2_conv_b, dec2_w, dec2_b, up1_conv_w, up1_conv_b, dec1_w, dec1_b,
                                     fuse_input_w, fuse_input_b, final_w, final_b};
    float* const grads[18] = {grad_enc1_w, grad_enc1_b, grad_enc2_w, grad_enc2_b, grad_enc3_w, grad_enc3_b, grad_up2_conv_w, grad_up2_conv_b, grad_dec2_w, grad_dec2_b,
                              grad_up1_conv_w, grad_up1_conv_b, grad_dec1_w, grad_dec1_b, grad_fuse_input_w, grad_fuse_input_b, grad_final_w, grad_final_b};
    if (!hg_params_ok(who, params)) return -IBGS_ERR_INVALID;
    if (!stages_arena) { set_error("%s: null stages arena", who); return -IBGS_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(stages_arena) & 127) { set_error("%s: stages arena is not 128-byte aligned", who); return -IBGS_ERR_INVALID; }
    if (!grad_residual && !grad_image_pred) { set_error("%s: null upstream: grad_residual and grad_image_pred are both null", who); return -IBGS_ERR_INVALID; }
    int given = 0;
    for (int i = 0; i < 18; ++i) given += grads[i] != nullptr;
    if (given != 0 && given != 18) {
        const int i = hg_first_null(grads);
        set_error("%s: null gradients: %s's %s (the eighteen are given together or not at all)", who, HG_LAYERS[i / 2].name, hg_part(i));
        return -IBGS_ERR_INVALID;
    }
    const bool want_params = given == 18, want_x = grad_x != nullptr;
    if (!want_params && !want_x) { set_error("%s: null outputs: neither grad_x nor the parameter gradients are asked for", who); return -IBGS_ERR_INVALID; }
    const HgbScratch sc = HgbScratch::carve(static_cast<char*>(scratch), H, W, &need);
    if (!arena_ok(who, "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    Carver forward_arena(static_cast<char*>(const_cast<void*>(stages_arena)));          // the arena of ibgs_hg_forward, read only
    const HgStages<const float> sg = hg_carve_stages<const float>(forward_arena, (size_t)H, (size_t)W, 1);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2;
    const size_t p1 = (size_t)H * W, p2 = (size_t)H2 * W2, p4 = (size_t)H4 * W4;

    // the head: g, d1 -> A, f -> B, g_f -> C, G_d1 -> D, g_x
    const float* g = grad_residual ? grad_residual : grad_image_pred;
    if (grad_residual && grad_image_pred) {
        hipLaunchKernelGGL(hgb_add_kernel, dim3(grid_for(3 * p1, HGB_THREADS)), dim3(HGB_THREADS), 0, st, grad_residual, grad_image_pred, sc.g, 3 * p1);
        g = sc.g;
    }
    hgb_conv<38, 38, 38, 9, false>(st, sg.u1, sg.e1, dec1_w, dec1_b, 0, 0, sc.A, nullptr, nullptr, 0.0f, nullptr, true, H, W);
    hgb_conv<38, 38, 38, 1, false>(st, sc.A, x, fuse_input_w, fuse_input_b, 0, 0, sc.B, nullptr, nullptr, 0.0f, nullptr, true, H, W);
    hgb_conv<3, 0, 38, 1, true>(st, g, nullptr, final_w, nullptr, 38, 0, sc.C, nullptr, nullptr, 0.0f, sc.B, false, H, W);
    hgb_conv<38, 0, 38, 1, true>(st, sc.C, nullptr, fuse_input_w, nullptr, 76, 0, sc.D, nullptr, nullptr, 0.0f, sc.A, false, H, W);
    if (want_x) hgb_conv<38, 0, 38, 1, true>(st, sc.C, nullptr, fuse_input_w, nullptr, 76, 38, grad_x, nullptr, grad_image_pred, burned_in_gauss, nullptr, false, H, W);
    if (want_params) {
        hgb_wgrad<38, 0, 3, CT_PLAIN, 1>(st, g, sc.B, nullptr, sc.partial, grad_final_w, grad_final_b, H, W, H, W);
        hgb_wgrad<38, 38, 38, CT_PLAIN, 1>(st, sc.C, sc.A, x, sc.partial, grad_fuse_input_w, grad_fuse_input_b, H, W, H, W);
        hgb_wgrad<38, 38, 38, CT_PLAIN, 9>(st, sc.D, sg.u1, sg.e1, sc.partial, grad_dec1_w, grad_dec1_b, H, W, H, W);
    }
    // dec1: G_u1 -> A, g_e1a -> B
    hgb_dgrad<38, 38>(st, sc.D, dec1_w, 76, 0, sc.A, nullptr, sg.u1, H, W);
    hgb_dgrad<38, 38>(st, sc.D, dec1_w, 76, 38, sc.B, nullptr, nullptr, H, W);
    // up1_conv: its g_I -> C, G_d2
    if (want_params) hgb_wgrad<19, 0, 38, CT_UP, 9>(st, sc.A, sg.d2, nullptr, sc.partial, grad_up1_conv_w, grad_up1_conv_b, H, W, H2, W2);
    hgb_dgrad<38, 19>(st, sc.A, up1_conv_w, 19, 0, sc.C, nullptr, nullptr, H, W);
    hipLaunchKernelGGL(hgb_unup_kernel, dim3(grid_for(19 * p2, HGB_THREADS)), dim3(HGB_THREADS), 0, st, sc.C, sg.d2, sc.Gd2, 19, H, W, H2, W2);
    // dec2: G_u2, g_e2a -> E2
    if (want_params) hgb_wgrad<19, 19, 19, CT_PLAIN, 9>(st, sc.Gd2, sg.u2, sg.e2, sc.partial, grad_dec2_w, grad_dec2_b, H2, W2, H2, W2);
    hgb_dgrad<19, 19>(st, sc.Gd2, dec2_w, 38, 0, sc.Gu2, nullptr, sg.u2, H2, W2);
    hgb_dgrad<19, 19>(st, sc.Gd2, dec2_w, 38, 19, sc.E2, nullptr, nullptr, H2, W2);
    // up2_conv: G_b
    if (want_params) hgb_wgrad<9, 0, 19, CT_UP, 9>(st, sc.Gu2, sg.b, nullptr, sc.partial, grad_up2_conv_w, grad_up2_conv_b, H2, W2, H4, W4);
    hgb_dgrad<19, 9>(st, sc.Gu2, up2_conv_w, 9, 0, sc.Iup2, nullptr, nullptr, H2, W2);
    hipLaunchKernelGGL(hgb_unup_kernel, dim3(grid_for(9 * p4, HGB_THREADS)), dim3(HGB_THREADS), 0, st, sc.Iup2, sg.b, sc.Gb, 9, H2, W2, H4, W4);
    // enc3: G_e2 (in E2)
    if (want_params) hgb_wgrad<19, 0, 9, CT_POOL, 9>(st, sc.Gb, sg.e2, nullptr, sc.partial, grad_enc3_w, grad_enc3_b, H4, W4, H2, W2);
    hgb_dgrad<9, 19>(st, sc.Gb, enc3_w, 19, 0, sc.Ienc3, nullptr, nullptr, H4, W4);
    hipLaunchKernelGGL(hgb_unpool_kernel, dim3(grid_for(19 * p2, HGB_THREADS)), dim3(HGB_THREADS), 0, st, sc.Ienc3, sg.e2, sc.E2, sc.E2, 19, H2, W2, H4, W4);
    // enc2: G_e1 (in B)
    if (want_params) hgb_wgrad<38, 0, 19, CT_POOL, 9>(st, sc.E2, sg.e1, nullptr, sc.partial, grad_enc2_w, grad_enc2_b, H2, W2, H, W);
    hgb_dgrad<19, 38>(st, sc.E2, enc2_w, 38, 0, sc.Ienc2, nullptr, nullptr, H2, W2);
    hipLaunchKernelGGL(hgb_unpool_kernel, dim3(grid_for(38 * p1, HGB_THREADS)), dim3(HGB_THREADS), 0, st, sc.Ienc2, sg.e1, sc.B, sc.B, 38, H, W, H2, W2);
    // enc1
    if (want_params) hgb_wgrad<38, 0, 38, CT_PLAIN, 9>(st, sc.B, x, nullptr, sc.partial, grad_enc1_w, grad_enc1_b, H, W, H, W);
    if (want_x) hgb_dgrad<38, 38>(st, sc.B, enc1_w, 38, 0, grad_x, grad_x, nullptr, H, W);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
