// The hourglass CNN of the reference's colour aggregation network on the device (C ABI: include/ibgs_hourglass.h; Python: ibgs_amd/hourglass.py): the forward
// of ConvDecoderAE(38) (color_aggregation_network.py:6-68) for test-time rendering -- nine convolutions, two pools, two nearest upsamples, three
// concatenations and the image_pred expression of fuse_color -- as seven launches of ONE templated 3 x 3 implicit-GEMM kernel.  No concatenation, pooled or
// upsampled tensor is ever materialised, and the last launch carries the two 1 x 1 convolutions: d1 and f never reach memory.
//
// CONTRACT (the definition is in the header)
//   Every output element is an f32 multiply-add chain on the matrix cores started from the bias: over k = 9 (input channel) + tap in the order of the weights'
//   layout for a 3 x 3 convolution, and over the input channel (in the order the registers give: below) for the 1 x 1 ones.  The contract is a tolerance
//   against a float64 restatement (tests/hourglass_ref.py), not this order.  The same arguments give the same bits on every call and
//   stream: no atomics, nothing crosses a workgroup.
//   image_pred = burned * x[35 + c] + residual with the product rounded first (no contraction): torch's expression on the returned residual, bit for bit.
//
// THE PRODUCTS are v_mfma_f32_16x16x4_f32 (exact f32: bit for bit a k-ordered fmaf chain).  Output channels are the M dimension, padded 38 -> 48, 19 -> 32,
// 9 -> 16 (the 32-wide form would pad 38 -> 64); 16 pixels of one row are N; K runs over k = 9 (input channel) + tap, four consecutive k per instruction
// (the order of the nn.Conv2d layout and of tests/hourglass_ref.chain_f32; K is padded to a multiple of 4 only: 342 -> 344).  The tile, its lane map (col,
// kq; register r of result tile mt is channel 16 mt + 4 kq + r of pixel col) and its staging are shared/conv_tile.h's, which lpips.hip and hgtrain.hip run
// too.  In the last launch a result tile is the next product's B operand as it stands: k-step (tile mt, register r) takes the channels 16 mt + 4 kq + r,
// and the 1 x 1 weights are staged in that (permuted) k order.
//
// KERNEL  hg_conv3_kernel<CA, CB, COUT, MODE, FUSE>: 256 threads = 4 waves per 16 x 16 output tile (a 2-D grid of tiles: nothing is capped, no workgroup
// walks the frame); a wave owns four rows of the tile and all output channels: (COUT padded / 16) x 4 accumulator tiles.  The input is [A (CA channels, read
// plain, pooled or upsampled as MODE says) | B (CB channels, read plain)].  Per chunk of 8 input channels the workgroup stages the 18 x 18 input window
// (tile and one-pixel halo; out-of-frame taps and padding channels are zeros, and no address outside a plane is formed: coordinates are clamped into the
// frame before an offset is made of them) and the chunk's weights (read from the nn.Conv2d layout in runs of 72 consecutive floats per output channel,
// stored k-major: the instruction's A layout) into LDS, then runs 18 k-steps.  A thread's loads of a chunk -- 16 window values, up to 14 weights -- are
// unconditional and issued together, ahead of the barrier that waits for the chunk before.  The staged planes are 336 floats apart (= 16 mod 32) and a
// k of the weights 49: the lanes of a half-wave read disjoint banks but for one.  The kernel keeps its chunk loop, its loads of a chunk ([a | b]) and the
// last launch's tail, its table of tap offsets and its k-steps; the window positions, the LDS stores and the output walk are the header's.
// What bounds it and what was measured: DESIGN.md section 15.
#include "common.h"
#include "shared/hg_net.h"
#include "shared/conv_tile.h"
#include "../../include/ibgs_hourglass.h"

namespace ibgs {

constexpr int HG_QC = 2;                             // groups of four input channels per staged chunk

// channel c of x (planes of h x w) at (y, x); zero outside the frame
__device__ __forceinline__ float hg_read_plain(const float* __restrict__ src, int c, int y, int x, int h, int w)
{
    if (y < 0 || y >= h || x < 0 || x >= w) return 0.0f;
    return src[(size_t)c * ((size_t)h * (size_t)w) + (size_t)y * w + x];
}

struct HgArgs {
    const float* a; const float* b;          // the two inputs ([a | b] along the channels); b may be null when CB == 0
    const float* weight; const float* bias;  // (COUT, CA + CB, 3, 3), (COUT)
    float* out;                              // COUT planes of h x w (null in the last launch)
    int h, w, hs, ws;                        // the output's resolution, and a's
    // the last launch: x (38 planes of h x w), fuse_input (38, 76), final (3, 38), the two outputs
    const float* x; const float* fuse_w; const float* fuse_b; const float* final_w; const float* final_b;
    float burned; float* residual; float* image_pred;
};

template <int CA, int CB, int COUT, int MODE, bool FUSE>
__global__ void __launch_bounds__(CT_THREADS, 2) hg_conv3_kernel(const HgArgs a)
{
    constexpr int CIN = CA + CB, KTOT = CIN * 9, MT = (COUT + 15) / 16, COUTP = MT * 16;
    constexpr int CHUNK_C = 4 * HG_QC, RUN = CHUNK_C * 9, STEPS = RUN / 4;          // channels, k and k-steps of a staged chunk
    constexpr int WROW = COUTP + 1;          // floats per k of the staged weights: consecutive k fall into different banks
    constexpr int IN_WORDS = CHUNK_C * CT_PLANE, W_WORDS = RUN * WROW;
    // the last launch's 1 x 1 weights: 12 k-steps over d1 and 10 over x for fuse_input (48 rows), 12 over f for final (16 rows)
    constexpr int FUSE_STEPS = 12 + (HG_C + 3) / 4, FIN_STEPS = 12;
    constexpr int FUSE_WORDS = FUSE ? FUSE_STEPS * 4 * 48 + FIN_STEPS * 4 * 16 : 0;
    static_assert(!FUSE || (COUT == HG_C && MT == 3), "the last launch is dec1");
    __shared__ float s_mem[IN_WORDS + W_WORDS > FUSE_WORDS ? IN_WORDS + W_WORDS : FUSE_WORDS];
    ct_lds* const s_in = (ct_lds*)s_mem;
    ct_lds* const s_w = s_in + IN_WORDS;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int tx0 = blockIdx.x * CT_TILE, ty0 = blockIdx.y * CT_TILE;
    const int h = a.h, w = a.w;

    ct_f32x4 acc[MT][CT_ROWS];
    ct_start<COUT>(acc, a.bias, kq);
    // This lane's k of step s of a chunk is 4 s + kq: its channel of the chunk and tap, as an offset into the staged window.  (The table and the k-steps that
    // read it stay in the kernel: as helpers of conv_tile.h they cost hg_conv3_kernel 0.4 - 0.8 % of its time.)
    int off[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int kk = 4 * s + kq, cl = kk / 9, t = kk - 9 * cl, dy = t / 3;
        off[s] = cl * CT_PLANE + dy * CT_WIN + (t - 3 * dy);
    }
    const int window_at = wave * CT_ROWS * CT_WIN + col;

    // A holds planes of hs x ws, read as MODE says; besides its window positions a thread stages NW elements of the weights
    static_assert(CB == 0 || MODE == CT_PLAIN, "a second input is read plain, at the first one's resolution");
    constexpr int NW = (COUTP * RUN + CT_THREADS - 1) / CT_THREADS;
    const size_t plane_a = (size_t)a.hs * (size_t)a.ws;
    int pos_off[CT_NPOS], pos_lds[CT_NPOS];
    bool pos_in[CT_NPOS];
    ct_window_positions<MODE>(pos_off, pos_lds, pos_in, tx0, ty0, h, w, a.hs, a.ws);
    float iv[CHUNK_C][CT_NPOS], wv[NW];
    auto load_chunk = [&](const int c0) {
#pragma unroll
        for (int cl = 0; cl < CHUNK_C; ++cl) {
            const int c = c0 + cl, cc = c < CIN ? c : CIN - 1;          // (uniform)
            const float* const base = (CB == 0 || cc < CA) ? a.a + (size_t)cc * plane_a : a.b + (size_t)(cc - CA) * plane_a;
#pragma unroll
            for (int r = 0; r < CT_NPOS; ++r) {
                const float v = ct_read<MODE>(base + pos_off[r], a.ws);
                iv[cl][r] = (c < CIN && pos_in[r]) ? v : 0.0f;
            }
        }
#pragma unroll
        for (int n = 0; n < NW; ++n) {          // runs of RUN consecutive floats of one output channel's row
            const int i = (int)threadIdx.x + n * CT_THREADS, m = i / RUN, j = i - m * RUN, kk = c0 * 9 + j;
            const float v = a.weight[(size_t)min(m, COUT - 1) * KTOT + min(kk, KTOT - 1)];
            wv[n] = (m < COUT && kk < KTOT) ? v : 0.0f;
        }
    };
    auto run_steps = [&](const int limit) {
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            if (s < limit) {
                float av[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[mt] = s_w[(4 * s + kq) * WROW + mt * 16 + col];
#pragma unroll
                for (int nt = 0; nt < CT_ROWS; ++nt) {
                    const float bv = s_in[window_at + nt * CT_WIN + off[s]];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = ct_mfma(av[mt], bv, acc[mt][nt]);
                }
            }
        }
    };
    for (int c0 = 0; c0 < CIN; c0 += CHUNK_C) {          // (uniform over the workgroup: every thread reaches the barriers)
        load_chunk(c0);           // (into registers: in flight while the other waves finish the chunk before)
        __syncthreads();          // the chunk before has been read
        ct_store_window(s_in, iv, pos_lds);
        ct_store_weights<COUTP, RUN, WROW>(s_w, wv);
        __syncthreads();
        const int left = (KTOT - c0 * 9 + 3) / 4;          // k-steps this chunk holds
        if (left >= STEPS) run_steps(STEPS);
        else run_steps(left);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < CT_ROWS; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mt][nt][r] = acc[mt][nt][r] > 0.0f ? acc[mt][nt][r] : 0.0f;

    const int x = tx0 + col;
    const size_t plane = (size_t)h * (size_t)w;
    if constexpr (!FUSE) {
        float* const out = a.out;
        ct_for_each_output(acc, tx0, ty0, wave, col, kq, [=](int ch, int y, int xo, float v) {
            if (ch < COUT && y < h && xo < w) out[(size_t)ch * plane + (size_t)y * w + xo] = v;
        });
    } else {
        // acc is d1 (its padding channels are exact zeros).  fuse_input and final on it, with the weights in the k order the registers give.
        float* const s_fw = s_mem;
        float* const s_lw = s_mem + FUSE_STEPS * 4 * 48;
        __syncthreads();          // the last chunk has been read
        for (int i = threadIdx.x; i < FUSE_STEPS * 4 * 48; i += CT_THREADS) {
            const int m = i % 48, k = (i / 48) & 3, step = i / 192;
            const int c = step < 12 ? (step >> 2) * 16 + k * 4 + (step & 3) : (step - 12) * 4 + k;          // a channel of d1, then of x
            s_fw[i] = (m < HG_C && c < HG_C) ? a.fuse_w[m * (2 * HG_C) + (step < 12 ? c : HG_C + c)] : 0.0f;
        }
        for (int i = threadIdx.x; i < FIN_STEPS * 4 * 16; i += CT_THREADS) {
            const int m = i & 15, k = (i >> 4) & 3, step = i >> 6;
            const int c = (step >> 2) * 16 + k * 4 + (step & 3);
            s_lw[i] = (m < 3 && c < HG_C) ? a.final_w[m * HG_C + c] : 0.0f;
        }
        __syncthreads();
        ct_f32x4 f[3][CT_ROWS];
        ct_start<HG_C>(f, a.fuse_b, kq);
#pragma unroll
        for (int step = 0; step < FUSE_STEPS; ++step) {
            float av[3];
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) av[mt] = s_fw[(step * 4 + kq) * 48 + mt * 16 + col];
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) {
                float bv;
                if (step < 12) bv = acc[step >> 2][nt][step & 3];
                else bv = (step - 12) * 4 + kq < HG_C ? hg_read_plain(a.x, (step - 12) * 4 + kq, ty0 + wave * CT_ROWS + nt, x, h, w) : 0.0f;
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) f[mt][nt] = ct_mfma(av[mt], bv, f[mt][nt]);
            }
        }
        ct_f32x4 res[1][CT_ROWS];
        ct_start<3>(res, a.final_b, kq);
#pragma unroll
        for (int step = 0; step < FIN_STEPS; ++step) {
            const float av = s_lw[(step * 4 + kq) * 16 + col];
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) {
                const float fv = f[step >> 2][nt][step & 3];
                res[0][nt] = ct_mfma(av, fv > 0.0f ? fv : 0.0f, res[0][nt]);
            }
        }
        if (kq == 0) {          // rows 0 .. 2 of the result tile: the three colour channels
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) {
                const int y = ty0 + wave * CT_ROWS + nt;
                if (y < h && x < w) {
                    const size_t p = (size_t)y * w + x;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        a.residual[(size_t)ch * plane + p] = res[0][nt][ch];
                        if (a.image_pred) a.image_pred[(size_t)ch * plane + p] = hg_blend(a.burned, a.x[(size_t)(HG_C - 3 + ch) * plane + p], res[0][nt][ch]);
                    }
                }
            }
        }
    }
}

template <int CA, int CB, int COUT, int MODE, bool FUSE>
static void hg_launch(hipStream_t st, const HgArgs& a)
{
    const dim3 grid((unsigned)((a.w + CT_TILE - 1) / CT_TILE), (unsigned)((a.h + CT_TILE - 1) / CT_TILE));
    hipLaunchKernelGGL((hg_conv3_kernel<CA, CB, COUT, MODE, FUSE>), grid, dim3(CT_THREADS), 0, st, a);
}

static HgArgs hg_layer(const float* in_a, const float* in_b, const float* weight, const float* bias, float* out, int h, int w, int hs, int ws)
{
    HgArgs a = {};
    a.a = in_a; a.b = in_b; a.weight = weight; a.bias = bias; a.out = out; a.h = h; a.w = w; a.hs = hs; a.ws = ws;
    return a;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_hg_required_scratch(int64_t H, int64_t W)
{
    if (!hg_shape_ok(nullptr, H, W)) return 0;
    Carver c(nullptr);
    hg_carve_stages<float>(c, (size_t)H, (size_t)W, 1);
    return hg_carved_bytes(c, nullptr);
}

int32_t ibgs_hg_forward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                        const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                        const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                        const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                        float burned_in_gauss, float* residual, float* image_pred, void* scratch, size_t scratch_bytes)
{
    if (!hg_shape_ok("hg_forward", H, W)) return -IBGS_ERR_INVALID;
    if (!x) { set_error("hg_forward: null input"); return -IBGS_ERR_INVALID; }
    const float* const params[18] = {enc1_w, enc1_b, enc2_w, enc2_b, enc3_w, enc3_b, up2_conv_w, up2_conv_b, dec2_w, dec2_b, up1_conv_w, up1_conv_b, dec1_w, dec1_b,
                                     fuse_input_w, fuse_input_b, final_w, final_b};
    if (!hg_params_ok("hg_forward", params)) return -IBGS_ERR_INVALID;
    if (!residual) { set_error("hg_forward: null outputs: residual is required"); return -IBGS_ERR_INVALID; }
    Carver c(static_cast<char*>(scratch));
    const HgStages<float> sc = hg_carve_stages<float>(c, (size_t)H, (size_t)W, 1);          // the arena of the header: float32 planes
    if (!arena_ok("hg_forward", "scratch", scratch, scratch_bytes, hg_carved_bytes(c, scratch))) return -IBGS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2;
    hg_launch<38, 0, 38, CT_PLAIN, false>(st, hg_layer(x, nullptr, enc1_w, enc1_b, sc.e1, H, W, H, W));
    hg_launch<38, 0, 19, CT_POOL, false>(st, hg_layer(sc.e1, nullptr, enc2_w, enc2_b, sc.e2, H2, W2, H, W));
    hg_launch<19, 0, 9, CT_POOL, false>(st, hg_layer(sc.e2, nullptr, enc3_w, enc3_b, sc.b, H4, W4, H2, W2));
    hg_launch<9, 0, 19, CT_UP, false>(st, hg_layer(sc.b, nullptr, up2_conv_w, up2_conv_b, sc.u2, H2, W2, H4, W4));
    hg_launch<19, 19, 19, CT_PLAIN, false>(st, hg_layer(sc.u2, sc.e2, dec2_w, dec2_b, sc.d2, H2, W2, H2, W2));
    hg_launch<19, 0, 38, CT_UP, false>(st, hg_layer(sc.d2, nullptr, up1_conv_w, up1_conv_b, sc.u1, H, W, H2, W2));
    HgArgs last = hg_layer(sc.u1, sc.e1, dec1_w, dec1_b, nullptr, H, W, H, W);
    last.x = x; last.fuse_w = fuse_input_w; last.fuse_b = fuse_input_b; last.final_w = final_w; last.final_b = final_b;
    last.burned = burned_in_gauss; last.residual = residual; last.image_pred = image_pred;
    hg_launch<38, 38, 38, CT_PLAIN, true>(st, last);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
