// LPIPS (VGG16, version 0.1) on the device (C ABI: include/ibgs_lpips.h; Python: ibgs_amd/lpips.py): the reference's lpipsPyTorch modules as metrics.py:82
// calls them -- z-score, the thirteen convolutions of vgg16.features up to relu5_3 with their four pools, and the normalise / difference / lin / mean head on
// five taps -- as thirteen launches of ONE templated 3 x 3 implicit-GEMM kernel over both images of a pair, five head launches and a final sum.  No pooled
// or z-scored tensor is ever materialised.
//
// CONTRACT (the definition is in the header)
//   Every feature is an f32 multiply-add chain on the matrix cores started from the bias, over k = 9 (input channel) + tap in the order of the weights'
//   layout.  The contract is a tolerance against a float64 restatement (tests/lpips_ref.py), not this order.  The same arguments give
//   the same bits on every call and stream: no atomics; the only thing that crosses a workgroup is the head's partial sums, added in a fixed order.
//
// THE PRODUCTS are v_mfma_f32_16x16x4_f32 on the 16 x 16 tile of shared/conv_tile.h, which states the lane map and the staging: output channels are M, 16
// pixels of one row N, K runs over k = 9 (input channel) + tap, four consecutive k per instruction.
//
// KERNEL  lpips_conv3_kernel<POOL, FIRST>: 256 threads = 4 waves per 16 x 16 output tile and block of 64 output channels of one image; grid = (tiles across,
// tiles down, 2 images x Cout / 64).  A wave owns four rows of the tile and the block's 64 channels: 4 x 4 accumulator tiles (64 registers).  The input
// channels are walked in chunks of 4 with a runtime trip count (every Cin of VGG16 but the first is a multiple of 4; the first layer's 3 channels are one
// chunk, K = 27 padded to 28: seven k-steps): per chunk the workgroup stages the 18 x 18 input window (tile and one-pixel halo; read plain, or as the 2 x 2
// maximum of the stage before with POOL; z-scored in frame with FIRST; out-of-frame taps and padding channels are zeros, and no address outside a plane is
// formed: coordinates are clamped into the frame before an offset is made of them) and the chunk's 64 x 36 weights (runs of 36 consecutive floats per
// output channel, stored k-major) into LDS, then runs 9 k-steps of 16 products each.  A thread's loads of a chunk are unconditional and issued together,
// ahead of the barrier that waits for the chunk before.  Offsets of a channel's plane and of an image are 64-bit (a stage passes 2^31 bytes from 2048 x
// 2048 on); offsets inside a plane fit 32 bits (4096 x 4096).
// KERNEL  lpips_head_kernel: a thread per pixel of a tap; lpips_final_kernel: one workgroup.  What bounds each and what was measured: DESIGN.md section 17.
#include "common.h"
#include "block_ops.h"
#include "shared/conv_tile.h"
#include "../../include/ibgs_lpips.h"

namespace ibgs {

constexpr int LP_CHUNK = 4;                          // input channels per staged chunk
constexpr int LP_MT = 4;                             // result tiles of 16 channels per wave
constexpr int LP_COB = 16 * LP_MT;                   // output channels per workgroup
constexpr int LP_RUN = LP_CHUNK * 9;                 // k of a chunk
constexpr int LP_STEPS = LP_RUN / 4;                 // k-steps of a chunk
constexpr int LP_WROW = LP_COB + 1;                  // floats per k of the staged weights: consecutive k fall into different banks
constexpr int LP_NW = LP_COB * LP_RUN / CT_THREADS;  // weights per thread and chunk
constexpr int LP_HEAD_THREADS = 256;
static_assert(LP_COB * LP_RUN % CT_THREADS == 0, "the staging below");

static const int LP_CHANNELS[IBGS_LPIPS_CONVS + 1] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int LP_LEVEL[IBGS_LPIPS_CONVS] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};          // resolution level of a convolution's output
static const int LP_TAP_CONV[IBGS_LPIPS_TAPS] = {1, 3, 6, 9, 12};                               // the convolution whose ReLU is tap k

// networks.py:41-51: (v - mean) / std of channel c, as two float32 operations
__device__ __forceinline__ float lp_zscore(float v, int c)
{
#pragma clang fp contract(off)
    const float mean = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float sd = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    return (v - mean) / sd;
}

struct LpArgs {
    const float* in_x; const float* in_y;          // the two images' inputs: cin planes of hs x ws each
    const float* weight; const float* bias;        // (cout, cin, 3, 3), (cout)
    float* out;                                    // [x: cout planes of h x w | y: the same]
    int cin, cout, h, w, hs, ws;                   // the output's resolution, and the input's
};

template <bool POOL, bool FIRST>
__global__ void __launch_bounds__(CT_THREADS, 2) lpips_conv3_kernel(const LpArgs a)
{
    constexpr int MODE = POOL ? CT_POOL : CT_PLAIN;
    __shared__ float s_mem[LP_CHUNK * CT_PLANE + LP_RUN * LP_WROW];
    ct_lds* const s_in = (ct_lds*)s_mem;
    ct_lds* const s_w = s_in + LP_CHUNK * CT_PLANE;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int tx0 = blockIdx.x * CT_TILE, ty0 = blockIdx.y * CT_TILE;
    const int blocks = a.cout / LP_COB, img = (int)blockIdx.z / blocks, co0 = ((int)blockIdx.z - img * blocks) * LP_COB;          // (uniform)
    const int h = a.h, w = a.w, cin = a.cin, ktot = cin * 9;
    const float* const src = img ? a.in_y : a.in_x;
    const float* const wsrc = a.weight + (size_t)co0 * ktot;

    ct_f32x4 acc[LP_MT][CT_ROWS];
    ct_start<LP_COB>(acc, a.bias + co0, kq);
    // This lane's k of step s of a chunk is 4 s + kq: its channel of the chunk and tap, as an offset into the staged window.  (The table and the k-steps that
    // read it stay in the kernel: as helpers of conv_tile.h they cost hg_conv3_kernel 0.4 - 0.8 % of its time.)
    int off[LP_STEPS];
#pragma unroll
    for (int s = 0; s < LP_STEPS; ++s) {
        const int kk = 4 * s + kq, cl = kk / 9, t = kk - 9 * cl, dy = t / 3;
        off[s] = cl * CT_PLANE + dy * CT_WIN + (t - 3 * dy);
    }
    const int window_at = wave * CT_ROWS * CT_WIN + col;

    // the input holds planes of hs x ws: (h, w) itself, or with POOL >= (2 h, 2 w)
    const size_t plane_in = (size_t)a.hs * (size_t)a.ws;
    int pos_off[CT_NPOS], pos_lds[CT_NPOS];
    bool pos_in[CT_NPOS];
    ct_window_positions<MODE>(pos_off, pos_lds, pos_in, tx0, ty0, h, w, a.hs, a.ws);
    float iv[LP_CHUNK][CT_NPOS], wv[LP_NW];
    auto load_chunk = [&](const int c0) {
#pragma unroll
        for (int cl = 0; cl < LP_CHUNK; ++cl) {
            if (FIRST && cl >= 3) {          // the first layer: three channels, the fourth of the chunk is padding
#pragma unroll
                for (int r = 0; r < CT_NPOS; ++r) iv[cl][r] = 0.0f;
                continue;
            }
            const int c = c0 + cl, cc = c < cin ? c : cin - 1;          // (uniform)
            const float* const base = src + (size_t)cc * plane_in;
#pragma unroll
            for (int r = 0; r < CT_NPOS; ++r) {
                float v = ct_read<MODE>(base + pos_off[r], a.ws);
                if (FIRST) v = lp_zscore(v, cc);          // in frame only: the padding is zero in z-space
                iv[cl][r] = (c < cin && pos_in[r]) ? v : 0.0f;
            }
        }
#pragma unroll
        for (int n = 0; n < LP_NW; ++n) {          // runs of LP_RUN consecutive floats of one output channel's row
            const int i = (int)threadIdx.x + n * CT_THREADS, m = i / LP_RUN, j = i - m * LP_RUN, kk = c0 * 9 + j;
            const float v = wsrc[(size_t)m * ktot + min(kk, ktot - 1)];
            wv[n] = kk < ktot ? v : 0.0f;
        }
    };
    auto run_steps = [&](const int limit) {
#pragma unroll
        for (int s = 0; s < LP_STEPS; ++s) {
            if (s < limit) {
                float av[LP_MT];
#pragma unroll
                for (int mt = 0; mt < LP_MT; ++mt) av[mt] = s_w[(4 * s + kq) * LP_WROW + mt * 16 + col];
#pragma unroll
                for (int nt = 0; nt < CT_ROWS; ++nt) {
                    const float bv = s_in[window_at + nt * CT_WIN + off[s]];
#pragma unroll
                    for (int mt = 0; mt < LP_MT; ++mt) acc[mt][nt] = ct_mfma(av[mt], bv, acc[mt][nt]);
                }
            }
        }
    };
#pragma unroll 1
    for (int c0 = 0; c0 < cin; c0 += LP_CHUNK) {          // (uniform over the workgroup: every thread reaches the barriers; one copy of the body: not peeled)
        load_chunk(c0);           // (into registers: in flight while the other waves finish the chunk before)
        __syncthreads();          // the chunk before has been read
        ct_store_window(s_in, iv, pos_lds);
        ct_store_weights<LP_COB, LP_RUN, LP_WROW>(s_w, wv);
        __syncthreads();
        if (FIRST) run_steps((27 + 3) / 4);          // K = 27 -> 28
        else run_steps(LP_STEPS);                    // (cin is a multiple of LP_CHUNK: the host checks)
    }

    const size_t plane = (size_t)h * (size_t)w;
    float* const dst = a.out + ((size_t)img * a.cout + co0) * plane;
    ct_for_each_output(acc, tx0, ty0, wave, col, kq, [=](int ch, int y, int x, float v) {
        if (y < h && x < w) dst[(size_t)ch * plane + (size_t)y * w + x] = v > 0.0f ? v : 0.0f;
    });
}

// utils.py:6-8 and lpips.py:30-36 on one tap: a thread per pixel.  Two passes over the channels (the norms, then the weighted squared differences), in
// double from the float32 features; m is rounded once to float32, and that float32 value is what the workgroup's partial sums.
struct LpHeadArgs { const float* fx; const float* fy; const float* lin; float* map; double* partial; int c, npix; };

__global__ void __launch_bounds__(LP_HEAD_THREADS) lpips_head_kernel(const LpHeadArgs a)
{
    // no contraction: n_x - n_y is the difference of two ROUNDED products (fma(f_x, i_x, -(f_y i_y)) would leave the rounding error of one of them for
    // identical images, and lpips(x, x) would not be 0, nor lpips(x, y) the bits of lpips(y, x)); the sums below are fma by name
#pragma clang fp contract(off)
    const int p = (int)blockIdx.x * LP_HEAD_THREADS + (int)threadIdx.x;
    const bool valid = p < a.npix;
    const size_t n = (size_t)a.npix;
    const float* const fx = a.fx + (valid ? p : a.npix - 1);          // (a pixel past the end reads the last one's features and contributes nothing)
    const float* const fy = a.fy + (valid ? p : a.npix - 1);
    double sx = 0.0, sy = 0.0;
#pragma unroll 4
    for (int c = 0; c < a.c; ++c) {
        const double vx = fx[(size_t)c * n], vy = fy[(size_t)c * n];
        sx = fma(vx, vx, sx);
        sy = fma(vy, vy, sy);
    }
    const double ix = 1.0 / (sqrt(sx) + 1e-10), iy = 1.0 / (sqrt(sy) + 1e-10);          // all-zero features: 0 x 1e10 = 0, not NaN
    double m = 0.0;
#pragma unroll 4
    for (int c = 0; c < a.c; ++c) {
        const double d = (double)fx[(size_t)c * n] * ix - (double)fy[(size_t)c * n] * iy;
        m = fma((double)a.lin[c], d * d, m);
    }
    const float mf = valid ? (float)m : 0.0f;
    if (a.map && valid) a.map[p] = mf;
    double sum[1] = {(double)mf};
    block_reduce<LP_HEAD_THREADS, 1>(sum, a.partial + blockIdx.x, op_add());
}

// v_k = (the partials of tap k, thread t adding t, t + 256, .. in that order, then block_reduce's tree) / pixels of tap k; lpips = v_1 + .. + v_5
struct LpFinalArgs { const double* partial; int count[IBGS_LPIPS_TAPS]; int npix[IBGS_LPIPS_TAPS]; float* lpips; float* tap_values; };

__global__ void __launch_bounds__(LP_HEAD_THREADS) lpips_final_kernel(const LpFinalArgs a)
{
    __shared__ double s_v[IBGS_LPIPS_TAPS];
    double sum[IBGS_LPIPS_TAPS];
    int at = 0;
#pragma unroll
    for (int k = 0; k < IBGS_LPIPS_TAPS; ++k) {
        double s = 0.0;
        for (int i = threadIdx.x; i < a.count[k]; i += LP_HEAD_THREADS) s += a.partial[at + i];
        sum[k] = s;
        at += a.count[k];
    }
    const double v = block_reduce<LP_HEAD_THREADS, IBGS_LPIPS_TAPS>(sum, op_add());
    if (threadIdx.x < IBGS_LPIPS_TAPS) s_v[threadIdx.x] = v / (double)a.npix[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < IBGS_LPIPS_TAPS; ++k) {
            total += s_v[k];
            if (a.tap_values) a.tap_values[k] = (float)s_v[k];
        }
        a.lpips[0] = (float)total;
    }
}

// who == nullptr: silent (the size query)
static bool lp_shape_ok(const char* who, int64_t H, int64_t W)
{
    if (H < IBGS_LPIPS_MIN_SIDE || W < IBGS_LPIPS_MIN_SIDE || H > IBGS_LPIPS_MAX_SIDE || W > IBGS_LPIPS_MAX_SIDE) {
        if (who) set_error("%s: a frame of %lld x %lld is out of range (sides %d .. %d)", who, (long long)H, (long long)W, IBGS_LPIPS_MIN_SIDE, IBGS_LPIPS_MAX_SIDE);
        return false;
    }
    return true;
}

struct LpScratch {          // the arena of the header
    float* stage[IBGS_LPIPS_CONVS];          // the output of every convolution: [x | y]
    double* partial;
    int h[IBGS_LPIPS_TAPS], w[IBGS_LPIPS_TAPS], count[IBGS_LPIPS_TAPS];
    static LpScratch carve(char* base, size_t H, size_t W, size_t* total)
    {
        LpScratch s;
        size_t n[IBGS_LPIPS_TAPS];          // n(C_k, k): floats of a stage of level k at the level's own channel count, both images
        static const size_t ch[IBGS_LPIPS_TAPS] = {64, 128, 256, 512, 512};
        size_t partials = 0;
        for (int k = 0; k < IBGS_LPIPS_TAPS; ++k) {
            s.h[k] = (int)(k ? s.h[k - 1] / 2 : H);
            s.w[k] = (int)(k ? s.w[k - 1] / 2 : W);
            n[k] = 2 * ch[k] * (size_t)s.h[k] * (size_t)s.w[k];
            s.count[k] = (int)(((size_t)s.h[k] * (size_t)s.w[k] + LP_HEAD_THREADS - 1) / LP_HEAD_THREADS);
            partials += (size_t)s.count[k];
        }
        Carver c(base);
        float* const q = c.take<float>(n[0]);
        float* const p = c.take<float>(n[0]);
        s.partial = c.take<double>(partials);
        float* const r3 = p + n[2];          // the space of relu3_2
        float* const r4 = r3 + n[3];         // the space of relu4_2
        s.stage[0] = p;  s.stage[1] = q;                                // relu1_1, relu1_2
        s.stage[2] = p;  s.stage[3] = p + n[1];                         // relu2_1, relu2_2
        s.stage[4] = p;  s.stage[5] = r3; s.stage[6] = p;               // relu3_1, relu3_2, relu3_3
        s.stage[7] = r3; s.stage[8] = r4; s.stage[9] = r3;              // relu4_1, relu4_2, relu4_3
        s.stage[10] = r4; s.stage[11] = r4 + n[4]; s.stage[12] = r4 + 2 * n[4];          // relu5_1, relu5_2, relu5_3
        if (total) *total = ((c.cur + 127) & ~uintptr_t(127)) - reinterpret_cast<uintptr_t>(base);
        return s;
    }
};

static void lp_launch(hipStream_t st, const LpArgs& a, bool pool, bool first)
{
    const dim3 grid((unsigned)((a.w + CT_TILE - 1) / CT_TILE), (unsigned)((a.h + CT_TILE - 1) / CT_TILE), (unsigned)(2 * (a.cout / LP_COB)));
    if (first) hipLaunchKernelGGL((lpips_conv3_kernel<false, true>), grid, dim3(CT_THREADS), 0, st, a);
    else if (pool) hipLaunchKernelGGL((lpips_conv3_kernel<true, false>), grid, dim3(CT_THREADS), 0, st, a);
    else hipLaunchKernelGGL((lpips_conv3_kernel<false, false>), grid, dim3(CT_THREADS), 0, st, a);
}

static LpArgs lp_layer(const float* in_x, const float* in_y, const float* weight, const float* bias, float* out, int cin, int cout, int h, int w, int hs, int ws)
{
    LpArgs a;
    a.in_x = in_x; a.in_y = in_y; a.weight = weight; a.bias = bias; a.out = out; a.cin = cin; a.cout = cout; a.h = h; a.w = w; a.hs = hs; a.ws = ws;
    return a;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_lpips_required_scratch(int64_t H, int64_t W)
{
    size_t total = 0;
    if (!lp_shape_ok(nullptr, H, W)) return 0;
    LpScratch::carve(nullptr, (size_t)H, (size_t)W, &total);
    return total;
}

int32_t ibgs_lpips_conv3(void* stream, int32_t hs, int32_t ws, int32_t cin, int32_t cout, int32_t pool, int32_t zscore, const float* in_x,
                         const float* in_y, const float* weight, const float* bias, float* out)
{
    const int h = pool ? hs / 2 : hs, w = pool ? ws / 2 : ws;
    if (hs < 1 || ws < 1 || h < 1 || w < 1 || hs > (pool ? 2 : 1) * IBGS_LPIPS_MAX_SIDE + 1 || ws > (pool ? 2 : 1) * IBGS_LPIPS_MAX_SIDE + 1 || h > IBGS_LPIPS_MAX_SIDE || w > IBGS_LPIPS_MAX_SIDE) {
        set_error("lpips_conv3: an input of %d x %d is out of range (output sides 1 .. %d)", hs, ws, IBGS_LPIPS_MAX_SIDE);
        return -IBGS_ERR_INVALID;
    }
    if (cout < LP_COB || cout % LP_COB || cout > 512) { set_error("lpips_conv3: cout = %d is not a multiple of %d in %d .. 512", cout, LP_COB, LP_COB); return -IBGS_ERR_INVALID; }
    if (zscore ? (cin != 3 || pool) : (cin < LP_CHUNK || cin % LP_CHUNK || cin > 512)) {
        set_error("lpips_conv3: cin = %d (3, unpooled, with the z-score; else a multiple of %d up to 512)", cin, LP_CHUNK);
        return -IBGS_ERR_INVALID;
    }
    if (!in_x || !in_y) { set_error("lpips_conv3: null input"); return -IBGS_ERR_INVALID; }
    if (!weight || !bias) { set_error("lpips_conv3: null parameters"); return -IBGS_ERR_INVALID; }
    if (!out) { set_error("lpips_conv3: null output"); return -IBGS_ERR_INVALID; }
    lp_launch(reinterpret_cast<hipStream_t>(stream), lp_layer(in_x, in_y, weight, bias, out, cin, cout, h, w, hs, ws), pool != 0, zscore != 0);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_lpips_forward(void* stream, int32_t H, int32_t W, const float* x, const float* y, const float* const* conv_w, const float* const* conv_b,
                           const float* const* lin_w, float* lpips, float* tap_values, float* const* maps, void* scratch, size_t scratch_bytes)
{
    size_t need = 0;
    if (!lp_shape_ok("lpips_forward", H, W)) return -IBGS_ERR_INVALID;
    if (!x || !y) { set_error("lpips_forward: null input: %s", x ? "y" : "x"); return -IBGS_ERR_INVALID; }
    if (!conv_w || !conv_b || !lin_w) { set_error("lpips_forward: null parameters: the %s table", !conv_w ? "conv_w" : (!conv_b ? "conv_b" : "lin_w")); return -IBGS_ERR_INVALID; }
    for (int i = 0; i < IBGS_LPIPS_CONVS; ++i)
        if (!conv_w[i] || !conv_b[i]) { set_error("lpips_forward: null parameters: convolution %d's %s", i, conv_w[i] ? "bias" : "weight"); return -IBGS_ERR_INVALID; }
    for (int k = 0; k < IBGS_LPIPS_TAPS; ++k)
        if (!lin_w[k]) { set_error("lpips_forward: null parameters: lin %d's weight", k); return -IBGS_ERR_INVALID; }
    if (!lpips) { set_error("lpips_forward: null outputs: lpips is required"); return -IBGS_ERR_INVALID; }
    const LpScratch sc = LpScratch::carve(static_cast<char*>(scratch), (size_t)H, (size_t)W, &need);
    if (!arena_ok("lpips_forward", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    LpFinalArgs fin;
    fin.partial = sc.partial; fin.lpips = lpips; fin.tap_values = tap_values;
    const float *in_x = x, *in_y = y;
    int tap = 0, at = 0;
    for (int i = 0; i < IBGS_LPIPS_CONVS; ++i) {
        const int k = LP_LEVEL[i], cin = LP_CHANNELS[i], cout = LP_CHANNELS[i + 1];
        const bool pool = i > 0 && LP_LEVEL[i - 1] != k;
        const int hs = pool ? sc.h[k - 1] : sc.h[k], ws = pool ? sc.w[k - 1] : sc.w[k];
        lp_launch(st, lp_layer(in_x, in_y, conv_w[i], conv_b[i], sc.stage[i], cin, cout, sc.h[k], sc.w[k], hs, ws), pool, i == 0);
        const size_t image = (size_t)cout * (size_t)sc.h[k] * (size_t)sc.w[k];
        in_x = sc.stage[i];
        in_y = sc.stage[i] + image;
        if (i == LP_TAP_CONV[tap]) {
            LpHeadArgs ha;
            ha.fx = in_x; ha.fy = in_y; ha.lin = lin_w[tap]; ha.map = maps ? maps[tap] : nullptr; ha.partial = sc.partial + at; ha.c = cout; ha.npix = sc.h[k] * sc.w[k];
            hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)sc.count[tap]), dim3(LP_HEAD_THREADS), 0, st, ha);
            fin.count[tap] = sc.count[tap]; fin.npix[tap] = ha.npix;
            at += sc.count[tap];
            ++tap;
        }
    }
    hipLaunchKernelGGL(lpips_final_kernel, dim3(1), dim3(LP_HEAD_THREADS), 0, st, fin);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
