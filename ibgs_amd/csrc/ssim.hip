// Fused SSIM on the device (C ABI: include/ibgs_ssim.h; Python: ibgs_amd/losses.py `ssim` / `ssim_map`, ibgs_amd/image_eval.py): the reference's `ssim` and
// `compute_photometric_ssim` (utils/loss_utils.py:34-91) -- five grouped 11 x 11 convolutions and about twenty element-wise kernels, and the same again in
// autograd's backward -- as one pass over the two images forward and one pass backward.  The contract is a tolerance against a float64 restatement
// ("Fused SSIM"; tests/ssim_ref.py), so this unit is compiled without -ffp-contract=off: the two filter passes are fma chains.  The window, the
// passes over a tile and the per-pixel forms are shared/ssim_window.h's (geoloss.hip runs the same ones); what their bits rest on is stated there.
//
// CONTRACT
//   map        m(x, y) of shared/ssim_window.h: zero padding of 5 on every side of every plane; m(x, y) == m(y, x) bit for bit, m == 1 exactly where x == y
//              over the window.
//   derivative planes (only when a gradient will be asked for): dm/du, dm/dp, dm/dr in the forms stated there; where x == y the gradient below is exactly zero.
//   backward   dL/dx(t) = (w*[G dm/du])(t) + 2 x(t) (w*[G dm/dp])(t) + y(t) (w*[G dm/dr])(t), the three products and two sums rounded one by one
//              (ssimw_combine).  G is the upstream gradient, per plane or per pixel, read on the device.  w is symmetric: the correlation of the forward is
//              the convolution here.
//   sums       sum m, sum (x - y)^2, sum |x - y| in f64 (x - y itself in f32, as the reference forms it): one partial per workgroup (block_reduce, block_ops.h),
//              then ssim_final_kernel: lane l of a wave adds a plane's partials l, l + 64, .. in that order, the xor tree of wave_reduce adds the lanes; an
//              image's sums are its planes' in channel order, the overall sums all planes' in index order.  No float atomics; an image's sums depend on
//              that image alone.
//
// KERNELS
//   ssim_fwd_kernel    one workgroup of 256 threads per 32 x 32 tile of one plane.  (1) the tile of x and y with its halo into LDS, one bounds-checked scalar
//                      load per texel: nothing assumes an alignment, nothing outside the plane is read; (2) the row pass over the five quantities; (3) the
//                      column pass, then m and what the call asked for.  42 KB of LDS: three workgroups per CU.
//   ssim_bwd_kernel    the same tiling over the three derivative planes, each multiplied by G on the way into LDS; 39 KB of LDS.
//   ssim_final_kernel  one workgroup; see "sums".
// What bounds them: DESIGN.md, "Fused SSIM".
#include "common.h"
#include "block_ops.h"
#include "shared/ssim_window.h"
#include "../../include/ibgs_ssim.h"

namespace ibgs {

constexpr int FT = 1024;                             // threads of the final kernel's one workgroup
static_assert(SSIMW_TAPS == IBGS_SSIM_WINDOW, "the shared window is the header's");

__global__ void __launch_bounds__(SSIMW_THREADS) ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int tiles_x, int tiles, size_t total,
                                                                 float* __restrict__ map_out, float* __restrict__ dmaps, double* __restrict__ partials)
{
    __shared__ float sx[SSIMW_SH * SSIMW_SS], sy[SSIMW_SH * SSIMW_SS];
    __shared__ __attribute__((aligned(16))) float hq[5][SSIMW_SH * SSIMW_TW];
    const SsimwTile t(tiles, tiles_x);
    const size_t base = (size_t)t.outer * (size_t)H * (size_t)W;

    for (int i = threadIdx.x; i < SSIMW_SH * SSIMW_SW; i += SSIMW_THREADS) {
        const int r = i / SSIMW_SW, c = i - r * SSIMW_SW;
        const int gy = t.ty0 - SSIMW_HALO + r, gx = t.tx0 - SSIMW_HALO + c;
        float a = 0.0f, b = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            a = x[o];
            b = y[o];
        }
        sx[r * SSIMW_SS + c] = a;
        sy[r * SSIMW_SS + c] = b;
    }
    __syncthreads();

    for (int task = threadIdx.x; task < SSIMW_SH * SSIMW_HGROUPS; task += SSIMW_THREADS) {
        const int r = task / SSIMW_HGROUPS, c0 = (task - r * SSIMW_HGROUPS) * SSIMW_OPT;
        ssimw_hpass_row5(sx, sy, hq, r, c0);
    }
    __syncthreads();

    const int col = threadIdx.x & (SSIMW_TW - 1), r0 = (int)(threadIdx.x / SSIMW_TW) * SSIMW_OPT;
    float f[5][SSIMW_OPT];
#pragma unroll
    for (int k = 0; k < 5; ++k) ssimw_vpass_col(hq[k], r0, col, f[k]);

    double acc[3] = {0.0, 0.0, 0.0};
    const int gx = t.tx0 + col;
#pragma unroll
    for (int i = 0; i < SSIMW_OPT; ++i) {
        const int gy = t.ty0 + r0 + i;
        if (gy < H && gx < W) {
            const SsimwPixel px = ssimw_pixel(f[0][i], f[1][i], f[2][i], f[3][i], f[4][i], dmaps != nullptr);
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            if (map_out) map_out[o] = px.m;
            if (dmaps) {
                dmaps[o] = px.du;
                dmaps[total + o] = px.dp;
                dmaps[2 * total + o] = px.dr;
            }
            const float d = sx[(r0 + i + SSIMW_HALO) * SSIMW_SS + col + SSIMW_HALO] - sy[(r0 + i + SSIMW_HALO) * SSIMW_SS + col + SSIMW_HALO];
            acc[0] += (double)px.m;
            acc[1] += (double)d * (double)d;
            acc[2] += (double)fabsf(d);
        }
    }
    if (partials) block_reduce<SSIMW_THREADS, 3>(acc, partials + (size_t)blockIdx.x * 3, op_add());          // (wave-uniform: a kernel argument)
}

__global__ void __launch_bounds__(SSIMW_THREADS) ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dmaps, size_t total,
                                                                 const float* __restrict__ plane_scale, const float* __restrict__ grad_map, int H, int W, int tiles_x, int tiles,
                                                                 float* __restrict__ grad_x)
{
    __shared__ float sd[3][SSIMW_SH * SSIMW_SS];
    __shared__ __attribute__((aligned(16))) float hq[3][SSIMW_SH * SSIMW_TW];
    const SsimwTile t(tiles, tiles_x);
    const size_t base = (size_t)t.outer * (size_t)H * (size_t)W;
    const float scale = plane_scale ? plane_scale[t.outer] : 0.0f;          // (wave-uniform)

    for (int i = threadIdx.x; i < SSIMW_SH * SSIMW_SW; i += SSIMW_THREADS) {
        const int r = i / SSIMW_SW, c = i - r * SSIMW_SW;
        const int gy = t.ty0 - SSIMW_HALO + r, gx = t.tx0 - SSIMW_HALO + c;
        float a = 0.0f, b = 0.0f, d = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            const float g = plane_scale ? scale : grad_map[o];
            a = g * dmaps[o];
            b = g * dmaps[total + o];
            d = g * dmaps[2 * total + o];
        }
        sd[0][r * SSIMW_SS + c] = a;
        sd[1][r * SSIMW_SS + c] = b;
        sd[2][r * SSIMW_SS + c] = d;
    }
    __syncthreads();

    for (int task = threadIdx.x; task < SSIMW_SH * SSIMW_HGROUPS; task += SSIMW_THREADS) {
        const int r = task / SSIMW_HGROUPS, c0 = (task - r * SSIMW_HGROUPS) * SSIMW_OPT;
#pragma unroll
        for (int k = 0; k < 3; ++k) ssimw_hpass_row(sd[k], hq[k], r, c0);
    }
    __syncthreads();

    const int col = threadIdx.x & (SSIMW_TW - 1), r0 = (int)(threadIdx.x / SSIMW_TW) * SSIMW_OPT;
    float f[3][SSIMW_OPT];
#pragma unroll
    for (int k = 0; k < 3; ++k) ssimw_vpass_col(hq[k], r0, col, f[k]);
    const int gx = t.tx0 + col;
#pragma unroll
    for (int i = 0; i < SSIMW_OPT; ++i) {
        const int gy = t.ty0 + r0 + i;
        if (gy < H && gx < W) {
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            grad_x[o] = ssimw_combine(f[0][i], f[1][i], f[2][i], x[o], y[o]);
        }
    }
}

// One workgroup of 16 waves.  Phase 1: wave w takes the planes w, w + 16, ..: lane l adds the plane's partials l, l + 64, .. in that order (the loads of eight
// steps in flight at once), wave_reduce adds the lanes, lane 0 stores the plane's three sums.  Phase 2: thread n adds the sums of image n's planes in channel
// order and writes the image's means; thread 0 adds all planes' sums in index order and writes the overall means.
__global__ void __launch_bounds__(FT) ssim_final_kernel(const double* __restrict__ partials, int tiles, int N, int C, double pixels_per_plane, double* plane_sums,
                                                        float* __restrict__ out_mean, float* __restrict__ out_per_image, float* __restrict__ out_mse_per_image,
                                                        float* __restrict__ out_l1, float* __restrict__ out_l1_per_image)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int planes = N * C;
    for (int pl = wave; pl < planes; pl += FT / 64) {
        const double* p = partials + (size_t)pl * (size_t)tiles * 3;
        double a[3] = {0.0, 0.0, 0.0};
#pragma unroll 8
        for (int i = lane; i < tiles; i += 64) {
            a[0] += p[(size_t)i * 3];
            a[1] += p[(size_t)i * 3 + 1];
            a[2] += p[(size_t)i * 3 + 2];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = wave_reduce(a[k], op_add());
        if (lane == 0) {
            plane_sums[(size_t)pl * 3] = a[0];
            plane_sums[(size_t)pl * 3 + 1] = a[1];
            plane_sums[(size_t)pl * 3 + 2] = a[2];
        }
    }
    __threadfence();
    __syncthreads();
    const volatile double* s = plane_sums;
    const double per_image = pixels_per_plane * (double)C;
    for (int n = threadIdx.x; n < N; n += FT) {
        double img[3] = {0.0, 0.0, 0.0};
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < 3; ++k) img[k] += s[((size_t)n * (size_t)C + c) * 3 + k];
        if (out_per_image) out_per_image[n] = (float)(img[0] / per_image);
        if (out_mse_per_image) out_mse_per_image[n] = (float)(img[1] / per_image);
        if (out_l1_per_image) out_l1_per_image[n] = (float)(img[2] / per_image);
    }
    if (threadIdx.x == 0 && (out_mean || out_l1)) {
        double m = 0.0, l1 = 0.0;
        for (int pl = 0; pl < planes; ++pl) { m += s[(size_t)pl * 3]; l1 += s[(size_t)pl * 3 + 2]; }
        if (out_mean) *out_mean = (float)(m / (per_image * (double)N));
        if (out_l1) *out_l1 = (float)(l1 / (per_image * (double)N));
    }
}

struct SsimShape {
    size_t planes, tiles, total;
    int tiles_x;
};

// who == nullptr: silent (the size query)
static bool ssim_shape_ok(const char* who, int64_t planes, int64_t H, int64_t W, SsimShape* s)
{
    if (planes < 1 || H < 1 || W < 1 || H > IBGS_SSIM_MAX_SIDE || W > IBGS_SSIM_MAX_SIDE || planes >= (int64_t(1) << 31)) {
        if (who) set_error("%s: %lld planes of %lld x %lld out of range (>= 1, sides <= %d)", who, (long long)planes, (long long)H, (long long)W, IBGS_SSIM_MAX_SIDE);
        return false;
    }
    const size_t tx = ((size_t)W + SSIMW_TW - 1) / SSIMW_TW, ty = ((size_t)H + SSIMW_TH - 1) / SSIMW_TH;
    if ((size_t)planes * tx * ty >= (size_t(1) << 31)) {
        if (who) set_error("%s: %lld planes of %lld x %lld out of range (planes x tiles < 2^31)", who, (long long)planes, (long long)H, (long long)W);
        return false;
    }
    s->planes = (size_t)planes;
    s->tiles = tx * ty;
    s->tiles_x = (int)tx;
    s->total = (size_t)planes * (size_t)H * (size_t)W;
    return true;
}

struct SsimScratch {
    double* partials;          // planes x tiles x 3
    double* plane_sums;        // planes x 3
    static SsimScratch carve(char* base, const SsimShape& s, size_t* total)
    {
        SsimScratch d;
        Carver c(base);
        d.partials = c.take<double>(s.planes * s.tiles * 3);
        d.plane_sums = c.take<double>(s.planes * 3);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return d;
    }
};

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_ssim_required_scratch(int64_t planes, int64_t H, int64_t W)
{
    SsimShape s;
    if (!ssim_shape_ok(nullptr, planes, H, W, &s)) return 0;
    size_t total = 0;
    SsimScratch::carve(nullptr, s, &total);
    return total;
}

void ibgs_ssim_tile(int32_t* th, int32_t* tw)
{
    if (th) *th = SSIMW_TH;
    if (tw) *tw = SSIMW_TW;
}

int32_t ibgs_ssim_forward(void* stream, int32_t N, int32_t C, int32_t H, int32_t W, const float* x, const float* y, float* map_out, float* dmaps_out,
                          float* out_mean, float* out_per_image, float* out_mse_per_image, float* out_l1, float* out_l1_per_image, void* scratch,
                          size_t scratch_bytes)
{
    SsimShape s;
    if (N < 1 || C < 1) { set_error("ssim_forward: N %d, C %d out of range (>= 1)", N, C); return -IBGS_ERR_INVALID; }
    if (!ssim_shape_ok("ssim_forward", (int64_t)N * (int64_t)C, H, W, &s)) return -IBGS_ERR_INVALID;
    if (!x || !y) { set_error("ssim_forward: null image"); return -IBGS_ERR_INVALID; }
    const bool sums = out_mean || out_per_image || out_mse_per_image || out_l1 || out_l1_per_image;
    if (!sums && !map_out && !dmaps_out) { set_error("ssim_forward: null outputs: nothing to compute"); return -IBGS_ERR_INVALID; }
    SsimScratch sc = {nullptr, nullptr};
    if (sums) {
        size_t need = 0;
        sc = SsimScratch::carve(static_cast<char*>(scratch), s, &need);
        if (!arena_ok("ssim_forward", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3((unsigned)(s.planes * s.tiles)), dim3(SSIMW_THREADS), 0, st, x, y, H, W, s.tiles_x, (int)s.tiles, s.total, map_out, dmaps_out, sc.partials);
    IBGS_HIP(hipGetLastError());
    if (sums) {
        hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(FT), 0, st, sc.partials, (int)s.tiles, N, C, (double)H * (double)W, sc.plane_sums, out_mean, out_per_image,
                           out_mse_per_image, out_l1, out_l1_per_image);
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

int32_t ibgs_ssim_backward(void* stream, int32_t N, int32_t C, int32_t H, int32_t W, const float* x, const float* y, const float* dmaps, const float* plane_scale,
                           const float* grad_map, float* grad_x)
{
    SsimShape s;
    if (N < 1 || C < 1) { set_error("ssim_backward: N %d, C %d out of range (>= 1)", N, C); return -IBGS_ERR_INVALID; }
    if (!ssim_shape_ok("ssim_backward", (int64_t)N * (int64_t)C, H, W, &s)) return -IBGS_ERR_INVALID;
    if (!x || !y || !dmaps || !grad_x) { set_error("ssim_backward: null array"); return -IBGS_ERR_INVALID; }
    if ((plane_scale != nullptr) == (grad_map != nullptr)) { set_error("ssim_backward: exactly one of plane_scale and grad_map must be given"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)(s.planes * s.tiles)), dim3(SSIMW_THREADS), 0, reinterpret_cast<hipStream_t>(stream), x, y, dmaps, s.total, plane_scale, grad_map,
                       H, W, s.tiles_x, (int)s.tiles, grad_x);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
