// The two geometry loss terms of the reference's steady-state iteration (train.py:308-338) on the device (C ABI: include/ibgs_geo_loss.h; Python:
// ibgs_amd/losses.py `photometric_loss` / `normal_consistency`): the multi-view photometric term -- mask, blend, a structural-similarity map per source,
// masked means, and autograd's mirror of each: nine plane launches and a dozen element-wise kernels over S x 3 x H x W in torch -- as one kernel per
// frame forward and one backward, and the normal-consistency term as one pass over its six planes.  Neither waits for the device: the number of valid
// pixels Nv, on which the reference branches on the host, is formed, tested and divided by on the device.
//
// The window weights, the two filter passes over a tile and the per-pixel forms are shared/ssim_window.h's, the ones ssim.hip runs (DESIGN.md section 13 says
// where that header lives and why); what their bits rest on is stated there.  Like ssim.hip this unit is compiled without -ffp-contract=off.
//
// CONTRACT (photometric)
//   valid      valid[s, p] = (((f0 + f1) + f2) + f3) > 0 on the four feature planes of source s, float32, in that order (cam_feat is signed).
//   masked     valid ? warped : gt, formed on the way into LDS: never in HBM.
//   m          the map of (gt, masked[s]): shared/ssim_window.h's with x = gt, y = masked.
//   sums       per workgroup (one tile of one source) in f64: sum valid (1 - (m0 + m1 + m2) / 3), sum valid (|d0| + |d1| + |d2|) / 3 with d = gt - warped in
//              f32, and sum valid.  geoloss_photo_final_kernel: thread t adds the partials t, t + 1024, .. in that order, block_reduce adds the threads; then
//              Nv == 0 ? 0 : photo_weight ((1 - w_s) l1 / Nv + w_s ss / Nv).  No float atomics.
//   derivative planes (when a gradient will be asked for): dm/dv, dm/dq, dm/dr -- ssimw_pixel with the roles of (u, p) and (v, q) swapped -- times valid.
//   backward   grad_warped = valid ? k_s combine(w*D0, w*D1, w*D2; warped, gt) + k_1 sign(warped - gt) : 0, with k_s = -go w_p w_s / (3 Nv) and
//              k_1 = go w_p (1 - w_s) / (3 Nv) formed in f64 from the device scalars go and Nv (both 0 when Nv == 0), sign(0) = 0.  The filter passes are
//              f32 fma chains as in ssim.hip; from their results on the expression is evaluated in f64 and rounded once (on a frame of a few pixels the
//              float32 yardstick is itself within an ulp of float64: tests/test_gpu_geoloss.py).  Sources from S on: zeros.
//
// CONTRACT (normal consistency)
//   loss = weight (0.4 mean_p sum_c |dn - n| + 0.6 mean_p (1 - sum_c dn n)); the per-pixel terms are formed in f64 from the f32 inputs and summed in f64:
//   one partial pair per workgroup, added by geoloss_normal_final_kernel as above.  Unit gradients from the same pass, each the f32 rounding of the f64
//   k (-/+ 0.4 sign(dn - n) - 0.6 other), k = weight / (H W); geoloss_rescale_kernel multiplies them by the incoming device scalar and leaves at once when it is 1.
//
// KERNELS
//   geoloss_photo_fwd_kernel     one workgroup of 256 threads per 32 x 32 tile and source.  The validity of the 42 x 42 staged texels once; then per channel
//                                ssim.hip's three steps (stage with halo, row pass, column pass) and the per-pixel form.  44 KB of LDS.
//   geoloss_photo_bwd_kernel     the same tiling over the three derivative planes of each channel; 39 KB of LDS.
//   geoloss_photo_final_kernel, geoloss_normal_kernel, geoloss_normal_final_kernel, geoloss_rescale_kernel
// What bounds them: DESIGN.md section 13.
#include "common.h"
#include "block_ops.h"
#include "shared/ssim_window.h"
#include "../../include/ibgs_geo_loss.h"

namespace ibgs {

constexpr int GF = 1024;                             // threads of the final kernels' one workgroup
constexpr int NC_THREADS = 256, NC_MAX_BLOCKS = 1024;

// ssimw_combine, evaluated in f64 from the f32 filtered planes: both products are exact there, so where x == y and cb == -cc / 2 (the two images agree
// over the window) the sum is exactly ca, as in the f32 form; what the f32 form rounds five times is rounded once, by the caller
__device__ __forceinline__ double geo_combine(float ca, float cb, float cc, float x, float y)
{
    const double t1 = (2.0 * (double)x) * (double)cb, t2 = (double)y * (double)cc;
    return (double)ca + (t1 + t2);
}

// the sum's order is the contract: cam_feat is signed
__device__ __forceinline__ bool geo_valid(const float* __restrict__ feat, size_t plane, size_t o)
{
#pragma clang fp contract(off)
    return (((feat[o] + feat[plane + o]) + feat[2 * plane + o]) + feat[3 * plane + o]) > 0.0f;
}

// gt: 3 planes; warped: S x 3 planes; feat: S x 4 planes; dplanes (or null): 3 x S x 3 planes; partials: (S x tiles) x 3
__global__ void __launch_bounds__(SSIMW_THREADS) geoloss_photo_fwd_kernel(const float* __restrict__ gt, const float* __restrict__ warped, const float* __restrict__ feat, int H, int W,
                                                                          int tiles_x, int tiles, size_t total, float* __restrict__ dplanes, double* __restrict__ partials)
{
    __shared__ float sx[SSIMW_SH * SSIMW_SS], sy[SSIMW_SH * SSIMW_SS];
    __shared__ __attribute__((aligned(16))) float hq[5][SSIMW_SH * SSIMW_TW];
    __shared__ unsigned char sv[SSIMW_SH * SSIMW_SW];
    const SsimwTile t(tiles, tiles_x);
    const size_t plane = (size_t)H * (size_t)W;
    const float* const fs = feat + (size_t)t.outer * 4 * plane;

    for (int i = threadIdx.x; i < SSIMW_SH * SSIMW_SW; i += SSIMW_THREADS) {
        const int r = i / SSIMW_SW, c = i - r * SSIMW_SW;
        const int gy = t.ty0 - SSIMW_HALO + r, gx = t.tx0 - SSIMW_HALO + c;
        bool v = false;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = geo_valid(fs, plane, (size_t)gy * (size_t)W + (size_t)gx);
        sv[i] = v ? 1 : 0;
    }
    __syncthreads();

    const int col = threadIdx.x & (SSIMW_TW - 1), r0 = (int)(threadIdx.x / SSIMW_TW) * SSIMW_OPT;
    const int gx = t.tx0 + col;
    double msum[SSIMW_OPT] = {0.0, 0.0, 0.0, 0.0}, dsum[SSIMW_OPT] = {0.0, 0.0, 0.0, 0.0};

    for (int ch = 0; ch < 3; ++ch) {
        const float* const xg = gt + (size_t)ch * plane;
        const float* const yw = warped + ((size_t)t.outer * 3 + ch) * plane;
        for (int i = threadIdx.x; i < SSIMW_SH * SSIMW_SW; i += SSIMW_THREADS) {
            const int r = i / SSIMW_SW, c = i - r * SSIMW_SW;
            const int gy = t.ty0 - SSIMW_HALO + r, gxx = t.tx0 - SSIMW_HALO + c;
            float a = 0.0f, b = 0.0f;
            if (gy >= 0 && gy < H && gxx >= 0 && gxx < W) {
                const size_t o = (size_t)gy * (size_t)W + (size_t)gxx;
                a = xg[o];
                b = a;
                if (sv[i]) b = yw[o];          // the warped colour is read at valid texels only
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

        float f[5][SSIMW_OPT];
#pragma unroll
        for (int k = 0; k < 5; ++k) ssimw_vpass_col(hq[k], r0, col, f[k]);
#pragma unroll
        for (int i = 0; i < SSIMW_OPT; ++i) {
            const int gy = t.ty0 + r0 + i;
            if (gy < H && gx < W) {
                // with respect to the masked side: the roles of (u, p) and (v, q) swapped; m itself does not notice
                const SsimwPixel px = ssimw_pixel(f[1][i], f[0][i], f[3][i], f[2][i], f[4][i], dplanes != nullptr);
                const bool v = sv[(r0 + i + SSIMW_HALO) * SSIMW_SW + col + SSIMW_HALO] != 0;
                if (dplanes) {
                    const size_t o = ((size_t)t.outer * 3 + ch) * plane + (size_t)gy * (size_t)W + (size_t)gx;
                    dplanes[o] = v ? px.du : 0.0f;
                    dplanes[total + o] = v ? px.dp : 0.0f;
                    dplanes[2 * total + o] = v ? px.dr : 0.0f;
                }
                const float d = sx[(r0 + i + SSIMW_HALO) * SSIMW_SS + col + SSIMW_HALO] - sy[(r0 + i + SSIMW_HALO) * SSIMW_SS + col + SSIMW_HALO];
                msum[i] += (double)px.m;
                dsum[i] += (double)fabsf(d);
            }
        }
        __syncthreads();          // the next channel's staging overwrites sx, sy, hq
    }

    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < SSIMW_OPT; ++i) {
        const int gy = t.ty0 + r0 + i;
        if (gy < H && gx < W && sv[(r0 + i + SSIMW_HALO) * SSIMW_SW + col + SSIMW_HALO]) {
            acc[0] += 1.0 - msum[i] / 3.0;
            acc[1] += dsum[i] / 3.0;
            acc[2] += 1.0;
        }
    }
    block_reduce<SSIMW_THREADS, 3>(acc, partials + (size_t)blockIdx.x * 3, op_add());
}

// One workgroup.  Thread t adds the partials t, t + GF, .. in that order; block_reduce adds the threads; thread 0 writes the loss and Nv.
__global__ void __launch_bounds__(GF) geoloss_photo_final_kernel(const double* __restrict__ partials, int count, double photo_weight, double w_s, float* __restrict__ loss,
                                                                 double* __restrict__ nv_out)
{
    __shared__ double s_sum[3];
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < count; i += GF) {
        a[0] += partials[(size_t)i * 3];
        a[1] += partials[(size_t)i * 3 + 1];
        a[2] += partials[(size_t)i * 3 + 2];
    }
    block_reduce<GF, 3>(a, s_sum, op_add());
    __syncthreads();
    if (threadIdx.x == 0) {
        const double nv = s_sum[2];
        *nv_out = nv;
        *loss = nv > 0.0 ? (float)(photo_weight * ((1.0 - w_s) * (s_sum[1] / nv) + w_s * (s_sum[0] / nv))) : 0.0f;
    }
}

// grid: S_total x tiles; the sources from S on are only zeroed
__global__ void __launch_bounds__(SSIMW_THREADS) geoloss_photo_bwd_kernel(const float* __restrict__ gt, const float* __restrict__ warped, const float* __restrict__ feat,
                                                                          const float* __restrict__ dplanes, size_t total, const double* __restrict__ nv_dev,
                                                                          const float* __restrict__ go_dev, double photo_weight, double w_s, int S, int H, int W, int tiles_x, int tiles,
                                                                          float* __restrict__ grad)
{
    __shared__ float sd[3][SSIMW_SH * SSIMW_SS];
    __shared__ __attribute__((aligned(16))) float hq[3][SSIMW_SH * SSIMW_TW];
    const SsimwTile t(tiles, tiles_x);
    const size_t plane = (size_t)H * (size_t)W;
    const int col = threadIdx.x & (SSIMW_TW - 1), r0 = (int)(threadIdx.x / SSIMW_TW) * SSIMW_OPT;
    const int gx = t.tx0 + col;

    if (t.outer >= S) {          // (wave-uniform) never read: their gradient is zero
        for (int ch = 0; ch < 3; ++ch)
            for (int i = 0; i < SSIMW_OPT; ++i) {
                const int gy = t.ty0 + r0 + i;
                if (gy < H && gx < W) grad[((size_t)t.outer * 3 + ch) * plane + (size_t)gy * (size_t)W + (size_t)gx] = 0.0f;
            }
        return;
    }

    const double nv = *nv_dev, go = (double)*go_dev;
    const double k_s = nv > 0.0 ? -go * photo_weight * w_s / (3.0 * nv) : 0.0;
    const double k_1 = nv > 0.0 ? go * photo_weight * (1.0 - w_s) / (3.0 * nv) : 0.0;
    const float* const fs = feat + (size_t)t.outer * 4 * plane;
    bool valid[SSIMW_OPT];
#pragma unroll
    for (int i = 0; i < SSIMW_OPT; ++i) {
        const int gy = t.ty0 + r0 + i;
        valid[i] = gy < H && gx < W && geo_valid(fs, plane, (size_t)gy * (size_t)W + (size_t)gx);
    }

    for (int ch = 0; ch < 3; ++ch) {
        const size_t base = ((size_t)t.outer * 3 + ch) * plane;
        for (int i = threadIdx.x; i < SSIMW_SH * SSIMW_SW; i += SSIMW_THREADS) {
            const int r = i / SSIMW_SW, c = i - r * SSIMW_SW;
            const int gy = t.ty0 - SSIMW_HALO + r, gxx = t.tx0 - SSIMW_HALO + c;
            float a = 0.0f, b = 0.0f, d = 0.0f;
            if (gy >= 0 && gy < H && gxx >= 0 && gxx < W) {
                const size_t o = base + (size_t)gy * (size_t)W + (size_t)gxx;
                a = dplanes[o];
                b = dplanes[total + o];
                d = dplanes[2 * total + o];
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

        float f[3][SSIMW_OPT];
#pragma unroll
        for (int k = 0; k < 3; ++k) ssimw_vpass_col(hq[k], r0, col, f[k]);
#pragma unroll
        for (int i = 0; i < SSIMW_OPT; ++i) {
            const int gy = t.ty0 + r0 + i;
            if (gy < H && gx < W) {
                const size_t o = (size_t)gy * (size_t)W + (size_t)gx;
                float g = 0.0f;
                if (valid[i]) {          // masked == warped here
                    const float wv = warped[base + o], gv = gt[(size_t)ch * plane + o];
                    const double sgn = wv > gv ? 1.0 : (wv < gv ? -1.0 : 0.0);
                    g = (float)(k_s * geo_combine(f[0][i], f[1][i], f[2][i], wv, gv) + k_1 * sgn);          // f64 from the filtered planes on: one rounding
                }
                grad[base + o] = g;
            }
        }
        __syncthreads();          // the next channel's staging overwrites sd, hq
    }
}

// n: 3 planes (rendered normal), dn: 3 planes (depth normal); gn, gdn (each 3 planes, or null): the unit gradients
__global__ void __launch_bounds__(NC_THREADS) geoloss_normal_kernel(const float* __restrict__ n, const float* __restrict__ dn, size_t plane, double k, float* __restrict__ gn,
                                                                    float* __restrict__ gdn, double* __restrict__ partials)
{
    double acc[2] = {0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * NC_THREADS + threadIdx.x; p < plane; p += (size_t)gridDim.x * NC_THREADS) {
        double l1 = 0.0, dot = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t o = (size_t)c * plane + p;
            const double a = (double)n[o], b = (double)dn[o];
            const double d = b - a;
            const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
            l1 += fabs(d);
            dot += b * a;
            if (gn) gn[o] = (float)(k * (-0.4 * sgn - 0.6 * b));
            if (gdn) gdn[o] = (float)(k * (0.4 * sgn - 0.6 * a));
        }
        acc[0] += l1;
        acc[1] += 1.0 - dot;
    }
    block_reduce<NC_THREADS, 2>(acc, partials + (size_t)blockIdx.x * 2, op_add());
}

__global__ void __launch_bounds__(GF) geoloss_normal_final_kernel(const double* __restrict__ partials, int count, double weight, double pixels, float* __restrict__ loss)
{
    double a[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < count; i += GF) {
        a[0] += partials[(size_t)i * 2];
        a[1] += partials[(size_t)i * 2 + 1];
    }
    __shared__ double s_sum[2];
    block_reduce<GF, 2>(a, s_sum, op_add());
    __syncthreads();
    if (threadIdx.x == 0) *loss = (float)(weight * (0.4 * (s_sum[0] / pixels) + 0.6 * (s_sum[1] / pixels)));
}

// a stored unit gradient times autograd's incoming gradient, a DEVICE scalar, in place; 1.0 moves no data
__global__ void __launch_bounds__(NC_THREADS) geoloss_rescale_kernel(float* __restrict__ grad, size_t n, const float* __restrict__ scale)
{
    const float k = *scale;
    if (k == 1.0f) return;          // (wave-uniform: a scalar load and a branch)
    for (size_t i = (size_t)blockIdx.x * NC_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * NC_THREADS) grad[i] *= k;
}

struct GeoShape {
    size_t tiles, plane;
    int tiles_x;
};

// who == nullptr: silent (the size query)
static bool geo_shape_ok(const char* who, int64_t sources, int64_t H, int64_t W, GeoShape* s)
{
    if (sources < 1 || sources > IBGS_GEOLOSS_MAX_SRC || H < 1 || W < 1 || H > IBGS_GEOLOSS_MAX_SIDE || W > IBGS_GEOLOSS_MAX_SIDE) {
        if (who) set_error("%s: %lld sources of %lld x %lld out of range (1 .. %d sources, sides 1 .. %d)", who, (long long)sources, (long long)H, (long long)W,
                           IBGS_GEOLOSS_MAX_SRC, IBGS_GEOLOSS_MAX_SIDE);
        return false;
    }
    const size_t tx = ((size_t)W + SSIMW_TW - 1) / SSIMW_TW, ty = ((size_t)H + SSIMW_TH - 1) / SSIMW_TH;
    s->tiles = tx * ty;          // <= 2048^2: sources x tiles < 2^31
    s->tiles_x = (int)tx;
    s->plane = (size_t)H * (size_t)W;
    return true;
}

struct GeoScratch {
    double* photo;          // sources x tiles x 3
    double* normal;         // NC_MAX_BLOCKS x 2
    static GeoScratch carve(char* base, size_t sources, const GeoShape& s, size_t* total)
    {
        GeoScratch d;
        Carver c(base);
        d.photo = c.take<double>(sources * s.tiles * 3);
        d.normal = c.take<double>((size_t)NC_MAX_BLOCKS * 2);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return d;
    }
};

static bool geo_weight_ok(double w) { return w == w && w > -1e30 && w < 1e30; }

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_geoloss_required_scratch(int64_t sources, int64_t H, int64_t W)
{
    GeoShape s;
    if (!geo_shape_ok(nullptr, sources, H, W, &s)) return 0;
    size_t total = 0;
    GeoScratch::carve(nullptr, (size_t)sources, s, &total);
    return total;
}

void ibgs_geoloss_tile(int32_t* th, int32_t* tw)
{
    if (th) *th = SSIMW_TH;
    if (tw) *tw = SSIMW_TW;
}

int32_t ibgs_geoloss_photo_forward(void* stream, int32_t S, int32_t H, int32_t W, const float* gt, const float* warped, const float* cam_feat, double photo_weight,
                                   double photo_ssim_weight, float* dplanes_out, float* loss_out, double* nv_out, void* scratch, size_t scratch_bytes)
{
    GeoShape s;
    if (!geo_shape_ok("geoloss_photo_forward", S, H, W, &s)) return -IBGS_ERR_INVALID;
    if (!gt || !warped || !cam_feat) { set_error("geoloss_photo_forward: null image"); return -IBGS_ERR_INVALID; }
    if (!loss_out || !nv_out) { set_error("geoloss_photo_forward: null outputs: loss_out and nv_out are required"); return -IBGS_ERR_INVALID; }
    if (!geo_weight_ok(photo_weight) || !geo_weight_ok(photo_ssim_weight)) { set_error("geoloss_photo_forward: the weights must be finite"); return -IBGS_ERR_INVALID; }
    size_t need = 0;
    const GeoScratch sc = GeoScratch::carve(static_cast<char*>(scratch), (size_t)S, s, &need);
    if (!arena_ok("geoloss_photo_forward", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t groups = (size_t)S * s.tiles;
    hipLaunchKernelGGL(geoloss_photo_fwd_kernel, dim3((unsigned)groups), dim3(SSIMW_THREADS), 0, st, gt, warped, cam_feat, H, W, s.tiles_x, (int)s.tiles, (size_t)S * 3 * s.plane,
                       dplanes_out, sc.photo);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(geoloss_photo_final_kernel, dim3(1), dim3(GF), 0, st, sc.photo, (int)groups, photo_weight, photo_ssim_weight, loss_out, nv_out);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_geoloss_photo_backward(void* stream, int32_t S, int32_t S_total, int32_t H, int32_t W, const float* gt, const float* warped, const float* cam_feat,
                                    const float* dplanes, const double* nv, const float* grad_out, double photo_weight, double photo_ssim_weight, float* grad_warped)
{
    GeoShape s;
    if (!geo_shape_ok("geoloss_photo_backward", S, H, W, &s) || !geo_shape_ok("geoloss_photo_backward", S_total, H, W, &s)) return -IBGS_ERR_INVALID;
    if (S > S_total) { set_error("geoloss_photo_backward: %d sources read of %d out of range", S, S_total); return -IBGS_ERR_INVALID; }
    if (!gt || !warped || !cam_feat || !dplanes || !nv || !grad_out || !grad_warped) { set_error("geoloss_photo_backward: null array"); return -IBGS_ERR_INVALID; }
    if (!geo_weight_ok(photo_weight) || !geo_weight_ok(photo_ssim_weight)) { set_error("geoloss_photo_backward: the weights must be finite"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(geoloss_photo_bwd_kernel, dim3((unsigned)((size_t)S_total * s.tiles)), dim3(SSIMW_THREADS), 0, reinterpret_cast<hipStream_t>(stream), gt, warped, cam_feat, dplanes,
                       (size_t)S * 3 * s.plane, nv, grad_out, photo_weight, photo_ssim_weight, S, H, W, s.tiles_x, (int)s.tiles, grad_warped);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_geoloss_normal_forward(void* stream, int32_t H, int32_t W, const float* normal, const float* depth_normal, double weight, float* grad_normal,
                                    float* grad_depth_normal, float* loss_out, void* scratch, size_t scratch_bytes)
{
    GeoShape s;
    if (!geo_shape_ok("geoloss_normal_forward", 1, H, W, &s)) return -IBGS_ERR_INVALID;
    if (!normal || !depth_normal) { set_error("geoloss_normal_forward: null image"); return -IBGS_ERR_INVALID; }
    if (!loss_out) { set_error("geoloss_normal_forward: null outputs: loss_out is required"); return -IBGS_ERR_INVALID; }
    if (!geo_weight_ok(weight)) { set_error("geoloss_normal_forward: the weight must be finite"); return -IBGS_ERR_INVALID; }
    size_t need = 0;
    const GeoScratch sc = GeoScratch::carve(static_cast<char*>(scratch), 1, s, &need);
    if (!arena_ok("geoloss_normal_forward", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    size_t nb = (s.plane + (size_t)NC_THREADS * 4 - 1) / ((size_t)NC_THREADS * 4);
    if (nb > (size_t)NC_MAX_BLOCKS) nb = NC_MAX_BLOCKS;
    hipLaunchKernelGGL(geoloss_normal_kernel, dim3((unsigned)nb), dim3(NC_THREADS), 0, st, normal, depth_normal, s.plane, weight / (double)s.plane, grad_normal,
                       grad_depth_normal, sc.normal);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(geoloss_normal_final_kernel, dim3(1), dim3(GF), 0, st, sc.normal, (int)nb, weight, (double)s.plane, loss_out);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_geoloss_rescale(void* stream, int64_t n, float* grad, const float* scale_dev)
{
    if (n < 1 || n > (int64_t)3 * IBGS_GEOLOSS_MAX_SIDE * IBGS_GEOLOSS_MAX_SIDE) { set_error("geoloss_rescale: %lld elements out of range", (long long)n); return -IBGS_ERR_INVALID; }
    if (!grad || !scale_dev) { set_error("geoloss_rescale: null array"); return -IBGS_ERR_INVALID; }
    size_t nb = ((size_t)n + (size_t)NC_THREADS * 4 - 1) / ((size_t)NC_THREADS * 4);
    if (nb > (size_t)NC_MAX_BLOCKS * 4) nb = (size_t)NC_MAX_BLOCKS * 4;
    hipLaunchKernelGGL(geoloss_rescale_kernel, dim3((unsigned)nb), dim3(NC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), grad, (size_t)n, scale_dev);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
