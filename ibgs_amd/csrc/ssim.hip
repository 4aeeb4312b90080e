// Fused SSIM on the device (C ABI: include/ibgs_ssim.h; Python: ibgs_amd/losses.py `ssim` / `ssim_map`, ibgs_amd/image_eval.py): the reference's `ssim` and
// `compute_photometric_ssim` (utils/loss_utils.py:34-91) -- five grouped 11 x 11 convolutions and about twenty element-wise kernels, and the same again in
// autograd's backward -- as one pass over the two images forward and one pass backward.  The contract is a tolerance against a float64 restatement
// ("Fused SSIM"; tests/ssim_ref.py), so this unit is compiled without -ffp-contract=off: the two filter passes are fma chains.  The per-pixel
// expressions are NOT contracted (ssim_pixel, ssim_combine): their symmetry in (x, y) and their exact cancellation at x == y depend on one rounding per
// operation.
//
// CONTRACT
//   window     11 taps, sigma 1.5: the reference's float32 1-D weights (exp in double, stored as float32, divided by their float32 sum: SSIM_W below holds the
//              six distinct results), applied separably -- along the row, then down the column -- with zero padding of 5 on every side of every plane.
//   forward    u, v = w*x, w*y;  p, q, r = w*x^2, w*y^2, w*xy;  s1 = p - u^2, s2 = q - v^2, s12 = r - uv
//              A = 2uv + C1, B = 2 s12 + C2, C = (u^2 + v^2) + C1, D = (s1 + s2) + C2, m = (A B) / (C D), a correctly rounded division.
//              Swapping x and y swaps u with v and p with q and changes no rounding: m(x, y) == m(y, x) bit for bit.  Where x == y over the window,
//              A == C and B == D bit for bit and m == 1 exactly.
//   derivative planes (only when a gradient will be asked for), with t = 2 / (C D):
//              dm/dr = t A;  dm/dp = -m / D, formed as -(dm/dr / 2) (B / D);  dm/du = 2v(B - A)/(CD) - 2u m/C + 2u m/D, formed as t (v (B - A) + (u m) (C - D)).
//              In these forms x == y gives dm/du == 0 and dm/dp == -dm/dr / 2 exactly, and the gradient below is exactly zero there.
//   backward   dL/dx(t) = (w*[G dm/du])(t) + 2 x(t) (w*[G dm/dp])(t) + y(t) (w*[G dm/dr])(t), the three products and two sums rounded one by one.  G is the
//              upstream gradient, per plane or per pixel, read on the device.  w is symmetric: the correlation of the forward is the convolution here.
//   sums       sum m, sum (x - y)^2, sum |x - y| in f64 (x - y itself in f32, as the reference forms it): one partial per workgroup (block_reduce, block_ops.h),
//              then ssim_final_kernel: lane l of a wave adds a plane's partials l, l + 64, .. in that order, the xor tree of wave_reduce adds the lanes; an
//              image's sums are its planes' in channel order, the overall sums all planes' in index order.  No float atomics; an image's sums depend on
//              that image alone.
//
// KERNELS
//   ssim_fwd_kernel    one workgroup of 256 threads per 32 x 32 tile of one plane.  (1) the tile of x and y with its halo (42 x 42, out-of-plane texels 0, a
//                      row stride of 45 floats) into LDS, one bounds-checked scalar load per texel: nothing assumes an alignment, nothing outside the plane is
//                      read; (2) the horizontal pass: a thread takes 4 adjacent outputs of one staged row -- 14 LDS reads of x and of y feed 5 x 4 x 11 fma -- and
//                      stores each quantity's four results with one 16-byte LDS write (the stride of 45 puts the 32 lanes of a half wave on 32 banks);
//                      (3) the vertical pass: a thread takes 4 outputs of one column, 14 LDS reads per quantity (the lanes of a half wave read 32 adjacent
//                      floats), then m and what the call asked for.  42 KB of LDS: three workgroups per CU.
//   ssim_bwd_kernel    the same tiling over the three derivative planes, each multiplied by G on the way into LDS; 39 KB of LDS.
//   ssim_final_kernel  one workgroup; see "sums".
// What bounds them: DESIGN.md, "Fused SSIM".
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_ssim.h"

namespace ibgs {

constexpr int ST = 256;                              // threads per workgroup of the two image kernels
constexpr int FT = 1024;                             // threads of the final kernel's one workgroup
constexpr int SSIM_TH = 32, SSIM_TW = 32;            // the tile of one workgroup
constexpr int TAPS = IBGS_SSIM_WINDOW, HALO = TAPS / 2;
constexpr int SH = SSIM_TH + 2 * HALO, SW = SSIM_TW + 2 * HALO;          // the staged tile
constexpr int SS = 45;                               // its row stride in LDS: 1 mod 4, so that four rows x eight 4-float groups land on 32 different banks
constexpr int OPT = 4;                               // outputs per thread along the filter direction
constexpr int NV = OPT + TAPS - 1;                   // values those outputs read
constexpr int HGROUPS = SSIM_TW / OPT;
static_assert(SSIM_TW == 32 && (ST / SSIM_TW) * OPT == SSIM_TH, "the vertical pass: a thread per column and group of OPT rows");
static_assert(SS >= SW && SS % 4 == 1, "row stride");

// gaussian(11, 1.5) of the reference (loss_utils.py:24-26) in float32: taps 0 .. 5, the window is symmetric (tests/test_ssim_host.py compares them)
constexpr float SSIM_W[6] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f};
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

__device__ __forceinline__ constexpr float ssim_w(int k) { return SSIM_W[k <= HALO ? k : TAPS - 1 - k]; }

// o[i] = sum_k w[k] v[i + k], k ascending, one fma per tap
__device__ __forceinline__ void conv_opt(const float (&v)[NV], float (&o)[OPT])
{
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
        float a = ssim_w(0) * v[i];
#pragma unroll
        for (int k = 1; k < TAPS; ++k) a = fmaf(ssim_w(k), v[i + k], a);
        o[i] = a;
    }
}

struct SsimTile {
    int plane, ty0, tx0;
    __device__ __forceinline__ SsimTile(int tiles, int tiles_x)
    {
        plane = (int)(blockIdx.x / (unsigned)tiles);
        const int tile = (int)(blockIdx.x - (unsigned)plane * (unsigned)tiles);
        const int ty = tile / tiles_x;
        ty0 = ty * SSIM_TH;
        tx0 = (tile - ty * tiles_x) * SSIM_TW;
    }
};

// the horizontal pass over NQ staged planes that need nothing but the filter (the backward's three)
__device__ __forceinline__ void hpass_row(const float* __restrict__ staged, float* __restrict__ out, int r, int c0)
{
    float v[NV], o[OPT];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = staged[r * SS + c0 + j];
    conv_opt(v, o);
    *reinterpret_cast<float4*>(out + r * SSIM_TW + c0) = make_float4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ void vpass_col(const float* __restrict__ hq, int r0, int col, float (&o)[OPT])
{
    float v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = hq[(r0 + j) * SSIM_TW + col];
    conv_opt(v, o);
}

struct SsimPixel { float m, du, dp, dr; };

// One rounding per operation: see CONTRACT for what depends on it.
__device__ __forceinline__ SsimPixel ssim_pixel(float u, float v, float p, float q, float r, bool derivatives)
{
#pragma clang fp contract(off)
    SsimPixel o;
    const float uv = u * v, uu = u * u, vv = v * v;
    const float s1 = p - uu, s2 = q - vv, s12 = r - uv;
    const float A = 2.0f * uv + SSIM_C1, B = 2.0f * s12 + SSIM_C2, C = (uu + vv) + SSIM_C1, D = (s1 + s2) + SSIM_C2;
    const float CD = C * D;
    o.m = (A * B) / CD;
    o.du = o.dp = o.dr = 0.0f;
    if (derivatives) {
        const float t = 2.0f / CD;
        o.dr = t * A;
        o.dp = (-0.5f * o.dr) * (B / D);
        o.du = t * (v * (B - A) + (u * o.m) * (C - D));
    }
    return o;
}

__device__ __forceinline__ float ssim_combine(float ca, float cb, float cc, float x, float y)
{
#pragma clang fp contract(off)
    const float t1 = (2.0f * x) * cb, t2 = y * cc;
    return ca + (t1 + t2);
}

__global__ void __launch_bounds__(ST) ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int tiles_x, int tiles, size_t total,
                                                      float* __restrict__ map_out, float* __restrict__ dmaps, double* __restrict__ partials)
{
    __shared__ float sx[SH * SS], sy[SH * SS];
    __shared__ __attribute__((aligned(16))) float hq[5][SH * SSIM_TW];
    const SsimTile t(tiles, tiles_x);
    const size_t base = (size_t)t.plane * (size_t)H * (size_t)W;

    for (int i = threadIdx.x; i < SH * SW; i += ST) {
        const int r = i / SW, c = i - r * SW;
        const int gy = t.ty0 - HALO + r, gx = t.tx0 - HALO + c;
        float a = 0.0f, b = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            a = x[o];
            b = y[o];
        }
        sx[r * SS + c] = a;
        sy[r * SS + c] = b;
    }
    __syncthreads();

    for (int task = threadIdx.x; task < SH * HGROUPS; task += ST) {
        const int r = task / HGROUPS, c0 = (task - r * HGROUPS) * OPT;
        float xv[NV], yv[NV], tv[NV], o[OPT];
#pragma unroll
        for (int j = 0; j < NV; ++j) { xv[j] = sx[r * SS + c0 + j]; yv[j] = sy[r * SS + c0 + j]; }
        float* const dst = &hq[0][r * SSIM_TW + c0];
        conv_opt(xv, o);
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        conv_opt(yv, o);
        *reinterpret_cast<float4*>(dst + SH * SSIM_TW) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
        for (int j = 0; j < NV; ++j) tv[j] = xv[j] * xv[j];
        conv_opt(tv, o);
        *reinterpret_cast<float4*>(dst + 2 * SH * SSIM_TW) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
        for (int j = 0; j < NV; ++j) tv[j] = yv[j] * yv[j];
        conv_opt(tv, o);
        *reinterpret_cast<float4*>(dst + 3 * SH * SSIM_TW) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
        for (int j = 0; j < NV; ++j) tv[j] = xv[j] * yv[j];
        conv_opt(tv, o);
        *reinterpret_cast<float4*>(dst + 4 * SH * SSIM_TW) = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();

    const int col = threadIdx.x & (SSIM_TW - 1), r0 = (int)(threadIdx.x / SSIM_TW) * OPT;
    float f[5][OPT];
#pragma unroll
    for (int k = 0; k < 5; ++k) vpass_col(hq[k], r0, col, f[k]);

    double acc[3] = {0.0, 0.0, 0.0};
    const int gx = t.tx0 + col;
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
        const int gy = t.ty0 + r0 + i;
        if (gy < H && gx < W) {
            const SsimPixel px = ssim_pixel(f[0][i], f[1][i], f[2][i], f[3][i], f[4][i], dmaps != nullptr);
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            if (map_out) map_out[o] = px.m;
            if (dmaps) {
                dmaps[o] = px.du;
                dmaps[total + o] = px.dp;
                dmaps[2 * total + o] = px.dr;
            }
            const float d = sx[(r0 + i + HALO) * SS + col + HALO] - sy[(r0 + i + HALO) * SS + col + HALO];
            acc[0] += (double)px.m;
            acc[1] += (double)d * (double)d;
            acc[2] += (double)fabsf(d);
        }
    }
    if (partials) block_reduce<ST, 3>(acc, partials + (size_t)blockIdx.x * 3, op_add());          // (wave-uniform: a kernel argument)
}

__global__ void __launch_bounds__(ST) ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dmaps, size_t total,
                                                      const float* __restrict__ plane_scale, const float* __restrict__ grad_map, int H, int W, int tiles_x, int tiles,
                                                      float* __restrict__ grad_x)
{
    __shared__ float sd[3][SH * SS];
    __shared__ __attribute__((aligned(16))) float hq[3][SH * SSIM_TW];
    const SsimTile t(tiles, tiles_x);
    const size_t base = (size_t)t.plane * (size_t)H * (size_t)W;
    const float scale = plane_scale ? plane_scale[t.plane] : 0.0f;          // (wave-uniform)

    for (int i = threadIdx.x; i < SH * SW; i += ST) {
        const int r = i / SW, c = i - r * SW;
        const int gy = t.ty0 - HALO + r, gx = t.tx0 - HALO + c;
        float a = 0.0f, b = 0.0f, d = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            const float g = plane_scale ? scale : grad_map[o];
            a = g * dmaps[o];
            b = g * dmaps[total + o];
            d = g * dmaps[2 * total + o];
        }
        sd[0][r * SS + c] = a;
        sd[1][r * SS + c] = b;
        sd[2][r * SS + c] = d;
    }
    __syncthreads();

    for (int task = threadIdx.x; task < SH * HGROUPS; task += ST) {
        const int r = task / HGROUPS, c0 = (task - r * HGROUPS) * OPT;
#pragma unroll
        for (int k = 0; k < 3; ++k) hpass_row(sd[k], hq[k], r, c0);
    }
    __syncthreads();

    const int col = threadIdx.x & (SSIM_TW - 1), r0 = (int)(threadIdx.x / SSIM_TW) * OPT;
    float f[3][OPT];
#pragma unroll
    for (int k = 0; k < 3; ++k) vpass_col(hq[k], r0, col, f[k]);
    const int gx = t.tx0 + col;
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
        const int gy = t.ty0 + r0 + i;
        if (gy < H && gx < W) {
            const size_t o = base + (size_t)gy * (size_t)W + (size_t)gx;
            grad_x[o] = ssim_combine(f[0][i], f[1][i], f[2][i], x[o], y[o]);
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
    const size_t tx = ((size_t)W + SSIM_TW - 1) / SSIM_TW, ty = ((size_t)H + SSIM_TH - 1) / SSIM_TH;
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
    if (th) *th = SSIM_TH;
    if (tw) *tw = SSIM_TW;
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
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3((unsigned)(s.planes * s.tiles)), dim3(ST), 0, st, x, y, H, W, s.tiles_x, (int)s.tiles, s.total, map_out, dmaps_out, sc.partials);
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
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)(s.planes * s.tiles)), dim3(ST), 0, reinterpret_cast<hipStream_t>(stream), x, y, dmaps, s.total, plane_scale, grad_map,
                       H, W, s.tiles_x, (int)s.tiles, grad_x);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
