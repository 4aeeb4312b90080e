// The reduced-resolution colour tail on the device (C ABI: include/ibgs_resample.h; Python: ibgs_amd/resample.py): the two resampling steps of the reference's
// fuse_color under residual_resolution_scale != 1 (color_aggregation_network.py:200-239) for test-time rendering.  The reference builds the masked 7-channel
// features of every source at full resolution, runs three F.interpolate over 21 + 3 + 3 planes, hands the result to the network, and interpolates the
// residual back.  Here the first three become one kernel that gathers the four full-resolution taps of a reduced pixel, masks each tap, blends, and runs the
// per-view MLP on the matrix cores without the full-resolution features ever existing; the last becomes one kernel that also forms image_pred.
//
// CONTRACT (the header states it in full)
//   taps       align_corners = True; y0 = (i (in - 1)) / (out - 1) and the remainder in integers, t = (float)rem / (float)(out - 1); columns alike.
//   value      top = fma(tx, b, (1 - tx) a); bottom = fma(tx, d, (1 - tx) c); value = fma(ty, bottom, (1 - ty) top).
//   features   x(q, k) = value of x_full(., k) over the taps, x_full the slot of ibgs_color_agg.h at the full-resolution tap with its own mask; then the two
//              Linear + ReLU layers, the mean or maximum over k < levels, the normalised ray and the colour.
//   upsample   residual_out = value of residual_r; image_pred_out = render_scale * render + residual_out (product and sum rounded one after the other).
//
// THE SLOT AND THE 32 x 32 PRODUCTS are shared/pv_mlp.h's, the chain coloragg.hip runs: the lane and register map and what the bits rest on are stated there.
// Of what it hands back this unit uses the slot's row (blended over the four taps before the layers) and h2.  THE TAP AND VALUE RULE (rsz_tap, rsz_blend) and
// the check of the sides are shared/rsz_taps.h's, which rsztrain.hip, this unit's backward, runs too.
//
// KERNELS
//   rsz_features_kernel  256 threads = 4 waves of 32 reduced pixels, one block of pixels per wave (the grid is not capped); per slot 4 x 7 gathered loads,
//                        21 blends and 20 MFMA.
//   rsz_upsample_kernel  a thread per 4 consecutive output columns of a row: 12 gathered loads per pixel from the small residual, 16-byte loads of render and
//                        16-byte stores of both outputs where the row allows (W % 4 == 0, aligned pointers), 4-byte ones otherwise.
// What bounds them: DESIGN.md section 19.
#include "common.h"
#include "shared/pv_mlp.h"
#include "shared/rsz_taps.h"
#include "../../include/ibgs_resample.h"

namespace ibgs {

constexpr int RT = 256;                              // threads per workgroup
constexpr int RWAVES = RT / 64;
constexpr int RB = 32;                               // reduced pixels per wave
constexpr int RCHUNK = RWAVES * RB;                  // reduced pixels per workgroup
constexpr int RQ = 4;                                // output columns per thread of the upsampling
static_assert(PV_F == IBGS_RSZ_FEATURES && RB == PV_F, "the lane maps below");

__device__ __forceinline__ float rsz_norm3(float a, float b, float c)
{
#pragma clang fp contract(off)
    return sqrtf((a * a + b * b) + c * c);
}

// a wave per block of 32 reduced pixels (wave-uniform bounds: the matrix instructions run with every lane on; a lane past the frame recomputes the last pixel)
template <int MODE>
__global__ void __launch_bounds__(RT) rsz_features_kernel(const float* __restrict__ render, const float* __restrict__ warped, const float* __restrict__ feat,
                                                          const float* __restrict__ ray, const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const float* __restrict__ b2, const int32_t* __restrict__ levels, int S, uint32_t H,
                                                          uint32_t W, uint32_t Hr, uint32_t Wr, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const PvFrag f(w1, w2, c, h);
    __shared__ PvBias bias;
    pv_stage_bias(bias, b1, b2);
    const int lv = *levels;          // (wave-uniform)
    const int L = lv < 0 ? 0 : (lv > S ? S : lv);
    const size_t plane = (size_t)H * W, plane_r = (size_t)Hr * Wr;
    const size_t first = ((size_t)blockIdx.x * RWAVES + wave) * RB;
    if (first >= plane_r) return;          // (the whole wave; after the only barrier)
    const bool in = first + c < plane_r;
    const size_t q = in ? first + c : plane_r - 1;
    const uint32_t i = (uint32_t)(q / Wr), j = (uint32_t)(q - (size_t)i * Wr);
    const RszTap ty = rsz_tap(i, H, Hr), tx = rsz_tap(j, W, Wr);
    const size_t p[4] = {(size_t)ty.i0 * W + tx.i0, (size_t)ty.i0 * W + tx.i1, (size_t)ty.i1 * W + tx.i0, (size_t)ty.i1 * W + tx.i1};
    float r[4][3];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        r[n][0] = render[p[n]]; r[n][1] = render[plane + p[n]]; r[n][2] = render[2 * plane + p[n]];
    }
    pv_f32x16 agg;
#pragma unroll
    for (int m = 0; m < 16; ++m) agg[m] = 0.0f;
    for (int k = 0; k < L; ++k) {
        float xf[4][PV_INP], x[PV_INP];
#pragma unroll
        for (int n = 0; n < 4; ++n) pv_slot(warped, feat, r[n], plane, p[n], k, xf[n]);          // (each tap under its own mask)
#pragma unroll
        for (int e = 0; e < PV_IN; ++e) x[e] = rsz_blend(xf[0][e], xf[1][e], xf[2][e], xf[3][e], ty, tx);
        x[7] = 0.0f;          // the eighth input of the first layer's four k-steps
        pv_f32x16 h1, h2;          // (h1 is not used here)
        pv_mlp(f, bias, x, h, h1, h2);
#pragma unroll
        for (int m = 0; m < 16; ++m) agg[m] = MODE == IBGS_RSZ_MEAN ? agg[m] + h2[m] : fmaxf(agg[m], h2[m]);          // (h2 >= 0: the maximum may start from 0)
    }
    if (MODE == IBGS_RSZ_MEAN && L > 1) {
        const float n = (float)L;
#pragma unroll
        for (int m = 0; m < 16; ++m) agg[m] = agg[m] / n;
    }
    if (!in) return;
#pragma unroll
    for (int m = 0; m < 16; ++m) out[(size_t)pv_ch(m, h) * plane_r + q] = agg[m];
    float v[3];
    if (h == 0) {          // half 0 writes the ray, half 1 the colour
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* const src = ray + (size_t)ch * plane;
            v[ch] = rsz_blend(src[p[0]], src[p[1]], src[p[2]], src[p[3]], ty, tx);
        }
        const float len = rsz_norm3(v[0], v[1], v[2]) + 1e-10f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = v[ch] / len;
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = rsz_blend(r[0][ch], r[1][ch], r[2][ch], r[3][ch], ty, tx);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[(size_t)(PV_F + 3 * h + ch) * plane_r + q] = v[ch];
}

// VEC: W % 4 == 0 and render, residual_out, image_pred_out are 16-byte aligned.  Item = (row, quad of 4 columns); the same arithmetic per element either way.
template <bool VEC>
__global__ void __launch_bounds__(RT) rsz_upsample_kernel(const float* __restrict__ res, const float* __restrict__ render, float scale, uint32_t H, uint32_t W, uint32_t Hr,
                                                          uint32_t Wr, uint32_t quads_per_row, uint32_t items, float* __restrict__ out, float* __restrict__ pred)
{
#pragma clang fp contract(off)
    const uint32_t item = blockIdx.x * (uint32_t)RT + threadIdx.x;
    if (item >= items) return;
    const uint32_t i = item / quads_per_row, j0 = (item - i * quads_per_row) * RQ;
    const size_t plane = (size_t)H * W, plane_r = (size_t)Hr * Wr;
    const RszTap ty = rsz_tap(i, Hr, H);
    const float* const row0 = res + (size_t)ty.i0 * Wr;
    const float* const row1 = res + (size_t)ty.i1 * Wr;
    float up[3][RQ];
#pragma unroll
    for (int e = 0; e < RQ; ++e) {
        const RszTap tx = rsz_tap(min(j0 + e, W - 1u), Wr, W);          // (a column past the row's end repeats the last one and is not stored)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* const a = row0 + (size_t)ch * plane_r;
            const float* const b = row1 + (size_t)ch * plane_r;
            up[ch][e] = rsz_blend(a[tx.i0], a[tx.i1], b[tx.i0], b[tx.i1], ty, tx);
        }
    }
    const size_t at = (size_t)i * W + j0;
    if (VEC) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float4 g = *reinterpret_cast<const float4*>(render + (size_t)ch * plane + at);
            *reinterpret_cast<float4*>(out + (size_t)ch * plane + at) = make_float4(up[ch][0], up[ch][1], up[ch][2], up[ch][3]);
            *reinterpret_cast<float4*>(pred + (size_t)ch * plane + at) = make_float4(scale * g.x + up[ch][0], scale * g.y + up[ch][1], scale * g.z + up[ch][2], scale * g.w + up[ch][3]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < RQ; ++e) {
            if (j0 + e >= W) break;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const size_t o = (size_t)ch * plane + at + e;
                out[o] = up[ch][e];
                pred[o] = scale * render[o] + up[ch][e];
            }
        }
    }
}

static bool rsz_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ibgs

using namespace ibgs;

extern "C" {

int32_t ibgs_rsz_features_forward(void* stream, int32_t S, int32_t H, int32_t W, int32_t Hr, int32_t Wr, int32_t mode, const float* render, const float* warped,
                                  const float* cam_feat, const float* camera_ray, const float* w1, const float* b1, const float* w2, const float* b2,
                                  const int32_t* levels, float* out)
{
    const char* const who = "rsz_features_forward";
    if (S < 1 || S > IBGS_RSZ_MAX_SRC) { set_error("%s: %d sources out of range (1 .. %d)", who, S, IBGS_RSZ_MAX_SRC); return -IBGS_ERR_INVALID; }
    if (!rsz_sides_ok(who, H, W, Hr, Wr)) return -IBGS_ERR_INVALID;
    if (mode != IBGS_RSZ_MEAN && mode != IBGS_RSZ_MAX) { set_error("%s: mode %d is neither IBGS_RSZ_MEAN nor IBGS_RSZ_MAX", who, mode); return -IBGS_ERR_INVALID; }
    if (!render || !warped || !cam_feat || !camera_ray) { set_error("%s: null image", who); return -IBGS_ERR_INVALID; }
    if (!w1 || !b1 || !w2 || !b2) { set_error("%s: null parameters", who); return -IBGS_ERR_INVALID; }
    if (!levels) { set_error("%s: null levels: the device word of cagg_levels is required", who); return -IBGS_ERR_INVALID; }
    if (!out) { set_error("%s: null outputs: out is required", who); return -IBGS_ERR_INVALID; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t plane_r = (size_t)Hr * (size_t)Wr;
    const unsigned groups = (unsigned)((plane_r + RCHUNK - 1) / RCHUNK);          // (at most 2^25)
    if (mode == IBGS_RSZ_MEAN)
        hipLaunchKernelGGL((rsz_features_kernel<IBGS_RSZ_MEAN>), dim3(groups), dim3(RT), 0, st, render, warped, cam_feat, camera_ray, w1, b1, w2, b2, levels, (int)S, (uint32_t)H,
                           (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr, out);
    else
        hipLaunchKernelGGL((rsz_features_kernel<IBGS_RSZ_MAX>), dim3(groups), dim3(RT), 0, st, render, warped, cam_feat, camera_ray, w1, b1, w2, b2, levels, (int)S, (uint32_t)H,
                           (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr, out);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_rsz_residual_upsample(void* stream, int32_t H, int32_t W, int32_t Hr, int32_t Wr, const float* residual_r, const float* render, float render_scale,
                                   float* residual_out, float* image_pred_out)
{
    const char* const who = "rsz_residual_upsample";
    if (!rsz_sides_ok(who, H, W, Hr, Wr)) return -IBGS_ERR_INVALID;
    if (!residual_r || !render) { set_error("%s: null image", who); return -IBGS_ERR_INVALID; }
    if (!residual_out || !image_pred_out) { set_error("%s: null outputs: residual_out and image_pred_out are required", who); return -IBGS_ERR_INVALID; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t quads_per_row = ((uint32_t)W + RQ - 1) / RQ, items = (uint32_t)H * quads_per_row;          // (at most 2^30)
    const unsigned groups = (items + RT - 1) / RT;
    if (W % RQ == 0 && rsz_aligned16(render) && rsz_aligned16(residual_out) && rsz_aligned16(image_pred_out))
        hipLaunchKernelGGL((rsz_upsample_kernel<true>), dim3(groups), dim3(RT), 0, st, residual_r, render, render_scale, (uint32_t)H, (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr,
                           quads_per_row, items, residual_out, image_pred_out);
    else
        hipLaunchKernelGGL((rsz_upsample_kernel<false>), dim3(groups), dim3(RT), 0, st, residual_r, render, render_scale, (uint32_t)H, (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr,
                           quads_per_row, items, residual_out, image_pred_out);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
