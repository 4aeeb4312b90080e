// The backward of the reduced-resolution colour tail (C ABI: include/ibgs_resample_train.h; Python: ibgs_amd/resample_train.py): the adjoints of resample.hip's
// two kernels, so that the colour network trains at Hr x Wr = int(H s) x int(W s) as the reference trains it under residual_resolution_scale != 1
// (color_aggregation_network.py:200-239, train.py:227-228).  The forwards stay resample.hip's.
//
// CONTRACT (the header states it in full)
//   reduced    per reduced pixel q and slot k < levels: the four masked taps, the blend and both layers recomputed with the forward's instructions (pv_slot and
//              pv_mlp of shared/pv_mlp.h; the tap and value rule of shared/rsz_taps.h, which resample.hip runs), then the per-slot backward that cagg_bwd_kernel
//              runs (shared/pv_mlp_bwd.h): dz2 = g (h2 > 0), dz1 = (w2^T dz2) (h1 > 0), gx = (w1^T dz1)[0 .. 2], UNMASKED, to scratch planes at Hr x Wr.
//   parameter gradients   shared/pv_mlp_bwd.h's, over the BLENDED slot: per-wave sums in a fixed order, one f64 partial per workgroup, and coloragg.hip's final
//              pass (pv_launch_final: cagg_final_kernel), one rounding.  No float atomics.
//   gather     a thread per FULL-resolution pixel: Hr <= H makes y0 strictly increasing, so a row is tap y0 of at most one reduced row and tap y1 of at most
//              one, found in integers; at most 2 x 2 reduced pixels per pixel, weights {u_y u_x, u_y t_x, t_y u_x, t_y t_x}; then the pixel's own mask.
//   upsample   a thread per REDUCED element adds, in ascending (i, j), the full-resolution pixels that have it among their taps: f64, one rounding.
//
// WHO STATES WHAT: shared/rsz_taps.h the tap and value rule and the check of the sides; shared/pv_mlp.h the slot and both layers; shared/pv_mlp_bwd.h the
// workgroup's geometry, the per-slot backward, the parameter sums and the layout of the partials.  This file: how a slot's row is made of four taps, where gx
// goes, the gather and the upsampling's adjoint.
//
// KERNELS
//   rzt_features_bwd_kernel  256 threads = 4 waves of 32 reduced pixels over a capped grid that walks the reduced frame in chunks of 128; per slot 4 x 7 gathered
//                            loads, 21 blends and 52 MFMA with parameter gradients.
//   rzt_gather_kernel        a thread per full-resolution pixel: at most 4 x (3 levels + 3) loads from the reduced planes, 4 levels feature loads, 3 S + 3 stores.
//   rzt_upsample_bwd_kernel  a thread per reduced element of the three planes.
// The final pass of the parameter gradients is cagg_final_kernel (coloragg.hip).  What bounds them: DESIGN.md section 19.
#include "common.h"
#include "shared/pv_mlp_bwd.h"
#include "shared/rsz_taps.h"
#include "../../include/ibgs_resample.h"
#include "../../include/ibgs_resample_train.h"

namespace ibgs {

constexpr int ZT = 256;                              // threads per workgroup of the gather and of the upsampling's adjoint (rzt_features_bwd_kernel's geometry is shared/pv_mlp_bwd.h's)
static_assert(PV_F == IBGS_RSZ_FEATURES && IBGS_RSZ_MEAN == PV_MEAN && IBGS_RSZ_MAX == PV_MAX, "the shared backward's width and modes");

// The smallest output index whose y0 is >= y, for out <= in (y0 strictly increasing): ceil(y (out - 1) / (in - 1)); `out` where there is none.  With out == 1
// index 0 (y0 = 0) is the only one.  64-bit: y (out - 1) + in - 2 can pass 2^32.
__device__ __forceinline__ uint32_t rzt_first_at_least(uint32_t y, uint32_t in, uint32_t out)
{
    if (out <= 1u || in <= 1u) return y == 0u ? 0u : out;
    const uint64_t a = ((uint64_t)y * (out - 1u) + (in - 2u)) / (in - 1u);
    return a < out ? (uint32_t)a : out;
}

// The reduced indices a full-resolution index y gathers from along one axis (out <= in), ascending: slot 0 the index whose y1 is y (its y0 is y - 1), weight
// its t; slot 1 the one whose y0 is y, weight its u; on[] says which exist.  A tap clamped onto its own row (y0 = y1 = in - 1) has t = 0 and is listed once, by u.
struct RztOwners { uint32_t idx[2]; float wt[2]; bool on[2]; };
__device__ __forceinline__ RztOwners rzt_owners(uint32_t y, uint32_t in, uint32_t out)
{
    RztOwners o;
    o.idx[0] = o.idx[1] = 0u;
    o.wt[0] = o.wt[1] = 0.0f;
    o.on[0] = o.on[1] = false;
    if (y >= 1u) {
        const uint32_t a = rzt_first_at_least(y - 1u, in, out);
        if (a < out) {
            const RszTap t = rsz_tap(a, in, out);
            if (t.i0 == y - 1u && t.i1 == y) { o.idx[0] = a; o.wt[0] = t.t; o.on[0] = true; }
        }
    }
    const uint32_t a = rzt_first_at_least(y, in, out);
    if (a < out) {
        const RszTap t = rsz_tap(a, in, out);
        if (t.i0 == y) { o.idx[1] = a; o.wt[1] = t.u; o.on[1] = true; }
    }
    return o;
}

// IG: an image gradient is asked for (gx goes to the scratch planes); PG: a parameter gradient is.  go: 38 planes of Hr x Wr; partials: gridDim.x x PVB_PARTIAL;
// gxs: S x 3 planes of Hr x Wr, written for k < levels.
template <int MODE, bool IG, bool PG>
__global__ void __launch_bounds__(PVB_T, 2) rzt_features_bwd_kernel(const float* __restrict__ render, const float* __restrict__ warped, const float* __restrict__ feat,
                                                                   const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                                   const float* __restrict__ b2, const int32_t* __restrict__ levels, int S, uint32_t H, uint32_t W, uint32_t Hr,
                                                                   uint32_t Wr, const float* __restrict__ go, float* __restrict__ gxs, double* __restrict__ partials)
{
    __shared__ PvBwdRows<PG> rows;
    __shared__ PvBwdW1c w1c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const PvFrag f(w1, w2, c, h);
    __shared__ PvBias bias;
    pv_stage_bias(bias, b1, b2);
    PvBwdLane a;
    pv_bwd_setup<IG>(w1c, a, w1, w2, c, h);
    const int L = pv_levels_of(levels, S);
    const size_t plane = (size_t)H * W, plane_r = (size_t)Hr * Wr;
    const size_t chunks = (plane_r + PVB_CHUNK - 1) / PVB_CHUNK;
    for (size_t ck = blockIdx.x; ck < chunks; ck += gridDim.x) {          // (uniform over the workgroup: the barriers of the calls below are reached by every thread)
        const size_t qq = ck * PVB_CHUNK + (size_t)wave * PVB_B + c;
        const bool in = qq < plane_r;
        const size_t q = in ? qq : plane_r - 1;          // a lane past the frame recomputes the last pixel under a zero gradient: it adds zeros
        const uint32_t i = (uint32_t)(q / Wr), j = (uint32_t)(q - (size_t)i * Wr);
        const RszTap ty = rsz_tap(i, H, Hr), tx = rsz_tap(j, W, Wr);
        const size_t p[4] = {(size_t)ty.i0 * W + tx.i0, (size_t)ty.i0 * W + tx.i1, (size_t)ty.i1 * W + tx.i0, (size_t)ty.i1 * W + tx.i1};
        float r[4][3];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            r[n][0] = render[p[n]]; r[n][1] = render[plane + p[n]]; r[n][2] = render[2 * plane + p[n]];
        }
        const auto load = [&](int k, float (&x)[PV_INP]) {
            float xf[4][PV_INP];
#pragma unroll
            for (int n = 0; n < 4; ++n) pv_slot(warped, feat, r[n], plane, p[n], k, xf[n]);          // (each tap under its own mask)
#pragma unroll
            for (int e = 0; e < PV_IN; ++e) x[e] = rsz_blend(xf[0][e], xf[1][e], xf[2][e], xf[3][e], ty, tx);
            x[7] = 0.0f;          // the eighth input of the first layer's four k-steps
        };
        pv_f32x16 g;
#pragma unroll
        for (int m = 0; m < 16; ++m) g[m] = in ? go[(size_t)pv_ch(m, h) * plane_r + q] : 0.0f;
        if (MODE == IBGS_RSZ_MEAN && L > 1) {
            const float n = (float)L;
#pragma unroll
            for (int m = 0; m < 16; ++m) g[m] = g[m] / n;
        }
        pv_f32x16 hmax;
        uint32_t taken = 0u;
        pv_bwd_hmax<MODE>(f, bias, L, load, hmax, h);
        for (int k = 0; k < L; ++k) {
            float x[PV_INP], gx[3];
            pv_f32x16 h1, dz2;
            load(k, x);
            pv_mlp(f, bias, x, h, h1, dz2);          // dz2 = h2 for now
            pv_bwd_slot<MODE, IG>(rows, w1c, a, h1, dz2, g, hmax, taken, x, in, gx, lane, wave, c, h);
            if constexpr (IG) {
                if (in && h == 0) {          // (unmasked: the mask is the full-resolution pixel's, applied by the gather)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) gxs[((size_t)k * 3 + ch) * plane_r + q] = gx[ch];
                }
            }
        }
        if constexpr (PG) pv_bwd_end_chunk(a);
    }
    if constexpr (PG) pv_bwd_flush(rows, a, partials, lane, wave, c, h);
}

// a thread per full-resolution pixel.  gxs: S x 3 planes of Hr x Wr (slots below `levels` written by rzt_features_bwd_kernel); go: 38 planes of Hr x Wr.
__global__ void __launch_bounds__(ZT) rzt_gather_kernel(const float* __restrict__ feat, const int32_t* __restrict__ levels, int S, uint32_t H, uint32_t W, uint32_t Hr,
                                                        uint32_t Wr, const float* __restrict__ go, const float* __restrict__ gxs, float* __restrict__ d_render,
                                                        float* __restrict__ d_warped)
{
#pragma clang fp contract(off)
    const size_t plane = (size_t)H * W, plane_r = (size_t)Hr * Wr;
    const size_t p = (size_t)blockIdx.x * ZT + threadIdx.x;
    if (p >= plane) return;
    const uint32_t y = (uint32_t)(p / W), x = (uint32_t)(p - (size_t)y * W);
    const RztOwners oy = rzt_owners(y, H, Hr), ox = rzt_owners(x, W, Wr);
    const int L = pv_levels_of(levels, S);
    size_t q[4];
    float wq[4];
    bool on[4];          // reduced rows ascending, then columns
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            on[2 * a + b] = oy.on[a] && ox.on[b];
            q[2 * a + b] = (size_t)oy.idx[a] * Wr + ox.idx[b];
            wq[2 * a + b] = oy.wt[a] * ox.wt[b];
        }
    float dr[3] = {0.0f, 0.0f, 0.0f};
    if (d_render) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (on[m]) dr[ch] = fmaf(wq[m], go[(size_t)(PV_F + 3 + ch) * plane_r + q[m]], dr[ch]);
    }
    for (int k = 0; k < L; ++k) {
        const float* const fk = feat + (size_t)k * 4 * plane + p;
        const float v = (((fk[0] + fk[plane]) + fk[2 * plane]) + fk[3 * plane]) > 0.0f ? 1.0f : 0.0f;          // the sum's order is the contract
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float G = 0.0f;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (on[m]) G = fmaf(wq[m], gxs[((size_t)k * 3 + ch) * plane_r + q[m]], G);
            const float gv = G * v;
            dr[ch] -= gv;
            if (d_warped) d_warped[((size_t)k * 3 + ch) * plane + p] = gv;
        }
    }
    if (d_render) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) d_render[(size_t)ch * plane + p] = dr[ch];
    }
    if (d_warped)
        for (int k = L; k < S; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) d_warped[((size_t)k * 3 + ch) * plane + p] = 0.0f;
}

// a thread per reduced element (plane, a, b); g_out, g_pred: 3 planes of H x W, either may be null
__global__ void __launch_bounds__(ZT) rzt_upsample_bwd_kernel(const float* __restrict__ g_out, const float* __restrict__ g_pred, uint32_t H, uint32_t W, uint32_t Hr, uint32_t Wr,
                                                              float* __restrict__ d_res)
{
#pragma clang fp contract(off)
    const size_t plane = (size_t)H * W, plane_r = (size_t)Hr * Wr;
    const size_t e = (size_t)blockIdx.x * ZT + threadIdx.x;
    if (e >= 3 * plane_r) return;
    const uint32_t ch = (uint32_t)(e / plane_r);
    const size_t q = e - (size_t)ch * plane_r;
    const uint32_t a = (uint32_t)(q / Wr), b = (uint32_t)(q - (size_t)a * Wr);
    // the rows whose y0 is a - 1 or a: y0(i) = (i (Hr - 1)) / (H - 1) is monotone, so y0(i) >= m from i = ceil(m (H - 1) / (Hr - 1)) on
    uint32_t i_lo = 0u, i_hi = H - 1u, j_lo = 0u, j_hi = W - 1u;
    if (H > 1u && Hr > 1u) {
        i_lo = a >= 1u ? (uint32_t)(((uint64_t)(a - 1u) * (H - 1u) + (Hr - 2u)) / (Hr - 1u)) : 0u;
        const uint64_t past = ((uint64_t)(a + 1u) * (H - 1u) + (Hr - 2u)) / (Hr - 1u);          // the first row whose y0 is >= a + 1
        i_hi = past < H ? (uint32_t)past - 1u : H - 1u;          // (past >= 1: a + 1 >= 1)
    }
    if (W > 1u && Wr > 1u) {
        j_lo = b >= 1u ? (uint32_t)(((uint64_t)(b - 1u) * (W - 1u) + (Wr - 2u)) / (Wr - 1u)) : 0u;
        const uint64_t past = ((uint64_t)(b + 1u) * (W - 1u) + (Wr - 2u)) / (Wr - 1u);
        j_hi = past < W ? (uint32_t)past - 1u : W - 1u;
    }
    double acc = 0.0;
    for (uint32_t i = i_lo; i <= i_hi; ++i) {
        const RszTap ty = rsz_tap(i, Hr, H);
        if (ty.i0 != a && ty.i1 != a) continue;
        const double wy = (double)(ty.i0 == a ? ty.u : ty.t);          // (y0 = y1 = a on the clamp: t = 0, the weight is u)
        for (uint32_t j = j_lo; j <= j_hi; ++j) {
            const RszTap tx = rsz_tap(j, Wr, W);
            if (tx.i0 != b && tx.i1 != b) continue;
            const double wx = (double)(tx.i0 == b ? tx.u : tx.t);
            const size_t o = (size_t)ch * plane + (size_t)i * W + j;
            const float g = g_out ? (g_pred ? g_out[o] + g_pred[o] : g_out[o]) : g_pred[o];
            acc = fma(wy * wx, (double)g, acc);          // (wy wx is exact in f64)
        }
    }
    d_res[e] = (float)acc;
}

// who == nullptr: silent (the size query)
static bool rzt_features_shape_ok(const char* who, int64_t S, int64_t H, int64_t W, int64_t Hr, int64_t Wr)
{
    if (S < 1 || S > IBGS_RSZ_MAX_SRC) {
        if (who) set_error("%s: %lld sources out of range (1 .. %d)", who, (long long)S, IBGS_RSZ_MAX_SRC);
        return false;
    }
    if (!rsz_sides_ok(who, H, W, Hr, Wr)) return false;
    if (Hr > H || Wr > W) {
        if (who) set_error("%s: a reduced frame of %lld x %lld is larger than the frame of %lld x %lld: training an upscaled network is not supported", who, (long long)Hr,
                           (long long)Wr, (long long)H, (long long)W);
        return false;
    }
    return true;
}

struct RztScratch {
    double* partials;         // workgroups of the reduced-resolution kernel x PVB_PARTIAL
    float* gx;                // S x 3 planes of Hr x Wr
    static RztScratch carve(char* base, size_t S, size_t plane_r, size_t* total)
    {
        RztScratch d;
        Carver c(base);
        d.partials = c.take<double>((size_t)pv_bwd_groups(plane_r) * PVB_PARTIAL);
        d.gx = c.take<float>(S * 3 * plane_r);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return d;
    }
};

template <int MODE>
static void rzt_launch_bwd(hipStream_t st, unsigned groups, bool ig, bool pg, const float* render, const float* warped, const float* feat, const float* w1, const float* b1,
                           const float* w2, const float* b2, const int32_t* levels, int S, uint32_t H, uint32_t W, uint32_t Hr, uint32_t Wr, const float* go, float* gxs,
                           double* partials)
{
    if (ig && pg) hipLaunchKernelGGL((rzt_features_bwd_kernel<MODE, true, true>), dim3(groups), dim3(PVB_T), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, H, W, Hr, Wr, go, gxs, partials);
    else if (pg) hipLaunchKernelGGL((rzt_features_bwd_kernel<MODE, false, true>), dim3(groups), dim3(PVB_T), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, H, W, Hr, Wr, go, gxs, partials);
    else hipLaunchKernelGGL((rzt_features_bwd_kernel<MODE, true, false>), dim3(groups), dim3(PVB_T), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, H, W, Hr, Wr, go, gxs, partials);
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_rzt_required_scratch(int64_t S, int64_t H, int64_t W, int64_t Hr, int64_t Wr)
{
    size_t total = 0;
    if (!rzt_features_shape_ok(nullptr, S, H, W, Hr, Wr)) return 0;
    RztScratch::carve(nullptr, (size_t)S, (size_t)Hr * (size_t)Wr, &total);
    return total;
}

int32_t ibgs_rzt_features_backward(void* stream, int32_t S, int32_t H, int32_t W, int32_t Hr, int32_t Wr, int32_t mode, const float* render, const float* warped,
                                   const float* cam_feat, const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* levels,
                                   const float* grad_out, float* grad_render, float* grad_warped, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                                   void* scratch, size_t scratch_bytes)
{
    const char* const who = "rzt_features_backward";
    if (!rzt_features_shape_ok(who, S, H, W, Hr, Wr)) return -IBGS_ERR_INVALID;
    if (mode != IBGS_RSZ_MEAN && mode != IBGS_RSZ_MAX) { set_error("%s: mode %d is neither IBGS_RSZ_MEAN nor IBGS_RSZ_MAX", who, mode); return -IBGS_ERR_INVALID; }
    if (!render || !warped || !cam_feat) { set_error("%s: null image", who); return -IBGS_ERR_INVALID; }
    if (!w1 || !b1 || !w2 || !b2) { set_error("%s: null parameters", who); return -IBGS_ERR_INVALID; }
    if (!levels) { set_error("%s: null levels: the device word of cagg_levels is required", who); return -IBGS_ERR_INVALID; }
    if (!grad_out) { set_error("%s: null grad_out", who); return -IBGS_ERR_INVALID; }
    const bool ig = grad_render || grad_warped, pg = grad_w1 || grad_b1 || grad_w2 || grad_b2;
    if (!ig && !pg) { set_error("%s: null outputs: no gradient is asked for", who); return -IBGS_ERR_INVALID; }
    const size_t plane = (size_t)H * (size_t)W, plane_r = (size_t)Hr * (size_t)Wr;
    size_t need = 0;
    const RztScratch sc = RztScratch::carve(static_cast<char*>(scratch), (size_t)S, plane_r, &need);
    if (!arena_ok(who, "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned groups = pv_bwd_groups(plane_r);
    if (mode == IBGS_RSZ_MEAN)
        rzt_launch_bwd<IBGS_RSZ_MEAN>(st, groups, ig, pg, render, warped, cam_feat, w1, b1, w2, b2, levels, (int)S, (uint32_t)H, (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr, grad_out,
                                      ig ? sc.gx : nullptr, pg ? sc.partials : nullptr);
    else
        rzt_launch_bwd<IBGS_RSZ_MAX>(st, groups, ig, pg, render, warped, cam_feat, w1, b1, w2, b2, levels, (int)S, (uint32_t)H, (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr, grad_out,
                                     ig ? sc.gx : nullptr, pg ? sc.partials : nullptr);
    IBGS_HIP(hipGetLastError());
    if (pg) {
        pv_launch_final(st, sc.partials, (int)groups, grad_w1, grad_b1, grad_w2, grad_b2);
        IBGS_HIP(hipGetLastError());
    }
    if (ig) {
        hipLaunchKernelGGL(rzt_gather_kernel, dim3((unsigned)((plane + ZT - 1) / ZT)), dim3(ZT), 0, st, cam_feat, levels, (int)S, (uint32_t)H, (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr,
                           grad_out, sc.gx, grad_render, grad_warped);          // (at most 2^24 workgroups)
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

int32_t ibgs_rzt_upsample_backward(void* stream, int32_t H, int32_t W, int32_t Hr, int32_t Wr, const float* grad_residual_out, const float* grad_image_pred,
                                   float* grad_residual_r)
{
    const char* const who = "rzt_upsample_backward";
    if (!rsz_sides_ok(who, H, W, Hr, Wr)) return -IBGS_ERR_INVALID;
    if (!grad_residual_out && !grad_image_pred) { set_error("%s: null gradients: grad_residual_out and grad_image_pred are both null", who); return -IBGS_ERR_INVALID; }
    if (!grad_residual_r) { set_error("%s: null outputs: grad_residual_r is required", who); return -IBGS_ERR_INVALID; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t elems = 3 * (size_t)Hr * (size_t)Wr;          // (at most 3 x 2^32: 2^26 workgroups)
    hipLaunchKernelGGL(rzt_upsample_bwd_kernel, dim3((unsigned)((elems + ZT - 1) / ZT)), dim3(ZT), 0, st, grad_residual_out, grad_image_pred, (uint32_t)H, (uint32_t)W, (uint32_t)Hr,
                       (uint32_t)Wr, grad_residual_r);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
