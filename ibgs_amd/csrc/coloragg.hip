// The per-view front end of the reference's colour aggregation network on the device (C ABI: include/ibgs_color_agg.h; Python: ibgs_amd/coloragg.py):
// what fuse_color and ColorFusionResidualNet.forward do between the rasterizer's planes and the input of the hourglass CNN
// (color_aggregation_network.py:102-133, 156-198, 229-233) -- permutes, a mask, a subtraction, a concatenation into (HW, M, 7), two Linear + ReLU over HW M
// rows of 32 floats, a mean over the views, a transpose and a concatenation into (1, 38, H, W), and one host sync to count the slot levels -- as one kernel
// forward and one backward that keep the 64 intermediate floats per pixel and source in registers.  Nothing waits for the host: the level count stays in a
// device word.
//
// CONTRACT
//   levels     min(slots of `warped` with any value != 0, nb_visible_src_frames, S), in a device word; the first `levels` slots are used.
//   slot k     v = (((f0 + f1) + f2) + f3) > 0 in float32, in that order (cam_feat is signed); x = [(warped - render) v, f0 .. f3];
//              h1 = relu(w1 x + b1), h2 = relu(w2 h1 + b2): shared/pv_mlp.h, which resample.hip and rsztrain.hip run too, states the chain and what its bits rest on.
//   agg        mean: ((h2_0 + h2_1) + ..) / levels; max: the maximum over k; zeros when levels == 0.  out = [agg, camera_ray, render].
//   backward   recomputes h1 and h2 with the same instructions (the same bits), then dz2 = g (h2 > 0) with g = grad_out / levels (mean) or grad_out at the
//              first slot attaining the maximum (max), dz1 = (w2^T dz2) (h1 > 0), dx = w1^T dz1; grad_warped[3k + c] = dx[c] v, grad_render[c] =
//              grad_out[35 + c] - sum_k dx[c] v; slots from `levels` on: zeros.
//   parameter gradients   dW2 = sum_p dz2 (x) h1, db2 = sum_p dz2, dW1 = sum_p dz1 (x) x, db1 = sum_p dz1.  Each wave sums its own 32 pixels of every chunk
//              and slot in a fixed order: dW2 as the matrix cores' f32 fma chain over one chunk's pixels and slots, from there on in f64; the other three in
//              f64 throughout (the products are exact there).  The four waves of a workgroup are added in order and the workgroup's 1312 f64 sums go to the
//              scratch arena; cagg_final_kernel adds the workgroups: sixteen strided series per element, then those in order, one rounding to f32 at the
//              end.  No float atomics.
//
// THE 32 x 32 PRODUCTS run on the matrix cores in exact f32, in the lane and register map of shared/pv_mlp.h: a wave holds 32 pixels, a 16-register tile's
// rows are channels and its columns pixels, and a product's result is the next one's B operand as it stands.  The backward's own products (w2^T dz2, the
// weight gradient) use the same map, so h1, h2, dz2, dz1 never leave the registers.  Only the weight gradient, whose long dimension is the pixels, goes
// through LDS: each lane stores its pixel's dz2, h1 and dz1 as rows and the wave reads them back a pixel pair per k-step.
//
// KERNELS
//   cagg_levels_kernel   S x B workgroups scan the slots; a workgroup that found a value ORs its slot's bit into a word, takes a ticket, and the last one
//                        writes the count (integer atomics on two words the entry point zeroes with a memset in front).
//   cagg_fwd_kernel      256 threads = 4 waves of 32 pixels; 20 MFMA per wave and slot.
//   cagg_bwd_kernel      the same over a capped grid that walks the frame in chunks of 128 pixels; 52 MFMA per wave and slot with parameter gradients.
//   cagg_final_kernel    82 workgroups: 16 elements each.
// What bounds them, storing against recomputing, and the matrix cores against the VALU: DESIGN.md section 14.
//
// WHO STATES WHAT: shared/pv_mlp.h the slot and both layers (resample.hip and rsztrain.hip run them too); shared/pv_mlp_bwd.h the backward's workgroup geometry,
// the per-slot backward, the parameter sums and the layout of the partials, for cagg_bwd_kernel and for rsztrain.hip's rzt_features_bwd_kernel.  This file: the
// level count, the forward, how the backward loads a slot (one pixel) and what it does with gx (times v, to grad_warped and grad_render), and cagg_final_kernel
// with its launcher pv_launch_final, which rsztrain.hip calls too: the final pass has one owner.
#include "common.h"
#include "shared/pv_mlp_bwd.h"
#include "../../include/ibgs_color_agg.h"

namespace ibgs {

constexpr int CT = 256;                              // the forward: threads per workgroup (the backward's geometry is shared/pv_mlp_bwd.h's)
constexpr int CWAVES = CT / 64;
constexpr int CB = 32;                               // pixels per wave
constexpr int CHUNK = CWAVES * CB;                   // pixels per workgroup and step
constexpr int CAGG_FWD_MAX_GROUPS = 4096;
constexpr int LV_THREADS = 256, LV_MAX_BLOCKS = 128; // level count: workgroups per slot
static_assert(PV_F == IBGS_CAGG_FEATURES && CB == PV_F && IBGS_CAGG_MEAN == PV_MEAN && IBGS_CAGG_MAX == PV_MAX, "the lane maps below, and the shared backward's modes");

// slot's grid: S x per_slot workgroups; state[0]: the slots that hold a value, state[1]: workgroups done (both zero on entry)
__global__ void __launch_bounds__(LV_THREADS) cagg_levels_kernel(const float* __restrict__ warped, size_t slot_elems, int per_slot, int S, int nb, uint32_t* __restrict__ state,
                                                                 int32_t* __restrict__ levels_out)
{
    const int slot = (int)(blockIdx.x / (unsigned)per_slot), b = (int)(blockIdx.x - (unsigned)slot * (unsigned)per_slot);
    const float* const base = warped + (size_t)slot * slot_elems;
    int any = 0;
    for (size_t i = (size_t)b * LV_THREADS + threadIdx.x; i < slot_elems; i += (size_t)per_slot * LV_THREADS) any |= base[i] != 0.0f ? 1 : 0;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        if (any) __hip_atomic_fetch_or(&state[0], 1u << slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // release what this workgroup found, acquire what the others did: the last ticket sees every bit
        const uint32_t ticket = __hip_atomic_fetch_add(&state[1], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == gridDim.x - 1) {
            const int n = __popc(__hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            *levels_out = min(n, min(nb, S));
        }
    }
}

// a wave per block of 32 pixels (wave-uniform bounds: the matrix instructions run with every lane on; a lane past the frame recomputes the last pixel)
template <int MODE>
__global__ void __launch_bounds__(CT) cagg_fwd_kernel(const float* __restrict__ render, const float* __restrict__ warped, const float* __restrict__ feat,
                                                      const float* __restrict__ ray, const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, const int32_t* __restrict__ levels, int S, size_t plane,
                                                      float* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const PvFrag f(w1, w2, c, h);
    __shared__ PvBias bias;
    pv_stage_bias(bias, b1, b2);
    const int L = pv_levels_of(levels, S);
    const size_t blocks = (plane + CB - 1) / CB;
    for (size_t b = (size_t)blockIdx.x * CWAVES + wave; b < blocks; b += (size_t)gridDim.x * CWAVES) {
        const size_t q = b * CB + c;
        const bool in = q < plane;
        const size_t p = in ? q : plane - 1;
        const float r[3] = {render[p], render[plane + p], render[2 * plane + p]};
        pv_f32x16 agg;
#pragma unroll
        for (int j = 0; j < 16; ++j) agg[j] = 0.0f;
        for (int k = 0; k < L; ++k) {
            float x[PV_INP];
            pv_f32x16 h1, h2;
            pv_slot(warped, feat, r, plane, p, k, x);
            pv_mlp(f, bias, x, h, h1, h2);
#pragma unroll
            for (int j = 0; j < 16; ++j) agg[j] = MODE == IBGS_CAGG_MEAN ? agg[j] + h2[j] : fmaxf(agg[j], h2[j]);          // (h2 >= 0: the maximum may start from 0)
        }
        if (MODE == IBGS_CAGG_MEAN && L > 1) {
            const float n = (float)L;
#pragma unroll
            for (int j = 0; j < 16; ++j) agg[j] = agg[j] / n;
        }
        if (in) {
#pragma unroll
            for (int j = 0; j < 16; ++j) out[(size_t)pv_ch(j, h) * plane + p] = agg[j];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {          // half 0 passes the ray on, half 1 the colour
                const float* const src = h ? render : ray;
                out[(size_t)(PV_F + 3 * h + ch) * plane + p] = src[(size_t)ch * plane + p];
            }
        }
    }
}

// IG: an image gradient is asked for; PG: a parameter gradient is.  go: 38 planes; partials: gridDim.x x PVB_PARTIAL
template <int MODE, bool IG, bool PG>
__global__ void __launch_bounds__(PVB_T, 2) cagg_bwd_kernel(const float* __restrict__ render, const float* __restrict__ warped, const float* __restrict__ feat,
                                                         const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, const int32_t* __restrict__ levels, int S, size_t plane, const float* __restrict__ go,
                                                         float* __restrict__ d_render, float* __restrict__ d_warped, double* __restrict__ partials)
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
    const size_t chunks = (plane + PVB_CHUNK - 1) / PVB_CHUNK;
    for (size_t ck = blockIdx.x; ck < chunks; ck += gridDim.x) {          // (uniform over the workgroup: the barriers of the calls below are reached by every thread)
        const size_t q = ck * PVB_CHUNK + (size_t)wave * PVB_B + c;
        const bool in = q < plane;
        const size_t p = in ? q : plane - 1;          // a lane past the frame recomputes the last pixel under a zero gradient: it adds zeros
        const float r[3] = {render[p], render[plane + p], render[2 * plane + p]};
        const auto load = [&](int k, float (&x)[PV_INP]) { return pv_slot(warped, feat, r, plane, p, k, x); };          // -> v
        pv_f32x16 g;
#pragma unroll
        for (int j = 0; j < 16; ++j) g[j] = in ? go[(size_t)pv_ch(j, h) * plane + p] : 0.0f;
        if (MODE == IBGS_CAGG_MEAN && L > 1) {
            const float n = (float)L;
#pragma unroll
            for (int j = 0; j < 16; ++j) g[j] = g[j] / n;
        }
        pv_f32x16 hmax;
        uint32_t taken = 0u;
        pv_bwd_hmax<MODE>(f, bias, L, load, hmax, h);
        float dr[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < L; ++k) {
            float x[PV_INP], gx[3];
            pv_f32x16 h1, dz2;
            const float v = load(k, x);
            pv_mlp(f, bias, x, h, h1, dz2);          // dz2 = h2 for now
            pv_bwd_slot<MODE, IG>(rows, w1c, a, h1, dz2, g, hmax, taken, x, in, gx, lane, wave, c, h);
            if constexpr (IG) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float gv = gx[ch] * v;
                    dr[ch] -= gv;
                    if (d_warped && in && h == 0) d_warped[((size_t)k * 3 + ch) * plane + p] = gv;
                }
            }
        }
        if constexpr (PG) pv_bwd_end_chunk(a);
        if (IG && in && h == 0) {
            if (d_render) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) d_render[(size_t)ch * plane + p] = go[(size_t)(PV_F + 3 + ch) * plane + p] + dr[ch];
            }
            if (d_warped)
                for (int k = L; k < S; ++k)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) d_warped[((size_t)k * 3 + ch) * plane + p] = 0.0f;
        }
    }
    if constexpr (PG) pv_bwd_flush(rows, a, partials, lane, wave, c, h);
}

// element e of the workgroups' sums: series s adds the workgroups s, s + 16, .. in that order in f64, thread e adds the series in order
__global__ void __launch_bounds__(PVB_T) cagg_final_kernel(const double* __restrict__ partials, int groups, float* __restrict__ d_w1, float* __restrict__ d_b1,
                                                           float* __restrict__ d_w2, float* __restrict__ d_b2)
{
    __shared__ double s_sum[PVB_FIN_SERIES][PVB_FIN_ELEMS];
    const int el = threadIdx.x & (PVB_FIN_ELEMS - 1), series = threadIdx.x / PVB_FIN_ELEMS;
    const int e = blockIdx.x * PVB_FIN_ELEMS + el;
    double a = 0.0;
    for (int g = series; g < groups; g += PVB_FIN_SERIES) a += partials[(size_t)g * PVB_PARTIAL + e];
    s_sum[series][el] = a;
    __syncthreads();
    if (threadIdx.x < PVB_FIN_ELEMS) {
        double t = s_sum[0][el];
        for (int k = 1; k < PVB_FIN_SERIES; ++k) t += s_sum[k][el];
        const float v = (float)t;
        if (e < PV_F * PV_INP) {
            const int i = e >> 3, c = e & 7;
            if (c < PV_IN) { if (d_w1) d_w1[i * PV_IN + c] = v; }
            else if (d_b1) d_b1[i] = v;
        } else if (e < PV_F * PV_INP + PV_F * PV_F) {
            if (d_w2) d_w2[e - PV_F * PV_INP] = v;
        } else if (d_b2) d_b2[e - PV_F * PV_INP - PV_F * PV_F] = v;
    }
}

void pv_launch_final(hipStream_t st, const double* partials, int groups, float* d_w1, float* d_b1, float* d_w2, float* d_b2)
{
    hipLaunchKernelGGL(cagg_final_kernel, dim3(PVB_PARTIAL / PVB_FIN_ELEMS), dim3(PVB_T), 0, st, partials, groups, d_w1, d_b1, d_w2, d_b2);
}

// who == nullptr: silent (the size query)
static bool cagg_shape_ok(const char* who, int64_t S, int64_t H, int64_t W, size_t* plane)
{
    if (S < 1 || S > IBGS_CAGG_MAX_SRC || H < 1 || W < 1 || H > IBGS_CAGG_MAX_SIDE || W > IBGS_CAGG_MAX_SIDE) {
        if (who) set_error("%s: %lld sources of %lld x %lld out of range (1 .. %d sources, sides 1 .. %d)", who, (long long)S, (long long)H, (long long)W, IBGS_CAGG_MAX_SRC,
                           IBGS_CAGG_MAX_SIDE);
        return false;
    }
    *plane = (size_t)H * (size_t)W;
    return true;
}

static bool cagg_mode_ok(const char* who, int32_t mode)
{
    if (mode == IBGS_CAGG_MEAN || mode == IBGS_CAGG_MAX) return true;
    set_error("%s: mode %d is neither IBGS_CAGG_MEAN nor IBGS_CAGG_MAX", who, mode);
    return false;
}

struct CaggScratch {
    uint32_t* state;          // 2 words: the level count's flags and tickets
    double* partials;         // workgroups of the backward x PVB_PARTIAL
    static CaggScratch carve(char* base, size_t plane, size_t* total)
    {
        CaggScratch d;
        Carver c(base);
        d.state = c.take<uint32_t>(2);
        d.partials = c.take<double>((size_t)pv_bwd_groups(plane) * PVB_PARTIAL);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return d;
    }
};

template <int MODE>
static void cagg_launch_bwd(hipStream_t st, unsigned groups, bool ig, bool pg, const float* render, const float* warped, const float* feat, const float* w1, const float* b1,
                            const float* w2, const float* b2, const int32_t* levels, int S, size_t plane, const float* go, float* d_render, float* d_warped, double* partials)
{
    if (ig && pg) hipLaunchKernelGGL((cagg_bwd_kernel<MODE, true, true>), dim3(groups), dim3(PVB_T), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, plane, go, d_render, d_warped, partials);
    else if (pg) hipLaunchKernelGGL((cagg_bwd_kernel<MODE, false, true>), dim3(groups), dim3(PVB_T), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, plane, go, d_render, d_warped, partials);
    else hipLaunchKernelGGL((cagg_bwd_kernel<MODE, true, false>), dim3(groups), dim3(PVB_T), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, plane, go, d_render, d_warped, partials);
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_cagg_required_scratch(int64_t S, int64_t H, int64_t W)
{
    size_t plane = 0, total = 0;
    if (!cagg_shape_ok(nullptr, S, H, W, &plane)) return 0;
    CaggScratch::carve(nullptr, plane, &total);
    return total;
}

int32_t ibgs_cagg_levels(void* stream, int32_t S, int32_t H, int32_t W, const float* warped, int32_t nb_visible_src_frames, int32_t* levels_out, void* scratch,
                         size_t scratch_bytes)
{
    size_t plane = 0, need = 0;
    if (!cagg_shape_ok("cagg_levels", S, H, W, &plane)) return -IBGS_ERR_INVALID;
    if (nb_visible_src_frames < 1) { set_error("cagg_levels: nb_visible_src_frames %d out of range (>= 1)", nb_visible_src_frames); return -IBGS_ERR_INVALID; }
    if (!warped) { set_error("cagg_levels: null image"); return -IBGS_ERR_INVALID; }
    if (!levels_out) { set_error("cagg_levels: null outputs: levels_out is required"); return -IBGS_ERR_INVALID; }
    const CaggScratch sc = CaggScratch::carve(static_cast<char*>(scratch), plane, &need);
    if (!arena_ok("cagg_levels", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t slot_elems = 3 * plane;
    size_t per_slot = (slot_elems + (size_t)LV_THREADS * 16 - 1) / ((size_t)LV_THREADS * 16);
    if (per_slot > (size_t)LV_MAX_BLOCKS) per_slot = LV_MAX_BLOCKS;
    IBGS_HIP(hipMemsetAsync(sc.state, 0, 2 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(cagg_levels_kernel, dim3((unsigned)((size_t)S * per_slot)), dim3(LV_THREADS), 0, st, warped, slot_elems, (int)per_slot, (int)S, (int)nb_visible_src_frames,
                       sc.state, levels_out);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_cagg_forward(void* stream, int32_t S, int32_t H, int32_t W, int32_t mode, const float* render, const float* warped, const float* cam_feat,
                          const float* camera_ray, const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* levels, float* out)
{
    size_t plane = 0;
    if (!cagg_shape_ok("cagg_forward", S, H, W, &plane) || !cagg_mode_ok("cagg_forward", mode)) return -IBGS_ERR_INVALID;
    if (!render || !warped || !cam_feat || !camera_ray) { set_error("cagg_forward: null image"); return -IBGS_ERR_INVALID; }
    if (!w1 || !b1 || !w2 || !b2) { set_error("cagg_forward: null parameters"); return -IBGS_ERR_INVALID; }
    if (!levels) { set_error("cagg_forward: null levels: the device word of cagg_levels is required"); return -IBGS_ERR_INVALID; }
    if (!out) { set_error("cagg_forward: null outputs: out is required"); return -IBGS_ERR_INVALID; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    size_t groups = (plane + CHUNK - 1) / CHUNK;
    if (groups > (size_t)CAGG_FWD_MAX_GROUPS) groups = CAGG_FWD_MAX_GROUPS;
    if (mode == IBGS_CAGG_MEAN)
        hipLaunchKernelGGL((cagg_fwd_kernel<IBGS_CAGG_MEAN>), dim3((unsigned)groups), dim3(CT), 0, st, render, warped, cam_feat, camera_ray, w1, b1, w2, b2, levels, (int)S, plane, out);
    else
        hipLaunchKernelGGL((cagg_fwd_kernel<IBGS_CAGG_MAX>), dim3((unsigned)groups), dim3(CT), 0, st, render, warped, cam_feat, camera_ray, w1, b1, w2, b2, levels, (int)S, plane, out);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_cagg_backward(void* stream, int32_t S, int32_t H, int32_t W, int32_t mode, const float* render, const float* warped, const float* cam_feat,
                           const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* levels, const float* grad_out, float* grad_render,
                           float* grad_warped, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, void* scratch, size_t scratch_bytes)
{
    size_t plane = 0, need = 0;
    if (!cagg_shape_ok("cagg_backward", S, H, W, &plane) || !cagg_mode_ok("cagg_backward", mode)) return -IBGS_ERR_INVALID;
    if (!render || !warped || !cam_feat) { set_error("cagg_backward: null image"); return -IBGS_ERR_INVALID; }
    if (!w1 || !b1 || !w2 || !b2) { set_error("cagg_backward: null parameters"); return -IBGS_ERR_INVALID; }
    if (!levels) { set_error("cagg_backward: null levels: the device word of cagg_levels is required"); return -IBGS_ERR_INVALID; }
    if (!grad_out) { set_error("cagg_backward: null grad_out"); return -IBGS_ERR_INVALID; }
    const bool ig = grad_render || grad_warped, pg = grad_w1 || grad_b1 || grad_w2 || grad_b2;
    if (!ig && !pg) { set_error("cagg_backward: null outputs: no gradient is asked for"); return -IBGS_ERR_INVALID; }
    CaggScratch sc = CaggScratch::carve(static_cast<char*>(scratch), plane, &need);
    if (pg && !arena_ok("cagg_backward", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    if (!pg) sc.partials = nullptr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned groups = pv_bwd_groups(plane);
    if (mode == IBGS_CAGG_MEAN)
        cagg_launch_bwd<IBGS_CAGG_MEAN>(st, groups, ig, pg, render, warped, cam_feat, w1, b1, w2, b2, levels, (int)S, plane, grad_out, grad_render, grad_warped, sc.partials);
    else
        cagg_launch_bwd<IBGS_CAGG_MAX>(st, groups, ig, pg, render, warped, cam_feat, w1, b1, w2, b2, levels, (int)S, plane, grad_out, grad_render, grad_warped, sc.partials);
    IBGS_HIP(hipGetLastError());
    if (pg) {
        pv_launch_final(st, sc.partials, (int)groups, grad_w1, grad_b1, grad_w2, grad_b2);
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
