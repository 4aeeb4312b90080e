// The per-view MLP of the colour aggregation network on the matrix cores: one slot's seven inputs -> relu(w1 x + b1) -> relu(w2 h1 + b2), 32 wide, for the
// 32 pixels of a wave.  The one statement of the chain that coloragg.hip (forward, and the backward's recomputation), resample.hip (the forward at a reduced
// resolution) and rsztrain.hip (that forward's recomputation in its backward) run: all are meant to be the same function of a slot, bit for bit.  The backward
// of the chain is pv_mlp_bwd.h's, which includes this header; resample.hip, forward only, does not compile it.  ibgs_amd/_build.py lists this header under the
// three units (UNIT_HEADERS), and under no other: it sits in a subdirectory of csrc/ so that no other unit's profile stamp holds it.
// Device code only.
//
// WHAT THE BITS REST ON
//   slot k     v = (((f0 + f1) + f2) + f3) > 0 in float32, in that order (cam_feat is signed); x = [(warped - render) v, f0 .. f3, 0], each difference and
//              product rounded on its own (pv_slot says `fp contract(off)` itself).
//   layers     h1 = relu(w1 x + b1), h2 = relu(w2 h1 + b2): each element an f32 fma chain started from the bias, its terms in the k order of the matrix
//              cores: v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain, at the vector fp32 rate.
//   the map    A wave holds 32 pixels: lane l = (pixel l & 31, half h = l >> 5), and register r of a 16-register tile belongs to channel
//              pv_ch(r, h) = (r & 3) + 8 (r >> 2) + 4 h: the layout in which the instruction leaves a result whose rows are channels and whose columns are
//              pixels.  That result is the NEXT product's B operand as it stands -- k-step kk takes register kk, i.e. the channels pv_ch(kk, 0) and
//              pv_ch(kk, 1) -- so the weights are loaded once per wave in that (permuted) k order, 16 registers per matrix, and h1 and h2 never leave the
//              registers.  The first layer's k-step kk takes the inputs 2 kk and 2 kk + 1; the eighth input is the zero of the slot's row.
//   every lane on   the matrix instructions run with the whole wave: a caller's bounds are wave-uniform, and a lane past the frame recomputes a pixel inside it.
#pragma once
#include "../common.h"

namespace ibgs {

typedef float pv_f32x16 __attribute__((ext_vector_type(16)));

constexpr int PV_F = 32;                             // feature width: the rows of both products, and the pixels of a wave
constexpr int PV_IN = 7, PV_INP = 8;                 // inputs of the first layer, and the row they are kept in

// the channel of register r of a tile in half h
__device__ __forceinline__ constexpr int pv_ch(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ pv_f32x16 pv_mfma(float a, float b, pv_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// A lane's share of the weights, loaded once: the A operands of the two layers (row = this lane's l & 31, k-step kk = the inputs 2 kk + h of the first
// layer and the channels pv_ch(kk, h) of the second).
struct PvFrag {
    float a1[4], a2[16];
    __device__ __forceinline__ PvFrag(const float* __restrict__ w1, const float* __restrict__ w2, int row, int h)
    {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) a1[kk] = 2 * kk + h < PV_IN ? w1[row * PV_IN + 2 * kk + h] : 0.0f;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) a2[kk] = w2[row * PV_F + pv_ch(kk, h)];
    }
};

// The biases as the tiles the chains start from: [layer][half][register], the same for every pixel, so they live in LDS and are read as broadcasts
// (32 registers per lane otherwise).  Ends with a barrier.
struct __attribute__((aligned(16))) PvBias { float t[2][2][16]; };
__device__ __forceinline__ void pv_stage_bias(PvBias& s, const float* __restrict__ b1, const float* __restrict__ b2)
{
    if (threadIdx.x < 64) {
        const int layer = threadIdx.x >> 5, hh = (threadIdx.x >> 4) & 1, r = threadIdx.x & 15;
        s.t[layer][hh][r] = (layer ? b2 : b1)[pv_ch(r, hh)];
    }
    __syncthreads();
}
__device__ __forceinline__ pv_f32x16 pv_bias_tile(const PvBias& s, int layer, int h)
{
    pv_f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(&s.t[layer][h][i]);
        z[i] = v.x; z[i + 1] = v.y; z[i + 2] = v.z; z[i + 3] = v.w;
    }
    return z;
}

// the features of slot k of the full-resolution pixel p, masked by that pixel's own v; x[7] = 0: the eighth input of the first layer's four k-steps.
// -> v as a float
__device__ __forceinline__ float pv_slot(const float* __restrict__ warped, const float* __restrict__ feat, const float (&r)[3], size_t plane, size_t p, int k, float (&x)[PV_INP])
{
#pragma clang fp contract(off)
    const float* const f = feat + (size_t)k * 4 * plane + p;
    const float* const w = warped + (size_t)k * 3 * plane + p;
    x[3] = f[0]; x[4] = f[plane]; x[5] = f[2 * plane]; x[6] = f[3 * plane];
    const float v = (((x[3] + x[4]) + x[5]) + x[6]) > 0.0f ? 1.0f : 0.0f;          // the sum's order is the contract
    x[0] = (w[0] - r[0]) * v; x[1] = (w[plane] - r[1]) * v; x[2] = (w[2 * plane] - r[2]) * v;
    x[7] = 0.0f;
    return v;
}

// both layers of the lane's pixel: its 16 channels of h1 and of h2 (every caller runs the same instructions: the same bits)
__device__ __forceinline__ void pv_mlp(const PvFrag& f, const PvBias& bias, const float (&x)[PV_INP], int h, pv_f32x16& h1, pv_f32x16& h2)
{
    pv_f32x16 z = pv_bias_tile(bias, 0, h);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) z = pv_mfma(f.a1[kk], h ? x[2 * kk + 1] : x[2 * kk], z);
#pragma unroll
    for (int r = 0; r < 16; ++r) h1[r] = z[r] > 0.0f ? z[r] : 0.0f;
    z = pv_bias_tile(bias, 1, h);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) z = pv_mfma(f.a2[kk], h1[kk], z);
#pragma unroll
    for (int r = 0; r < 16; ++r) h2[r] = z[r] > 0.0f ? z[r] : 0.0f;
}

}  // namespace ibgs
