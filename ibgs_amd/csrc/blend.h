// The per-pair arithmetic that the blend kernels share (internal; render_fwd.hip and render_bwd.hip include it, nobody else).
//
// The forward and the backward visit exactly the same (pixel, Gaussian) pairs because both decide on the same number, E = -log2(o G) of the pair,
// formed by the SAME expressions in the same order: the ones below.  A wave's lane holds one pixel of each of its PPL 8 x 8 quadrants; what depends
// on how the quadrants lie in the tile (their pixel offsets, the shift of E and of conic * d from quadrant 0 to the others, the moments of the lane's
// pixels about its quadrant-0 pixel) is written here once, and so are the pieces that the two backward bodies have in common (record staging, the
// "k < n_contrib" masks, the head of the reference-arithmetic branch).  Every function is __device__ __forceinline__, holds no state and touches no LDS.
// Every helper has the shape under which its callers' assembly is what the open-coded lines gave (docs/EXPERIMENTS.md section 16 has the per-kernel
// comparison and the shapes that failed it): the pixel mapping and the chunk mask are plain value functions for that reason, and the backward's per-pixel
// prologue and the order words of three of its entry kernels stay written out in render_bwd.hip.
#pragma once
#include "common.h"

namespace ibgs {

__device__ __forceinline__ float quant8(float a, int quant) { return quant ? floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f) : a; }

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
    return v;
}

// Slot `slot` of a launch order (tile_order_kernel, render_bwd.hip): its tile, without the flag that says which wave shape should walk it; false: an empty slot
// (0xFFFFFFFF), `tile` untouched.  (render_fwd_kernel and the two *_risk_kernel; the other backward entries decode in place, see render_bwd.hip.)
__device__ __forceinline__ bool ordered_tile(const uint32_t* __restrict__ order, uint32_t slot, int& tile)
{
    const uint32_t t = order[slot];
    if (t == 0xFFFFFFFFu) return false;
    tile = (int)(t & ~ORDER_SPLIT_BIT);
    return true;
}

// ---- where a lane's pixels are -------------------------------------------------------------------------------------------------------------
// Lane l holds pixel (l % 8, l / 8) of an 8 x 8 quadrant; quadrant qq of a tile (0..3) lies at ((qq & 1) * 8, (qq >> 1) * 8) from the tile's origin.
// quadrant_x / quadrant_y: that pixel's frame coordinates for the tile at (tx0, ty0).
__device__ __forceinline__ int quadrant_x(int tx0, int qq, int lane) { return tx0 + (qq & 1) * 8 + (lane & 7); }
__device__ __forceinline__ int quadrant_y(int ty0, int qq, int lane) { return ty0 + (qq >> 1) * 8 + (lane >> 3); }
// Offset of the lane's q-th pixel from its first: PPL == 4 (a tile): (0,0), (8,0), (0,8), (8,8); PPL == 2 (two quadrants side by side): (0,0), (8,0)
template <int PPL>
__device__ __forceinline__ void quadrant_offset(int q, float& ox, float& oy)
{
    ox = (PPL == 4) ? (float)((q & 1) * 8) : (float)(q * 8);
    oy = (PPL == 4) ? (float)((q >> 1) * 8) : 0.f;
}

// ---- the exponent ----------------------------------------------------------------------------------------------------------------------------
// E = -log2(o G) = d^T conic d - log2 o of a staged record (q0: x, y, -log2 opacity; q1: the conic in exp2 units; stage_for_exp2, common.h) at the lane's
// pixels, d = Gaussian centre - pixel.  The quadratic form is evaluated once, for the pixel (pxf0, pyf0), and shifted to the others (pixel offsets s =
// (8,0), (0,8), (8,8)):  E(d - s) = E(d) - 2 s^T conic d + s^T conic s  -- 14 VALU instructions for four pixels instead of 32 -- and
// E(d - (8,8)) = E2 + (E1 - E0) + 128 b: three instructions instead of four.  l0 = conic d0 is handed back for those who shift it too (quadrant_E_l).
// TILE_Q >= 0 (PPL == 1: a quadrant wave of the hybrid colour kernel, TILE_Q its quadrant at compile time): (pxf0, pyf0) is the lane's pixel in quadrant
// 0 of the TILE and E is formed as a tile wave forms it for quadrant TILE_Q, operation by operation, so that a pixel's colour does not depend, not by one
// bit, on which shape walked its tile.
template <int PPL, int TILE_Q = -1>
__device__ __forceinline__ void quadrant_E(float (&p2q)[PPL], float& dx0, float& dy0, float& lx0, float& ly0, const float4& q0, const float4& q1, float pxf0, float pyf0)
{
    dx0 = q0.x - pxf0; dy0 = q0.y - pyf0;
    lx0 = q1.x * dx0 + q1.y * dy0; ly0 = q1.y * dx0 + q1.z * dy0;
    const float P0 = fmaf(dx0, lx0, fmaf(dy0, ly0, q0.z));
    p2q[0] = P0;
    if constexpr (PPL >= 2) p2q[1] = fmaf(-16.0f, lx0, P0 + 64.0f * q1.x);
    if constexpr (PPL == 4) {
        p2q[2] = fmaf(-16.0f, ly0, P0 + 64.0f * q1.z);
        p2q[3] = fmaf(128.0f, q1.y, p2q[2] + (p2q[1] - P0));
    }
    if constexpr (TILE_Q >= 1 && PPL == 1) {
        const float E1 = fmaf(-16.0f, lx0, P0 + 64.0f * q1.x);
        const float E2 = fmaf(-16.0f, ly0, P0 + 64.0f * q1.z);
        p2q[0] = TILE_Q == 1 ? E1 : (TILE_Q == 2 ? E2 : fmaf(128.0f, q1.y, E2 + (E1 - P0)));
    }
}
template <int PPL, int TILE_Q = -1>
__device__ __forceinline__ void quadrant_E(float (&p2q)[PPL], const float4& q0, const float4& q1, float pxf0, float pyf0)
{
    float dx0, dy0, lx0, ly0;
    quadrant_E<PPL, TILE_Q>(p2q, dx0, dy0, lx0, ly0, q0, q1, pxf0, pyf0);
}
// The backward's form: E as above, d0 for the moments, and under ABS l = conic d of every pixel (only the |.| moments need it): one fma each from l0.
template <int PPL, bool ABS>
__device__ __forceinline__ void quadrant_E_l(float (&p2q)[PPL], float (&lxq)[PPL], float (&lyq)[PPL], float& dx0, float& dy0, const float4& q0, const float4& q1, float pxf0, float pyf0)
{
    quadrant_E<PPL>(p2q, dx0, dy0, lxq[0], lyq[0], q0, q1, pxf0, pyf0);
    const float ca = q1.x, cb = q1.y, cc = q1.z;
    if constexpr (ABS && PPL >= 2) { lxq[1] = fmaf(-8.0f, ca, lxq[0]); lyq[1] = fmaf(-8.0f, cb, lyq[0]); }
    if constexpr (ABS && PPL == 4) {
        lxq[2] = fmaf(-8.0f, cb, lxq[0]); lyq[2] = fmaf(-8.0f, cc, lyq[0]);
        lxq[3] = fmaf(-8.0f, cb, lxq[1]); lyq[3] = fmaf(-8.0f, cc, lyq[1]);
    }
}

// ---- the six geometric sums of a Gaussian over the lane's pixels ---------------------------------------------------------------------------
// v[0..1] = sum Q d, v[4..6] = sum Q d d^T, v[7] = sum Q, with Q_q = o G dL/dalpha of the lane's q-th pixel (0 where it does not blend) and d0 = Gaussian
// centre - first pixel; the other pixels sit at d0 - (8,0), (0,8), (8,8), so with A = Q1 + Q3, B = Q2 + Q3, S0 = Q0 + Q1 + Q2 + Q3
//     sum Q d     = d0 S0 - 8 (A, B)
//     sum Q dx^2  = dx0 (dx0 S0 - 16 A) + 64 A            (likewise y)
//     sum Q dx dy = dy0 Sx - 8 (dx0 B - 8 Q3)
// -- 17 instructions per Gaussian instead of 8 per (Gaussian, quadrant).
template <int PPL, int NV>
__device__ __forceinline__ void d_moments(float (&v)[NV], const float (&Q)[PPL], float dx0, float dy0)
{
    if constexpr (PPL == 4) {
        const float A = Q[1] + Q[3], B = Q[2] + Q[3], S0 = (Q[0] + Q[2]) + A;
        const float t = dx0 * S0, u = dy0 * S0;
        v[0] = fmaf(-8.0f, A, t); v[1] = fmaf(-8.0f, B, u);
        v[4] = fmaf(dx0, fmaf(-16.0f, A, t), 64.0f * A);
        v[6] = fmaf(dy0, fmaf(-16.0f, B, u), 64.0f * B);
        v[5] = fmaf(-8.0f, fmaf(-8.0f, Q[3], dx0 * B), dy0 * v[0]);
        v[7] = S0;
    } else if constexpr (PPL == 2) {       // two quadrants side by side: d1 = d0 - (8, 0)
        const float S0 = Q[0] + Q[1];
        const float t = dx0 * S0;
        v[0] = fmaf(-8.0f, Q[1], t); v[1] = dy0 * S0;
        v[4] = fmaf(dx0, fmaf(-16.0f, Q[1], t), 64.0f * Q[1]);
        v[5] = dy0 * v[0]; v[6] = dy0 * v[1];
        v[7] = S0;
    } else {
        const float qdx = Q[0] * dx0, qdy = Q[0] * dy0;
        v[0] = qdx; v[1] = qdy; v[4] = qdx * dx0; v[5] = qdx * dy0; v[6] = qdy * dy0; v[7] = Q[0];
    }
}
// The same six sums for a near-singular conic on the fast path (render_bwd.hip, "near-singular conics"), in l-space: v[0..1] = sum q l, v[4..6] = sum q l l^T,
// v[7] = sum q, with l = (scaled conic) d formed per pixel -- the first pixel's value shifted like E.  What cancels catastrophically downstream of the
// d-moments (K S K with K = conic) never enters: l is small where the Gaussian is.  ~30 instructions instead of 17, for these Gaussians only (a wave-uniform branch).
// preprocess_bwd.hip undoes the exp2 scale of the conic (EXP2_UNSCALE, squared for the second moments) and takes the second moments as dL/dcov2D.
template <int PPL, int NV>
__device__ __forceinline__ void l_moments(float (&v)[NV], const float (&Q)[PPL], float dx0, float dy0, float ca, float cb, float cc)
{
    const float lx0 = ca * dx0 + cb * dy0, ly0 = cb * dx0 + cc * dy0;
    float sx = 0.f, sy = 0.f, sxx = 0.f, sxy = 0.f, syy = 0.f, s0 = 0.f;
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        float ox, oy;
        quadrant_offset<PPL>(q, ox, oy);
        const float lx = fmaf(-ox, ca, fmaf(-oy, cb, lx0)), ly = fmaf(-ox, cb, fmaf(-oy, cc, ly0));
        const float qx = Q[q] * lx, qy = Q[q] * ly;
        sx += qx; sy += qy; s0 += Q[q];
        sxx = fmaf(qx, lx, sxx); sxy = fmaf(qx, ly, sxy); syy = fmaf(qy, ly, syy);
    }
    v[0] = sx; v[1] = sy; v[4] = sxx; v[5] = sxy; v[6] = syy; v[7] = s0;
}

// ---- what the two backward bodies share ------------------------------------------------------------------------------------------------------
// List entry `entry` as the backward stages it: quads 0 and 1 as the forward stages them (stage_for_exp2, common.h: same numbers, same decisions), the record's
// spare slot ra.w carrying the Gaussian index to the atomic; risky: a near-singular conic (the forward's rare branch).  Returns the record as preprocess wrote
// it (quads 2 and 3 are staged as they are).
__device__ __forceinline__ const float4* bwd_stage_record(const uint32_t* __restrict__ point_list, const float4* __restrict__ rec, uint32_t entry, float4& ra, float4& c1, bool& risky)
{
    const uint32_t id = point_list[entry];
    const float4* r = rec + (size_t)id * 4;
    ra = r[0];
    ra.w = __uint_as_float(id);
    c1 = r[1];
    risky = conic_takes_ref_power(c1.x, c1.y, c1.z);
    stage_for_exp2(ra, c1);
    return r;
}
// Pixels of one quadrant that take part in a chunk: k < n_contrib.  k runs from top - 1 down to top - count and a pixel only ever switches ON (at k = n_contrib - 1),
// so when the masks at both ends agree the returned one holds for the whole chunk; `stable` is cleared when they do not.
__device__ __forceinline__ uint64_t bwd_chunk_mask(uint32_t ncontrib, int top, int count, bool& stable)
{
    const uint64_t m = __builtin_amdgcn_ballot_w64((uint32_t)(top - count) < ncontrib);
    stable = stable && (m == __builtin_amdgcn_ballot_w64((uint32_t)(top - 1) < ncontrib));
    return m;
}
__device__ __forceinline__ float ref_power(float dx, float dy, float a, float b, float c)
{
#pragma clang fp contract(off)
    return -0.5f * (a * dx * dx + c * dy * dy) - b * dx * dy;          // forward.cu:419, backward.cu:644
}
// A pair of a near-singular conic in the reference's arithmetic (IBGS_FLAG_REF_ARITH; render_bwd.hip, "near-singular conics"), up to its blend weight: the lane's
// q-th pixel against the record as preprocess wrote it (g0, g1: unscaled conic, opacity).  okm: the lanes whose pair blends -- E (the decision) from the
// reference's expression, `power > 0` pairs dropped (common.h); zero: nobody's does, and T is left alone.  G = exp(power) at libm accuracy (backward.cu:648;
// 0 where the test fails: alpha = 0 leaves T and S unchanged), T / (1 - alpha) as an IEEE division (:654), w = alpha T.
struct RefPair { uint64_t okm; float dx, dy, G, alpha, om, w; };
template <int PPL>
__device__ __forceinline__ RefPair ref_pair_head(int q, float pxf0, float pyf0, const float4& g0, const float4& g1, float nlo, uint32_t k, uint32_t ncontrib, float& T)
{
    RefPair o{};
    float ox, oy;
    quadrant_offset<PPL>(q, ox, oy);
    o.dx = g0.x - (pxf0 + ox); o.dy = g0.y - (pyf0 + oy);
    const float power = ref_power(o.dx, o.dy, g1.x, g1.y, g1.z);
    const float E = ref_power_E(o.dx, o.dy, g1.x, g1.y, g1.z, nlo);          // what both passes decide on (+inf: `power > 0`)
    o.okm = __builtin_amdgcn_ballot_w64(k < ncontrib) & __builtin_amdgcn_ballot_w64(E <= ALPHA_SKIP_E);
    if (o.okm == 0ull) return o;
    o.G = __builtin_amdgcn_inverse_ballot_w64(o.okm) ? expf(power) : 0.f;
    o.alpha = fminf(0.99f, g0.z * o.G);
    o.om = 1.f - o.alpha;
    T = T / o.om;
    o.w = o.alpha * T;
    return o;
}

}  // namespace ibgs
