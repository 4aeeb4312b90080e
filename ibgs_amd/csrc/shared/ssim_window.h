// The 11-tap window of the structural-similarity map and everything the two units that filter with it -- ssim.hip and geoloss.hip -- run on one 32 x 32 tile:
// the tile's constants, the weights, the row and column passes, and the per-pixel forms.  The one statement of what each of the two used to spell out for
// itself; ibgs_amd/_build.py lists this header under both units (UNIT_HEADERS), and under no other: it sits in a subdirectory of csrc/ so that no other
// unit's profile stamp holds it.  Device code only.
//
// WHAT THE BITS REST ON
//   window     11 taps, sigma 1.5: the reference's float32 1-D weights (exp in double, stored as float32, divided by their float32 sum: SSIMW_W holds the six
//              distinct results; tests/test_ssim_host.py compares them with the reference's), applied separably -- along the row, then down the column --
//              with zero padding of 5 on every side of every plane.
//   passes     ssimw_conv: o[i] = w[0] v[i], then one fmaf per tap, k ascending.  Both users are compiled without -ffp-contract=off, and the chain is written
//              as fmaf: it does not depend on the flag.  The five quantities of a forward row pass are x, y, x x, y y, x y, the products rounded before they
//              are filtered.
//   per pixel  ssimw_pixel and ssimw_combine say `fp contract(off)` themselves: one rounding per operation.
//              u, v = w*x, w*y;  p, q, r = w*x^2, w*y^2, w*xy;  s1 = p - u^2, s2 = q - v^2, s12 = r - uv
//              A = 2uv + C1, B = 2 s12 + C2, C = (u^2 + v^2) + C1, D = (s1 + s2) + C2, m = (A B) / (C D), a correctly rounded division.
//              Swapping x and y swaps u with v and p with q and changes no rounding: m(x, y) == m(y, x) bit for bit.  Where x == y over the window,
//              A == C and B == D bit for bit and m == 1 exactly.
//   derivatives, with t = 2 / (C D):
//              dm/dr = t A;  dm/dp = -m / D, formed as -(dm/dr / 2) (B / D);  dm/du = 2v(B - A)/(CD) - 2u m/C + 2u m/D, formed as t (v (B - A) + (u m) (C - D)).
//              In these forms x == y gives dm/du == 0 and dm/dp == -dm/dr / 2 exactly, and ssimw_combine is exactly zero there.
//
// THE TILE  a workgroup of SSIMW_THREADS = 256 threads per 32 x 32 tile.  The tile with its halo (42 x 42, out-of-plane texels 0) is staged with a row stride
//           of 45 floats.  Row pass: a thread takes 4 adjacent outputs of one staged row -- 14 LDS reads feed 4 x 11 fma per quantity -- and stores each
//           quantity's four results with one 16-byte LDS write (the stride of 45 puts the 32 lanes of a half wave on 32 banks).  Column pass: a thread takes 4
//           outputs of one column, 14 LDS reads per quantity (the lanes of a half wave read 32 adjacent floats).
#pragma once
#include "../common.h"

namespace ibgs {

constexpr int SSIMW_THREADS = 256;                   // threads per workgroup of the tile kernels
constexpr int SSIMW_TH = 32, SSIMW_TW = 32;          // the tile of one workgroup
constexpr int SSIMW_TAPS = 11, SSIMW_HALO = SSIMW_TAPS / 2;
constexpr int SSIMW_SH = SSIMW_TH + 2 * SSIMW_HALO, SSIMW_SW = SSIMW_TW + 2 * SSIMW_HALO;          // the staged tile
constexpr int SSIMW_SS = 45;                         // its row stride in LDS: 1 mod 4, so that four rows x eight 4-float groups land on 32 different banks
constexpr int SSIMW_OPT = 4;                         // outputs per thread along the filter direction
constexpr int SSIMW_NV = SSIMW_OPT + SSIMW_TAPS - 1; // values those outputs read
constexpr int SSIMW_HGROUPS = SSIMW_TW / SSIMW_OPT;
static_assert(SSIMW_TW == 32 && (SSIMW_THREADS / SSIMW_TW) * SSIMW_OPT == SSIMW_TH, "the vertical pass: a thread per column and group of SSIMW_OPT rows");
static_assert(SSIMW_SS >= SSIMW_SW && SSIMW_SS % 4 == 1, "row stride");

// gaussian(11, 1.5) of the reference (loss_utils.py:24-26) in float32: taps 0 .. 5, the window is symmetric
constexpr float SSIMW_W[6] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f};
constexpr float SSIMW_C1 = 0.01f * 0.01f, SSIMW_C2 = 0.03f * 0.03f;

__device__ __forceinline__ constexpr float ssimw_w(int k) { return SSIMW_W[k <= SSIMW_HALO ? k : SSIMW_TAPS - 1 - k]; }

// o[i] = sum_k w[k] v[i + k], k ascending, one fma per tap
__device__ __forceinline__ void ssimw_conv(const float (&v)[SSIMW_NV], float (&o)[SSIMW_OPT])
{
#pragma unroll
    for (int i = 0; i < SSIMW_OPT; ++i) {
        float a = ssimw_w(0) * v[i];
#pragma unroll
        for (int k = 1; k < SSIMW_TAPS; ++k) a = fmaf(ssimw_w(k), v[i + k], a);
        o[i] = a;
    }
}

// blockIdx.x = outer x tiles + tile: outer is the plane (ssim.hip) or the source (geoloss.hip), (ty0, tx0) the tile's first pixel
struct SsimwTile {
    int outer, ty0, tx0;
    __device__ __forceinline__ SsimwTile(int tiles, int tiles_x)
    {
        outer = (int)(blockIdx.x / (unsigned)tiles);
        const int tile = (int)(blockIdx.x - (unsigned)outer * (unsigned)tiles);
        const int ty = tile / tiles_x;
        ty0 = ty * SSIMW_TH;
        tx0 = (tile - ty * tiles_x) * SSIMW_TW;
    }
};

// the row pass over one staged plane that needs nothing but the filter (the backward's three)
__device__ __forceinline__ void ssimw_hpass_row(const float* __restrict__ staged, float* __restrict__ out, int r, int c0)
{
    float v[SSIMW_NV], o[SSIMW_OPT];
#pragma unroll
    for (int j = 0; j < SSIMW_NV; ++j) v[j] = staged[r * SSIMW_SS + c0 + j];
    ssimw_conv(v, o);
    *reinterpret_cast<float4*>(out + r * SSIMW_TW + c0) = make_float4(o[0], o[1], o[2], o[3]);
}

// the forward's row pass: x, y, x x, y y, x y of the staged sx, sy into the five planes of hq
__device__ __forceinline__ void ssimw_hpass_row5(const float* __restrict__ sx, const float* __restrict__ sy, float (&hq)[5][SSIMW_SH * SSIMW_TW], int r, int c0)
{
    float xv[SSIMW_NV], yv[SSIMW_NV], tv[SSIMW_NV], o[SSIMW_OPT];
#pragma unroll
    for (int j = 0; j < SSIMW_NV; ++j) { xv[j] = sx[r * SSIMW_SS + c0 + j]; yv[j] = sy[r * SSIMW_SS + c0 + j]; }
    float* const dst = &hq[0][r * SSIMW_TW + c0];
    ssimw_conv(xv, o);
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    ssimw_conv(yv, o);
    *reinterpret_cast<float4*>(dst + SSIMW_SH * SSIMW_TW) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
    for (int j = 0; j < SSIMW_NV; ++j) tv[j] = xv[j] * xv[j];
    ssimw_conv(tv, o);
    *reinterpret_cast<float4*>(dst + 2 * SSIMW_SH * SSIMW_TW) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
    for (int j = 0; j < SSIMW_NV; ++j) tv[j] = yv[j] * yv[j];
    ssimw_conv(tv, o);
    *reinterpret_cast<float4*>(dst + 3 * SSIMW_SH * SSIMW_TW) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
    for (int j = 0; j < SSIMW_NV; ++j) tv[j] = xv[j] * yv[j];
    ssimw_conv(tv, o);
    *reinterpret_cast<float4*>(dst + 4 * SSIMW_SH * SSIMW_TW) = make_float4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ void ssimw_vpass_col(const float* __restrict__ hq, int r0, int col, float (&o)[SSIMW_OPT])
{
    float v[SSIMW_NV];
#pragma unroll
    for (int j = 0; j < SSIMW_NV; ++j) v[j] = hq[(r0 + j) * SSIMW_TW + col];
    ssimw_conv(v, o);
}

struct SsimwPixel { float m, du, dp, dr; };

// One rounding per operation: see "per pixel" above for what depends on it.
__device__ __forceinline__ SsimwPixel ssimw_pixel(float u, float v, float p, float q, float r, bool derivatives)
{
#pragma clang fp contract(off)
    SsimwPixel o;
    const float uv = u * v, uu = u * u, vv = v * v;
    const float s1 = p - uu, s2 = q - vv, s12 = r - uv;
    const float A = 2.0f * uv + SSIMW_C1, B = 2.0f * s12 + SSIMW_C2, C = (uu + vv) + SSIMW_C1, D = (s1 + s2) + SSIMW_C2;
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

// dL/dx of one pixel from the three filtered derivative planes: ca + 2 x cb + y cc, the three products and two sums rounded one by one
__device__ __forceinline__ float ssimw_combine(float ca, float cb, float cc, float x, float y)
{
#pragma clang fp contract(off)
    const float t1 = (2.0f * x) * cb, t2 = y * cc;
    return ca + (t1 + t2);
}

}  // namespace ibgs
