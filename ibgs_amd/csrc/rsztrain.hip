// The backward of the reduced-resolution colour tail (C ABI: include/ibgs_resample_train.h; Python: ibgs_amd/resample_train.py): the adjoints of resample.hip's
// two kernels, so that the colour network trains at Hr x Wr = int(H s) x int(W s) as the reference trains it under residual_resolution_scale != 1
// (color_aggregation_network.py:200-239, train.py:227-228).  The forwards stay resample.hip's.
//
// CONTRACT (the header states it in full)
//   reduced    per reduced pixel q and slot k < levels: the four masked taps, the blend and both layers recomputed with the forward's instructions (pv_slot and
//              pv_mlp of shared/pv_mlp.h; the tap and value rule of ibgs_resample.h, restated below), then coloragg.hip's backward: dz2 = g (h2 > 0),
//              dz1 = (w2^T dz2) (h1 > 0), gx = (w1^T dz1)[0 .. 2], UNMASKED, to scratch planes at Hr x Wr.
//   parameter gradients   as cagg_bwd_kernel / cagg_final_kernel: per-wave sums in a fixed order (dW2 as the matrix cores' f32 chain over one chunk, from there
//              on in f64; the rest in f64 throughout), one f64 partial per workgroup, a fixed-order final pass, one rounding.  No float atomics.
//   gather     a thread per FULL-resolution pixel: Hr <= H makes y0 strictly increasing, so a row is tap y0 of at most one reduced row and tap y1 of at most
//              one, found in integers; at most 2 x 2 reduced pixels per pixel, weights {u_y u_x, u_y t_x, t_y u_x, t_y t_x}; then the pixel's own mask.
//   upsample   a thread per REDUCED element adds, in ascending (i, j), the full-resolution pixels that have it among their taps: f64, one rounding.
//
// The tap rule, the value rule and the per-slot backward arithmetic are restated here: resample.hip and coloragg.hip keep theirs untouched (their device code and
// profile stamps with them).  tests/test_resample_train_host.py holds rzt_tap and rzt_blend to resample.hip's text.
//
// KERNELS
//   rzt_features_bwd_kernel  256 threads = 4 waves of 32 reduced pixels over a capped grid that walks the reduced frame in chunks of 128; per slot 4 x 7 gathered
//                            loads, 21 blends and 52 MFMA with parameter gradients.
//   rzt_final_kernel         82 workgroups: 16 elements each.
//   rzt_gather_kernel        a thread per full-resolution pixel: at most 4 x (3 levels + 3) loads from the reduced planes, 4 levels feature loads, 3 S + 3 stores.
//   rzt_upsample_bwd_kernel  a thread per reduced element of the three planes.
// What bounds them: DESIGN.md section 19.
#include "common.h"
#include "shared/pv_mlp.h"
#include "../../include/ibgs_resample.h"
#include "../../include/ibgs_resample_train.h"

namespace ibgs {

constexpr int ZT = 256;                              // threads per workgroup
constexpr int ZWAVES = ZT / 64;
constexpr int ZB = 32;                               // reduced pixels per wave
constexpr int ZCHUNK = ZWAVES * ZB;                  // reduced pixels per workgroup and step
constexpr int ZROW = 33;                             // row stride of the staged rows: the 32 lanes of a half store one column into 32 banks
constexpr int RZT_PARTIAL = PV_F * PV_INP + PV_F * PV_F + PV_F;          // a workgroup's sums: [dW1 | db1] (32 x 8), dW2 (32 x 32), db2 (32)
constexpr int RZT_MAX_GROUPS = 512;                  // workgroups of the reduced-resolution kernel (256 CUs x 2 resident): what bounds the arena
constexpr int RZT_WAVE_WORDS = PV_F * PV_F + PV_F * PV_INP + 2 * PV_F;   // a wave's accumulators as the cross-wave sum reads them
constexpr int ZFIN_ELEMS = 16, ZFIN_SERIES = 16;     // final kernel: elements per workgroup, strided series per element
static_assert(PV_F == IBGS_RSZ_FEATURES && ZB == PV_F && RZT_PARTIAL % ZFIN_ELEMS == 0 && ZFIN_ELEMS * ZFIN_SERIES == ZT, "the lane maps below");
static_assert(ZWAVES * RZT_WAVE_WORDS * sizeof(double) <= ZWAVES * 3 * ZB * ZROW * sizeof(float), "the cross-wave sum reuses the staged rows");

// One axis of the coordinate rule: the two taps of output index i of an `out`-long axis made of an `in`-long one, t and 1 - t.  (i (in - 1) < 2^32: both
// sides are at most 65536.)
struct RztTap { uint32_t i0, i1; float t, u; };
__device__ __forceinline__ RztTap rzt_tap(uint32_t i, uint32_t in, uint32_t out)
{
    const uint32_t den = out > 1u ? out - 1u : 1u, num = out > 1u ? i * (in - 1u) : 0u;
    RztTap r;
    r.i0 = num / den;
    r.i1 = min(r.i0 + 1u, in - 1u);
    r.t = (float)(num - r.i0 * den) / (float)den;
    r.u = 1.0f - r.t;
    return r;
}

// the value rule on the taps a, b (row y0) and c, d (row y1)
__device__ __forceinline__ float rzt_blend(float a, float b, float c, float d, const RztTap& ty, const RztTap& tx)
{
    const float top = fmaf(tx.t, b, tx.u * a), bottom = fmaf(tx.t, d, tx.u * c);
    return fmaf(ty.t, bottom, ty.u * top);
}

__device__ __forceinline__ int rzt_levels_of(const int32_t* __restrict__ levels, int S)
{
    const int l = *levels;          // (wave-uniform)
    return l < 0 ? 0 : (l > S ? S : l);
}

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
            const RztTap t = rzt_tap(a, in, out);
            if (t.i0 == y - 1u && t.i1 == y) { o.idx[0] = a; o.wt[0] = t.t; o.on[0] = true; }
        }
    }
    const uint32_t a = rzt_first_at_least(y, in, out);
    if (a < out) {
        const RztTap t = rzt_tap(a, in, out);
        if (t.i0 == y) { o.idx[1] = a; o.wt[1] = t.u; o.on[1] = true; }
    }
    return o;
}

// IG: an image gradient is asked for (gx goes to the scratch planes); PG: a parameter gradient is.  go: 38 planes of Hr x Wr; partials: gridDim.x x RZT_PARTIAL;
// gxs: S x 3 planes of Hr x Wr, written for k < levels.
template <int MODE, bool IG, bool PG>
__global__ void __launch_bounds__(ZT, 2) rzt_features_bwd_kernel(const float* __restrict__ render, const float* __restrict__ warped, const float* __restrict__ feat,
                                                                const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                                const float* __restrict__ b2, const int32_t* __restrict__ levels, int S, uint32_t H, uint32_t W, uint32_t Hr,
                                                                uint32_t Wr, const float* __restrict__ go, float* __restrict__ gxs, double* __restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) float s_t[PG ? ZWAVES : 1][PG ? 3 : 1][PG ? ZB : 1][PG ? ZROW : 1];          // per wave: its pixels' dz2, h1, dz1 as rows
    __shared__ __attribute__((aligned(16))) float s_x[PG ? ZWAVES : 1][PG ? ZB : 1][PV_INP];  // ... and [x | 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const PvFrag f(w1, w2, c, h);
    __shared__ PvBias bias;
    pv_stage_bias(bias, b1, b2);
    float a2t[16];          // the A operand of w2^T dz2: row = this lane's input channel c, k-step kk = the output channels ch(kk, h)
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) a2t[kk] = w2[pv_ch(kk, h) * PV_F + c];
    __shared__ float4 s_w1c[2][16];          // w1's first three columns at the 16 channels of each half (the same for every pixel: read as a broadcast)
    if (IG && threadIdx.x < 32) {
        const int r = threadIdx.x & 15, hh = threadIdx.x >> 4;
        s_w1c[hh][r] = make_float4(w1[pv_ch(r, hh) * PV_IN], w1[pv_ch(r, hh) * PV_IN + 1], w1[pv_ch(r, hh) * PV_IN + 2], 0.0f);
    }
    __syncthreads();
    const int L = rzt_levels_of(levels, S);
    const int r1 = lane >> 1, c0 = (lane & 1) * 4;          // this lane's elements of [dW1 | db1]: row r1 (dz1), columns c0 .. c0 + 3 (x, 1)
    pv_f32x16 acc2;          // dW2: register r = row ch(r, h) (dz2), column c (h1); the f32 chain of one chunk's pixels and slots, then added to acc2d
    double acc2d[16], acc1[4] = {0.0, 0.0, 0.0, 0.0}, accb = 0.0;          // accb: db2 of channel c over the pixels 16 h .. 16 h + 15 of the wave
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc2[r] = 0.0f; acc2d[r] = 0.0; }
    const size_t plane = (size_t)H * W, plane_r = (size_t)Hr * Wr;
    const size_t chunks = (plane_r + ZCHUNK - 1) / ZCHUNK;
    for (size_t ck = blockIdx.x; ck < chunks; ck += gridDim.x) {          // (uniform over the workgroup: the barriers below are reached by every thread)
        const size_t qq = ck * ZCHUNK + (size_t)wave * ZB + c;
        const bool in = qq < plane_r;
        const size_t q = in ? qq : plane_r - 1;          // a lane past the frame recomputes the last pixel under a zero gradient: it adds zeros
        const uint32_t i = (uint32_t)(q / Wr), j = (uint32_t)(q - (size_t)i * Wr);
        const RztTap ty = rzt_tap(i, H, Hr), tx = rzt_tap(j, W, Wr);
        const size_t p[4] = {(size_t)ty.i0 * W + tx.i0, (size_t)ty.i0 * W + tx.i1, (size_t)ty.i1 * W + tx.i0, (size_t)ty.i1 * W + tx.i1};
        float r[4][3];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            r[n][0] = render[p[n]]; r[n][1] = render[plane + p[n]]; r[n][2] = render[2 * plane + p[n]];
        }
        pv_f32x16 g;
#pragma unroll
        for (int m = 0; m < 16; ++m) g[m] = in ? go[(size_t)pv_ch(m, h) * plane_r + q] : 0.0f;
        if (MODE == IBGS_RSZ_MEAN && L > 1) {
            const float n = (float)L;
#pragma unroll
            for (int m = 0; m < 16; ++m) g[m] = g[m] / n;
        }
        pv_f32x16 hmax;
        uint32_t taken = 0u;          // max mode: the channels whose maximum an earlier slot attained
        if (MODE == IBGS_RSZ_MAX) {
#pragma unroll
            for (int m = 0; m < 16; ++m) hmax[m] = 0.0f;
            for (int k = 0; k < L; ++k) {
                float xf[4][PV_INP], x[PV_INP];
#pragma unroll
                for (int n = 0; n < 4; ++n) pv_slot(warped, feat, r[n], plane, p[n], k, xf[n]);
#pragma unroll
                for (int e = 0; e < PV_IN; ++e) x[e] = rzt_blend(xf[0][e], xf[1][e], xf[2][e], xf[3][e], ty, tx);
                x[7] = 0.0f;
                pv_f32x16 h1, h2;
                pv_mlp(f, bias, x, h, h1, h2);
#pragma unroll
                for (int m = 0; m < 16; ++m) hmax[m] = fmaxf(hmax[m], h2[m]);
            }
        }
        for (int k = 0; k < L; ++k) {
            float xf[4][PV_INP], x[PV_INP];
#pragma unroll
            for (int n = 0; n < 4; ++n) pv_slot(warped, feat, r[n], plane, p[n], k, xf[n]);          // (each tap under its own mask)
#pragma unroll
            for (int e = 0; e < PV_IN; ++e) x[e] = rzt_blend(xf[0][e], xf[1][e], xf[2][e], xf[3][e], ty, tx);
            x[7] = 0.0f;          // the eighth input of the first layer's four k-steps
            pv_f32x16 h1, dz2, dz1;
            pv_mlp(f, bias, x, h, h1, dz2);          // dz2 = h2 for now
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                bool on = dz2[m] > 0.0f;
                if (MODE == IBGS_RSZ_MAX) {
                    const bool mine = dz2[m] == hmax[m] && !((taken >> m) & 1u);
                    if (mine) taken |= 1u << m;
                    on = on && mine;
                }
                dz2[m] = on ? g[m] : 0.0f;
                dz1[m] = 0.0f;
            }
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) dz1 = pv_mfma(a2t[kk], dz2[kk], dz1);
#pragma unroll
            for (int m = 0; m < 16; ++m) dz1[m] = h1[m] > 0.0f ? dz1[m] : 0.0f;
            if constexpr (IG) {
                float dx[3] = {0.0f, 0.0f, 0.0f};          // the lane's 16 channels, then the other half's
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const float4 w = s_w1c[h][m];
                    dx[0] = fmaf(w.x, dz1[m], dx[0]); dx[1] = fmaf(w.y, dz1[m], dx[1]); dx[2] = fmaf(w.z, dz1[m], dx[2]);
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float gx = dx[ch] + __shfl_xor(dx[ch], 32, 64);          // (unmasked: the mask is the full-resolution pixel's, applied by the gather)
                    if (in && h == 0) gxs[((size_t)k * 3 + ch) * plane_r + q] = gx;
                }
            }
            if constexpr (PG) {
                // (a wave writes and reads only its own rows; the barriers are cagg_bwd_kernel's: its comment says why they are __syncthreads())
                __syncthreads();          // the rows of the slot before have been read
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    s_t[wave][0][c][pv_ch(m, h)] = dz2[m];
                    s_t[wave][1][c][pv_ch(m, h)] = h1[m];
                    s_t[wave][2][c][pv_ch(m, h)] = dz1[m];
                }
                *reinterpret_cast<float4*>(&s_x[wave][c][4 * h]) = h ? make_float4(x[4], x[5], x[6], in ? 1.0f : 0.0f) : make_float4(x[0], x[1], x[2], x[3]);
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) acc2 = pv_mfma(s_t[wave][0][2 * kk + h][c], s_t[wave][1][2 * kk + h][c], acc2);          // pixels in order
#pragma unroll 4
                for (int t = 0; t < 16; ++t) accb += (double)s_t[wave][0][16 * h + t][c];
#pragma unroll 4
                for (int t = 0; t < ZB; ++t) {
                    const double d = (double)s_t[wave][2][t][r1];          // (a product of two floats is exact in f64)
                    const float4 xe = *reinterpret_cast<const float4*>(&s_x[wave][t][c0]);
                    acc1[0] = fma(d, (double)xe.x, acc1[0]); acc1[1] = fma(d, (double)xe.y, acc1[1]); acc1[2] = fma(d, (double)xe.z, acc1[2]); acc1[3] = fma(d, (double)xe.w, acc1[3]);
                }
            }
        }
        if constexpr (PG) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc2d[r] += (double)acc2[r]; acc2[r] = 0.0f; }
        }
    }
    if constexpr (PG) {
        double* const buf = reinterpret_cast<double*>(&s_t[0][0][0][0]);
        double* const mine = buf + wave * RZT_WAVE_WORDS;          // [dW2 (32 x 32) | dW1, db1 (32 x 8) | db2 by half (2 x 32)]
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[pv_ch(r, h) * PV_F + c] = acc2d[r];
#pragma unroll
        for (int m = 0; m < 4; ++m) mine[PV_F * PV_F + r1 * PV_INP + c0 + m] = acc1[m];
        mine[PV_F * PV_F + PV_F * PV_INP + h * PV_F + c] = accb;
        __syncthreads();
        for (int e = threadIdx.x; e < RZT_PARTIAL; e += ZT) {          // the waves in order
            double sum = 0.0;
            for (int w = 0; w < ZWAVES; ++w) {
                const double* const src = buf + w * RZT_WAVE_WORDS;
                if (e < PV_F * PV_INP) sum += src[PV_F * PV_F + e];
                else if (e < PV_F * PV_INP + PV_F * PV_F) sum += src[e - PV_F * PV_INP];
                else sum += src[PV_F * PV_F + PV_F * PV_INP + (e - PV_F * PV_INP - PV_F * PV_F)] + src[PV_F * PV_F + PV_F * PV_INP + PV_F + (e - PV_F * PV_INP - PV_F * PV_F)];
            }
            partials[(size_t)blockIdx.x * RZT_PARTIAL + e] = sum;
        }
    }
}

// element e of the workgroups' sums: series s adds the workgroups s, s + 16, .. in that order in f64, thread e adds the series in order
__global__ void __launch_bounds__(ZT) rzt_final_kernel(const double* __restrict__ partials, int groups, float* __restrict__ d_w1, float* __restrict__ d_b1,
                                                       float* __restrict__ d_w2, float* __restrict__ d_b2)
{
    __shared__ double s_sum[ZFIN_SERIES][ZFIN_ELEMS];
    const int el = threadIdx.x & (ZFIN_ELEMS - 1), series = threadIdx.x / ZFIN_ELEMS;
    const int e = blockIdx.x * ZFIN_ELEMS + el;
    double a = 0.0;
    for (int g = series; g < groups; g += ZFIN_SERIES) a += partials[(size_t)g * RZT_PARTIAL + e];
    s_sum[series][el] = a;
    __syncthreads();
    if (threadIdx.x < ZFIN_ELEMS) {
        double t = s_sum[0][el];
        for (int k = 1; k < ZFIN_SERIES; ++k) t += s_sum[k][el];
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
    const int L = rzt_levels_of(levels, S);
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
        const RztTap ty = rzt_tap(i, Hr, H);
        if (ty.i0 != a && ty.i1 != a) continue;
        const double wy = (double)(ty.i0 == a ? ty.u : ty.t);          // (y0 = y1 = a on the clamp: t = 0, the weight is u)
        for (uint32_t j = j_lo; j <= j_hi; ++j) {
            const RztTap tx = rzt_tap(j, Wr, W);
            if (tx.i0 != b && tx.i1 != b) continue;
            const double wx = (double)(tx.i0 == b ? tx.u : tx.t);
            const size_t o = (size_t)ch * plane + (size_t)i * W + j;
            const float g = g_out ? (g_pred ? g_out[o] + g_pred[o] : g_out[o]) : g_pred[o];
            acc = fma(wy * wx, (double)g, acc);          // (wy wx is exact in f64)
        }
    }
    d_res[e] = (float)acc;
}

static bool rzt_sides_ok(const char* who, int64_t H, int64_t W, int64_t Hr, int64_t Wr)
{
    if (H < 1 || W < 1 || H > IBGS_RSZ_MAX_SIDE || W > IBGS_RSZ_MAX_SIDE) {
        if (who) set_error("%s: a frame of %lld x %lld is out of range (sides 1 .. %d)", who, (long long)H, (long long)W, IBGS_RSZ_MAX_SIDE);
        return false;
    }
    if (Hr < 1 || Wr < 1 || Hr > IBGS_RSZ_MAX_SIDE || Wr > IBGS_RSZ_MAX_SIDE) {
        if (who) set_error("%s: a reduced frame of %lld x %lld is out of range (sides 1 .. %d)", who, (long long)Hr, (long long)Wr, IBGS_RSZ_MAX_SIDE);
        return false;
    }
    return true;
}

// who == nullptr: silent (the size query)
static bool rzt_features_shape_ok(const char* who, int64_t S, int64_t H, int64_t W, int64_t Hr, int64_t Wr)
{
    if (S < 1 || S > IBGS_RSZ_MAX_SRC) {
        if (who) set_error("%s: %lld sources out of range (1 .. %d)", who, (long long)S, IBGS_RSZ_MAX_SRC);
        return false;
    }
    if (!rzt_sides_ok(who, H, W, Hr, Wr)) return false;
    if (Hr > H || Wr > W) {
        if (who) set_error("%s: a reduced frame of %lld x %lld is larger than the frame of %lld x %lld: training an upscaled network is not supported", who, (long long)Hr,
                           (long long)Wr, (long long)H, (long long)W);
        return false;
    }
    return true;
}

static unsigned rzt_groups(size_t plane_r)
{
    const size_t chunks = (plane_r + ZCHUNK - 1) / ZCHUNK;
    return (unsigned)(chunks < (size_t)RZT_MAX_GROUPS ? chunks : (size_t)RZT_MAX_GROUPS);
}

struct RztScratch {
    double* partials;         // workgroups of the reduced-resolution kernel x RZT_PARTIAL
    float* gx;                // S x 3 planes of Hr x Wr
    static RztScratch carve(char* base, size_t S, size_t plane_r, size_t* total)
    {
        RztScratch d;
        Carver c(base);
        d.partials = c.take<double>((size_t)rzt_groups(plane_r) * RZT_PARTIAL);
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
    if (ig && pg) hipLaunchKernelGGL((rzt_features_bwd_kernel<MODE, true, true>), dim3(groups), dim3(ZT), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, H, W, Hr, Wr, go, gxs, partials);
    else if (pg) hipLaunchKernelGGL((rzt_features_bwd_kernel<MODE, false, true>), dim3(groups), dim3(ZT), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, H, W, Hr, Wr, go, gxs, partials);
    else hipLaunchKernelGGL((rzt_features_bwd_kernel<MODE, true, false>), dim3(groups), dim3(ZT), 0, st, render, warped, feat, w1, b1, w2, b2, levels, S, H, W, Hr, Wr, go, gxs, partials);
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
    const unsigned groups = rzt_groups(plane_r);
    if (mode == IBGS_RSZ_MEAN)
        rzt_launch_bwd<IBGS_RSZ_MEAN>(st, groups, ig, pg, render, warped, cam_feat, w1, b1, w2, b2, levels, (int)S, (uint32_t)H, (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr, grad_out,
                                      ig ? sc.gx : nullptr, pg ? sc.partials : nullptr);
    else
        rzt_launch_bwd<IBGS_RSZ_MAX>(st, groups, ig, pg, render, warped, cam_feat, w1, b1, w2, b2, levels, (int)S, (uint32_t)H, (uint32_t)W, (uint32_t)Hr, (uint32_t)Wr, grad_out,
                                     ig ? sc.gx : nullptr, pg ? sc.partials : nullptr);
    IBGS_HIP(hipGetLastError());
    if (pg) {
        hipLaunchKernelGGL(rzt_final_kernel, dim3(RZT_PARTIAL / ZFIN_ELEMS), dim3(ZT), 0, st, sc.partials, (int)groups, grad_w1, grad_b1, grad_w2, grad_b2);
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
    if (!rzt_sides_ok(who, H, W, Hr, Wr)) return -IBGS_ERR_INVALID;
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
