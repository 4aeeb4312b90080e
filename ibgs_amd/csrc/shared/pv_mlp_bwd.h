// The backward of the per-view MLP (shared/pv_mlp.h) for one slot of the 32 pixels of a wave, and the sums of its parameter gradients, stated once for the two
// kernels that run it: cagg_bwd_kernel (coloragg.hip: a slot's row is one pixel's) and rzt_features_bwd_kernel (rsztrain.hip: a slot's row is four masked taps,
// blended).  The two are meant to be the same function of a slot's row, bit for bit, and to add the same sums in the same order.  A header of its own, not a
// part of pv_mlp.h: resample.hip is forward only and does not compile this.  ibgs_amd/_build.py lists it under the two units (UNIT_HEADERS) and no other.
//
// WHAT THE BITS REST ON
//   a slot     from the forward's own h1 and h2 (pv_mlp: the same instructions, the same bits): dz2 = g (h2 > 0), in max mode only at the first slot attaining
//              the maximum; dz1 = (w2^T dz2) (h1 > 0) as a k-ordered chain on the matrix cores in pv_mlp.h's map; gx = (w1^T dz1)[0 .. 2]: 16 fmaf per half
//              in register order, then half 0 + half 1.  UNMASKED: what a caller multiplies it by is its own business.
//   parameter gradients   dW2 = sum dz2 (x) h1, db2 = sum dz2, dW1 = sum dz1 (x) x, db1 = sum dz1.  Each wave sums its own 32 pixels of every chunk and slot in
//              a fixed order: dW2 as the matrix cores' f32 fma chain over one chunk's pixels and slots, from there on in f64; the other three in f64 throughout
//              (the products are exact there).  The four waves of a workgroup are added in order and the workgroup's PVB_PARTIAL f64 sums go to its row of
//              `partials`; pv_launch_final adds the workgroups: sixteen strided series per element, then those in order, one rounding to f32.  No float atomics.
//   through LDS   only the weight gradient, whose long dimension is the pixels: each lane stores its pixel's dz2, h1 and dz1 as rows and the wave reads them
//              back a pixel pair per k-step.  h1, h2, dz2, dz1 never leave the registers otherwise.
//
// A KERNEL runs, in this order: pv_stage_bias and pv_bwd_setup once; per chunk of PVB_CHUNK pixels pv_bwd_hmax, then per slot its own loader, pv_mlp and
// pv_bwd_slot, then pv_bwd_end_chunk; pv_bwd_flush once.  The chunk loop, how a slot's row is made and what becomes of gx are the kernel's own.  Every thread
// of the workgroup reaches every call (barriers inside): the chunk and slot bounds are uniform over the workgroup.  lane, wave, c, h: the kernel's own
// lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5 of pv_mlp.h's map, handed on as they are (a helper that derived them again
// left cagg_bwd_kernel's parameters-only form 1 % slower: DESIGN.md section 14).
#pragma once
#include "pv_mlp.h"

namespace ibgs {

constexpr int PV_MEAN = 0, PV_MAX = 1;               // a kernel's MODE: the mean over the slots, or their maximum
constexpr int PVB_T = 256;                           // threads per workgroup
constexpr int PVB_WAVES = PVB_T / 64;
constexpr int PVB_B = 32;                            // pixels per wave
constexpr int PVB_CHUNK = PVB_WAVES * PVB_B;         // pixels per workgroup and step
constexpr int PVB_ROW = 33;                          // row stride of the staged rows: the 32 lanes of a half store one column into 32 banks
constexpr int PVB_PARTIAL = PV_F * PV_INP + PV_F * PV_F + PV_F;          // a workgroup's sums: [dW1 | db1] (32 x 8), dW2 (32 x 32), db2 (32)
constexpr int PVB_MAX_GROUPS = 512;                  // workgroups of a backward (256 CUs x 2 resident): what bounds the arena
constexpr int PVB_WAVE_WORDS = PV_F * PV_F + PV_F * PV_INP + 2 * PV_F;   // a wave's accumulators as the cross-wave sum reads them
constexpr int PVB_FIN_ELEMS = 16, PVB_FIN_SERIES = 16;                   // final kernel: elements per workgroup, strided series per element
static_assert(PVB_B == PV_F && PVB_PARTIAL % PVB_FIN_ELEMS == 0 && PVB_FIN_ELEMS * PVB_FIN_SERIES == PVB_T, "the lane maps below");
static_assert(PVB_WAVES * PVB_WAVE_WORDS * sizeof(double) <= PVB_WAVES * 3 * PVB_B * PVB_ROW * sizeof(float), "the cross-wave sum reuses the staged rows");

// the final pass over `groups` rows of `partials` (PVB_PARTIAL each) into the gradients that are not null; defined in coloragg.hip, whose cagg_final_kernel it launches
void pv_launch_final(hipStream_t st, const double* partials, int groups, float* d_w1, float* d_b1, float* d_w2, float* d_b2);

// the grid of a backward over `pixels` pixels: a workgroup per chunk, capped (a workgroup then walks several chunks)
inline unsigned pv_bwd_groups(size_t pixels)
{
    const size_t chunks = (pixels + PVB_CHUNK - 1) / PVB_CHUNK;
    return (unsigned)(chunks < (size_t)PVB_MAX_GROUPS ? chunks : (size_t)PVB_MAX_GROUPS);
}

__device__ __forceinline__ int pv_levels_of(const int32_t* __restrict__ levels, int S)
{
    const int l = *levels;          // (wave-uniform)
    return l < 0 ? 0 : (l > S ? S : l);
}

// A workgroup's LDS: a kernel declares one of each __shared__ (what its instantiation does not touch takes no room).
// PG: a parameter gradient is asked for (the rows are degenerate otherwise).
template <bool PG>
struct __attribute__((aligned(16))) PvBwdRows {
    float t[PG ? PVB_WAVES : 1][PG ? 3 : 1][PG ? PVB_B : 1][PG ? PVB_ROW : 1];          // per wave: its pixels' dz2, h1, dz1 as rows
    float x[PG ? PVB_WAVES : 1][PG ? PVB_B : 1][PV_INP];          // ... and [x | 1]
};
struct PvBwdW1c { float4 at[2][16]; };          // w1's first three columns at the 16 channels of each half (the same for every pixel: read as a broadcast)

// A lane's registers across the kernel.
struct PvBwdLane {
    float a2t[16];          // the A operand of w2^T dz2: row = this lane's input channel c, k-step kk = the output channels ch(kk, h)
    pv_f32x16 acc2;         // dW2: register r = row ch(r, h) (dz2), column c (h1); the f32 chain of one chunk's pixels and slots, then added to acc2d
    double acc2d[16], acc1[4], accb;          // acc1: [dW1 | db1] at row lane >> 1, columns 4 (lane & 1) .. + 3; accb: db2 of channel c over the pixels 16 h .. 16 h + 15 of the wave
};

// IG: an image gradient is asked for.  Ends with a barrier.
template <bool IG>
__device__ __forceinline__ void pv_bwd_setup(PvBwdW1c& s_w1c, PvBwdLane& a, const float* __restrict__ w1, const float* __restrict__ w2, int c, int h)
{
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) a.a2t[kk] = w2[pv_ch(kk, h) * PV_F + c];
    if (IG && threadIdx.x < 32) {
        const int r = threadIdx.x & 15, hh = threadIdx.x >> 4;
        s_w1c.at[hh][r] = make_float4(w1[pv_ch(r, hh) * PV_IN], w1[pv_ch(r, hh) * PV_IN + 1], w1[pv_ch(r, hh) * PV_IN + 2], 0.0f);
    }
    __syncthreads();
    a.acc1[0] = a.acc1[1] = a.acc1[2] = a.acc1[3] = 0.0;
    a.accb = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a.acc2[r] = 0.0f; a.acc2d[r] = 0.0; }
}

// Max mode: the maximum of h2 over the slots k < L of the lane's pixel, through the caller's own loader `load(k, x)`, the one its slot loop calls.
template <int MODE, class Load>
__device__ __forceinline__ void pv_bwd_hmax(const PvFrag& f, const PvBias& bias, int L, const Load& load, pv_f32x16& hmax, int h)
{
    if (MODE == PV_MAX) {
#pragma unroll
        for (int j = 0; j < 16; ++j) hmax[j] = 0.0f;
        for (int k = 0; k < L; ++k) {
            float x[PV_INP];
            pv_f32x16 h1, h2;
            load(k, x);
            pv_mlp(f, bias, x, h, h1, h2);
#pragma unroll
            for (int j = 0; j < 16; ++j) hmax[j] = fmaxf(hmax[j], h2[j]);
        }
    }
}

// One slot of the lane's pixel.  dz2: h2 on entry.  g: the gradient of the aggregate at the lane's 16 channels (zero for a lane past the frame: it adds
// zeros); taken: max mode, the channels whose maximum an earlier slot attained (0 before the first slot); x: the slot's row; in: the lane's pixel is inside
// the frame.  -> gx when IG.
template <int MODE, bool IG, bool PG>
__device__ __forceinline__ void pv_bwd_slot(PvBwdRows<PG>& s, const PvBwdW1c& s_w1c, PvBwdLane& a, const pv_f32x16& h1, pv_f32x16& dz2, const pv_f32x16& g, const pv_f32x16& hmax,
                                            uint32_t& taken, const float (&x)[PV_INP], bool in, float (&gx)[3], int lane, int wave, int c, int h)
{
    const int r1 = lane >> 1, c0 = (lane & 1) * 4;          // this lane's elements of [dW1 | db1]: row r1 (dz1), columns c0 .. c0 + 3 (x, 1)
    pv_f32x16 dz1;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        bool on = dz2[j] > 0.0f;
        if (MODE == PV_MAX) {
            const bool mine = dz2[j] == hmax[j] && !((taken >> j) & 1u);
            if (mine) taken |= 1u << j;
            on = on && mine;
        }
        dz2[j] = on ? g[j] : 0.0f;
        dz1[j] = 0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) dz1 = pv_mfma(a.a2t[kk], dz2[kk], dz1);
#pragma unroll
    for (int j = 0; j < 16; ++j) dz1[j] = h1[j] > 0.0f ? dz1[j] : 0.0f;
    if constexpr (IG) {
        float dx[3] = {0.0f, 0.0f, 0.0f};          // the lane's 16 channels, then the other half's
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float4 w = s_w1c.at[h][j];
            dx[0] = fmaf(w.x, dz1[j], dx[0]); dx[1] = fmaf(w.y, dz1[j], dx[1]); dx[2] = fmaf(w.z, dz1[j], dx[2]);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) gx[ch] = dx[ch] + __shfl_xor(dx[ch], 32, 64);
    }
    if constexpr (PG) {
        // A wave writes and reads only its own rows (s.t[wave], s.x[wave]): what the data flow needs is that the wave's own stores have landed before its
        // loads of other lanes' rows, and the reverse before the next slot's stores.  __syncthreads() is the construct that promises exactly that for
        // LDS, at the price of lining the four waves up twice per slot; a wave-scope fence in its place was measured, not adopted
        // (docs/EXPERIMENTS.md section 15).
        __syncthreads();          // the rows of the slot before have been read
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            s.t[wave][0][c][pv_ch(j, h)] = dz2[j];
            s.t[wave][1][c][pv_ch(j, h)] = h1[j];
            s.t[wave][2][c][pv_ch(j, h)] = dz1[j];
        }
        *reinterpret_cast<float4*>(&s.x[wave][c][4 * h]) = h ? make_float4(x[4], x[5], x[6], in ? 1.0f : 0.0f) : make_float4(x[0], x[1], x[2], x[3]);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) a.acc2 = pv_mfma(s.t[wave][0][2 * kk + h][c], s.t[wave][1][2 * kk + h][c], a.acc2);          // pixels in order
#pragma unroll 4
        for (int t = 0; t < 16; ++t) a.accb += (double)s.t[wave][0][16 * h + t][c];
#pragma unroll 4
        for (int t = 0; t < PVB_B; ++t) {
            const double d = (double)s.t[wave][2][t][r1];          // (a product of two floats is exact in f64)
            const float4 xe = *reinterpret_cast<const float4*>(&s.x[wave][t][c0]);
            a.acc1[0] = fma(d, (double)xe.x, a.acc1[0]); a.acc1[1] = fma(d, (double)xe.y, a.acc1[1]); a.acc1[2] = fma(d, (double)xe.z, a.acc1[2]); a.acc1[3] = fma(d, (double)xe.w, a.acc1[3]);
        }
    }
}

// the chunk's f32 chain of dW2 joins the f64 sum
__device__ __forceinline__ void pv_bwd_end_chunk(PvBwdLane& a)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) { a.acc2d[r] += (double)a.acc2[r]; a.acc2[r] = 0.0f; }
}

// the four waves' sums, added in order, to partials[blockIdx.x]; the staged rows are reused, so no slot follows
__device__ __forceinline__ void pv_bwd_flush(PvBwdRows<true>& s, const PvBwdLane& a, double* __restrict__ partials, int lane, int wave, int c, int h)
{
    const int r1 = lane >> 1, c0 = (lane & 1) * 4;
    double* const buf = reinterpret_cast<double*>(&s.t[0][0][0][0]);
    double* const mine = buf + wave * PVB_WAVE_WORDS;          // [dW2 (32 x 32) | dW1, db1 (32 x 8) | db2 by half (2 x 32)]
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[pv_ch(r, h) * PV_F + c] = a.acc2d[r];
#pragma unroll
    for (int m = 0; m < 4; ++m) mine[PV_F * PV_F + r1 * PV_INP + c0 + m] = a.acc1[m];
    mine[PV_F * PV_F + PV_F * PV_INP + h * PV_F + c] = a.accb;
    __syncthreads();
    for (int e = threadIdx.x; e < PVB_PARTIAL; e += PVB_T) {          // the waves in order
        double sum = 0.0;
        for (int w = 0; w < PVB_WAVES; ++w) {
            const double* const src = buf + w * PVB_WAVE_WORDS;
            if (e < PV_F * PV_INP) sum += src[PV_F * PV_F + e];
            else if (e < PV_F * PV_INP + PV_F * PV_F) sum += src[e - PV_F * PV_INP];
            else sum += src[PV_F * PV_F + PV_F * PV_INP + (e - PV_F * PV_INP - PV_F * PV_F)] + src[PV_F * PV_F + PV_F * PV_INP + PV_F + (e - PV_F * PV_INP - PV_F * PV_F)];
        }
        partials[(size_t)blockIdx.x * PVB_PARTIAL + e] = sum;
    }
}

}  // namespace ibgs
