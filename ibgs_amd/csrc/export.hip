// The frame export (include/ibgs_export.h; the second loop of the reference's render.py, render_set, lines 221-249, and colorize,
// utils/general_utils.py:153-184): 8-bit HWC images of a rendered frame -- save_image's rounding, the cv2 branch, the normal map, the normalised
// residual, the colourised depth -- and the quantisation of metrics.py's protocol.  The contract is equality of every byte with tests/frame_export_ref.py.
//
// ARITHMETIC.  Every float operation below is ONE float32 operation of the reference.  The library's flags allow contraction (no -ffp-contract=off for this
// unit), and __fmul_rn / __fadd_rn are no protection here: this toolchain defines them as a plain product and a plain sum, which the compiler may contract
// like any other.  So the whole translation unit is compiled under `#pragma clang fp contract(off)` (below, at file scope): x * 255 + 0.5 stays a rounded
// product and a rounded sum, and the percentile's A + (B - A) g two rounded operations (contracted, that one changes bits: tests/test_frame_export_host.py
// keeps inputs on which it does; for x * 255 + 0.5 the same test shows that no float32 x exists whose BYTE an fma would change).  Divisions are
// written as `/`: correctly rounded under the library's flags (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt), not v_rcp_f32 and a fix-up.
//
// KERNELS
//   fexp_hist_kernel<PASS>  pass 0, 1, 2 of the radix select over an order-preserving key of the valid values (11 + 11 + 10 bits from the top).  A capped
//                           grid walks the values in quads (one 16-byte load each); each workgroup counts into LDS (pass 0: one histogram; passes 1, 2: one
//                           per DISTINCT prefix among the <= 8 ranks carried) and adds its non-zero bins to the table in the arena with integer atomics.
//                           Pass 0 also takes the integer maximum of the bits of |residual| when a RESIDUAL image rides along.
//   fexp_narrow_kernel<PASS>  one workgroup: block_exclusive_scan over the table, per rank the bin that holds it -> prefix and remaining rank.  Pass 0 forms
//                           the ranks from the valid count; pass 2 forms the percentiles and the status word.
//   fexp_status_kernel      the status word of a frame that has a RESIDUAL image and no percentile.
//   fexp_write_kernel       every image of a frame in one launch (blockIdx.y = image): a lane takes 4 consecutive pixels -- one 16-byte load per plane,
//                           12 contiguous bytes out as three dword stores -- and one lane the last H W mod 4 pixels.  The colour table goes through LDS.
//   fexp_quantize_kernel    ROUND then / 255, float to float.
// What bounds them: DESIGN.md section 20 (profiles/export.txt).
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_export.h"

#pragma clang fp contract(off)

namespace ibgs {

constexpr int FT = 256;                    // threads of every workgroup here
constexpr int FX_BINS0 = 2048, FX_BINS1 = 2048, FX_BINS2 = 1024;          // key bits 31..21, 20..10, 9..0
constexpr int FX_RANKS = 2 * IBGS_FEXP_MAX_Q;
constexpr int FX_HIST_GROUPS = 512;
constexpr int FX_UNROLL = 4;
// the arena, in 32-bit words: [hist0 | hist1 x FX_RANKS | hist2 x FX_RANKS | FX_MAX] are accumulated into and zeroed by every call; the rest is written before it is read
constexpr int FX_HIST1 = FX_BINS0, FX_HIST2 = FX_HIST1 + FX_RANKS * FX_BINS1, FX_WORDS = FX_HIST2 + FX_RANKS * FX_BINS2;
constexpr int FX_MAX = 0, FX_N = 1, FX_RANK = 2, FX_PREFIX = FX_RANK + FX_RANKS, FX_G = FX_PREFIX + FX_RANKS, FX_RESULT = FX_G + IBGS_FEXP_MAX_Q, FX_NWORDS = 32;
constexpr size_t FX_ZEROED = (size_t)FX_WORDS + 1;
static_assert(FX_RESULT + IBGS_FEXP_MAX_Q <= FX_NWORDS && FX_BINS0 % FT == 0 && FX_BINS2 % FT == 0, "the words fit; a whole number of bins per thread of the scan");
static_assert((size_t)FX_RANKS * FX_BINS1 * sizeof(uint32_t) + 64 <= 160 * 1024, "the histograms of passes 1 and 2 live in LDS");

// 16 bytes of floats / 4 mask bytes at an address that is only as aligned as its elements (a plane of H W floats behind another starts anywhere)
typedef float fexp_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t fexp_u32 __attribute__((aligned(1)));

// order-preserving: a < b as floats <=> key(a) < key(b) as unsigned, with -0.0 and +0.0 on one key (numpy compares them equal)
__device__ __forceinline__ uint32_t fexp_key(float v)
{
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fexp_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

struct FexpSel { const float* values; const uint8_t* mask; size_t n; float invalid_val; int use_invalid_val; };
__device__ __forceinline__ bool fexp_valid(const FexpSel& s, float v, uint32_t mask_byte) { return v == v && !(s.use_invalid_val && v == s.invalid_val) && mask_byte == 0u; }

// which of the R ranks count for themselves: rank r borrows the histogram of the first rank with its prefix (lo and hi of a percentile usually share one)
__device__ __forceinline__ void fexp_owners(const uint32_t* words, int R, uint32_t (&pre)[FX_RANKS], int (&owner)[FX_RANKS])
{
#pragma unroll
    for (int r = 0; r < FX_RANKS; ++r) {
        pre[r] = r < R ? words[FX_PREFIX + r] : 0u;
        owner[r] = r;
#pragma unroll
        for (int o = r - 1; o >= 0; --o)
            if (pre[o] == pre[r]) owner[r] = o;
    }
}

template <int PASS>
__global__ void __launch_bounds__(FT) fexp_hist_kernel(const FexpSel s, uint32_t* __restrict__ tab, int R, const float* __restrict__ residual, size_t rn)
{
    constexpr int BINS = PASS == 2 ? FX_BINS2 : FX_BINS0;
    constexpr int ROWS = PASS == 0 ? 1 : FX_RANKS;
    constexpr int TOP = PASS == 1 ? 21 : 10;          // the bits above this pass's digit (passes 1, 2)
    constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
    __shared__ uint32_t s_h[ROWS * BINS];
    __shared__ uint32_t s_max;
    uint32_t* hist = tab + (PASS == 0 ? 0 : PASS == 1 ? FX_HIST1 : FX_HIST2);
    const int rows = PASS == 0 ? 1 : R;
    uint32_t pre[FX_RANKS];
    int owner[FX_RANKS];
    if (PASS > 0) fexp_owners(tab + FX_WORDS, R, pre, owner);
    for (int i = threadIdx.x; i < rows * BINS; i += FT) s_h[i] = 0u;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    auto count = [&](float v, uint32_t mask_byte) {
        if (!fexp_valid(s, v, mask_byte)) return;
        const uint32_t key = fexp_key(v);
        if (PASS == 0) {
            atomicAdd(&s_h[key >> SHIFT], 1u);
        } else {
            const uint32_t top = key >> TOP, digit = (key >> SHIFT) & (BINS - 1);
#pragma unroll
            for (int r = 0; r < FX_RANKS; ++r)
                if (r < R && owner[r] == r && top == pre[r]) atomicAdd(&s_h[r * BINS + digit], 1u);
        }
    };
    const size_t stride = (size_t)gridDim.x * FT, first = (size_t)blockIdx.x * FT + threadIdx.x;
    const size_t quads = s.n / 4;
    // FX_UNROLL quads per thread and step, every load issued before the first is counted: with a capped grid a thread walks only a few quads, and one
    // load latency per quad would be most of the kernel's time
    for (size_t q0 = first; q0 < quads; q0 += FX_UNROLL * stride) {
        fexp_f4 v[FX_UNROLL];
        uint32_t m[FX_UNROLL];
#pragma unroll
        for (int u = 0; u < FX_UNROLL; ++u) {
            const size_t q = q0 + u * stride;
            if (q < quads) {
                v[u] = *reinterpret_cast<const fexp_f4*>(s.values + 4 * q);
                m[u] = s.mask ? *reinterpret_cast<const fexp_u32*>(s.mask + 4 * q) : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < FX_UNROLL; ++u) {
            if (q0 + u * stride >= quads) break;
            count(v[u].x, m[u] & 0xFFu); count(v[u].y, (m[u] >> 8) & 0xFFu); count(v[u].z, (m[u] >> 16) & 0xFFu); count(v[u].w, m[u] >> 24);
        }
    }
    if (first == 0)
        for (size_t e = 4 * quads; e < s.n; ++e) count(s.values[e], s.mask ? s.mask[e] : 0u);
    if (PASS == 0 && residual) {          // the bits of |r| order as |r| does: an integer maximum, the same on every run
        uint32_t m = 0u;
        const size_t rquads = rn / 4;
        for (size_t q = first; q < rquads; q += stride) {
            const fexp_f4 v = *reinterpret_cast<const fexp_f4*>(residual + 4 * q);
            m = max(max(m, __float_as_uint(v.x) & 0x7FFFFFFFu), __float_as_uint(v.y) & 0x7FFFFFFFu);
            m = max(max(m, __float_as_uint(v.z) & 0x7FFFFFFFu), __float_as_uint(v.w) & 0x7FFFFFFFu);
        }
        if (first == 0)
            for (size_t e = 4 * rquads; e < rn; ++e) m = max(m, __float_as_uint(residual[e]) & 0x7FFFFFFFu);
        m = wave_reduce(m, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&s_max, m);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * BINS; i += FT) {
        const uint32_t c = s_h[i];
        if (c) atomicAdd(&hist[i], c);
    }
    if (PASS == 0 && residual && threadIdx.x == 0 && s_max) atomicMax(&tab[FX_WORDS + FX_MAX], s_max);
}

struct FexpQ { int nq; float q32[IBGS_FEXP_MAX_Q]; };

// the bin of c[0 .. PER) (the thread's own, `before` values ahead of them) that holds rank rk: -> true, *bin, *ahead = the values ahead of that bin
template <int PER>
__device__ __forceinline__ bool fexp_find(const uint32_t (&c)[PER], uint32_t before, uint32_t sum, uint32_t rk, int* bin, uint32_t* ahead)
{
    if (rk < before || rk - before >= sum) return false;
    uint32_t cum = before;
    int k = 0;
#pragma unroll
    for (int j = 0; j < PER - 1; ++j)
        if (k == j && rk - cum >= c[j]) { cum += c[j]; k = j + 1; }
    *bin = (int)threadIdx.x * PER + k;
    *ahead = cum;
    return true;
}

template <int PASS>
__global__ void __launch_bounds__(FT) fexp_narrow_kernel(uint32_t* tab, const FexpQ q, float* out, int32_t* status, int has_residual)          // (out may lie in tab: the frame's)
{
    constexpr int BINS = PASS == 2 ? FX_BINS2 : FX_BINS0;
    constexpr int PER = BINS / FT;
    constexpr int DIGIT_BITS = PASS == 2 ? 10 : 11;
    __shared__ uint32_t s_row[FT / 64];
    __shared__ uint32_t s_key[FX_RANKS];
    uint32_t* words = tab + FX_WORDS;
    const int R = 2 * q.nq;
    uint32_t c[PER];
    if (PASS == 0) {
        uint32_t sum = 0u, n = 0u;
#pragma unroll
        for (int k = 0; k < PER; ++k) { c[k] = tab[threadIdx.x * PER + k]; sum += c[k]; }
        const uint32_t before = block_exclusive_scan<FT>(sum, &n, s_row);
#pragma unroll
        for (int k = 0; k < IBGS_FEXP_MAX_Q; ++k) {
            if (k >= q.nq) break;
            uint32_t rk[2] = {0u, 0u};
            float g = 0.0f;
            if (n) {
                const float vi = (float)(n - 1u) * q.q32[k];          // n <= 2^24: n - 1 is exact
                const float lo = floorf(vi);
                g = vi - lo;
                rk[0] = min((uint32_t)lo, n - 1u);
                rk[1] = min(rk[0] + 1u, n - 1u);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int bin;
                uint32_t ahead;
                if (fexp_find<PER>(c, before, sum, rk[j], &bin, &ahead)) { words[FX_PREFIX + 2 * k + j] = (uint32_t)bin; words[FX_RANK + 2 * k + j] = rk[j] - ahead; }
            }
            if (threadIdx.x == 0) words[FX_G + k] = __float_as_uint(g);
        }
        if (threadIdx.x == 0) words[FX_N] = n;
        if (n == 0u && threadIdx.x < FX_RANKS) { words[FX_PREFIX + threadIdx.x] = 0u; words[FX_RANK + threadIdx.x] = 0u; }
        return;
    }
    const uint32_t* hist = tab + (PASS == 1 ? FX_HIST1 : FX_HIST2);
    uint32_t pre[FX_RANKS], rk[FX_RANKS];
    int owner[FX_RANKS];
    fexp_owners(words, R, pre, owner);
#pragma unroll
    for (int r = 0; r < FX_RANKS; ++r) rk[r] = r < R ? words[FX_RANK + r] : 0u;
    if (threadIdx.x < FX_RANKS) s_key[threadIdx.x] = 0u;
    __syncthreads();          // every thread holds the prefixes and ranks before one of them is replaced
#pragma unroll
    for (int r = 0; r < FX_RANKS; ++r) {
        if (r >= R) break;
        uint32_t sum = 0u, total = 0u;
#pragma unroll
        for (int k = 0; k < PER; ++k) { c[k] = hist[owner[r] * BINS + threadIdx.x * PER + k]; sum += c[k]; }
        const uint32_t before = block_exclusive_scan<FT>(sum, &total, s_row);
        int bin;
        uint32_t ahead;
        if (fexp_find<PER>(c, before, sum, rk[r], &bin, &ahead)) {
            const uint32_t p = (pre[r] << DIGIT_BITS) | (uint32_t)bin;
            words[FX_PREFIX + r] = p;
            words[FX_RANK + r] = rk[r] - ahead;
            if (PASS == 2) s_key[r] = p;
        }
        __syncthreads();          // s_row is free again; s_key[r] is written
    }
    if (PASS == 2 && threadIdx.x == 0) {
        const uint32_t n = words[FX_N];
        for (int k = 0; k < q.nq; ++k) {
            const float A = fexp_unkey(s_key[2 * k]), B = fexp_unkey(s_key[2 * k + 1]), g = __uint_as_float(words[FX_G + k]);
            const float d = B - A;
            const float r = g >= 0.5f ? B - d * (1.0f - g) : A + d * g;          // numpy's _lerp
            const float res = n ? r : 0.0f;
            out[k] = res;
            words[FX_RESULT + k] = __float_as_uint(res);
        }
        *status = (has_residual && words[FX_MAX] == 0u ? IBGS_FEXP_ZERO_RESIDUAL : 0) | (n == 0u ? IBGS_FEXP_NO_VALID : 0);
    }
}

__global__ void fexp_status_kernel(const uint32_t* __restrict__ tab, int32_t* __restrict__ status)
{
    if (threadIdx.x == 0) *status = tab[FX_WORDS + FX_MAX] == 0u ? IBGS_FEXP_ZERO_RESIDUAL : 0;
}

// ---- the rules, one float32 operation per line of the reference ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fexp_byte(float t) { return (uint32_t)fminf(fmaxf(t, 0.0f), 255.0f); }          // clamp (a NaN: 0), truncate
__device__ __forceinline__ uint32_t fexp_round(float x)
{
    float t = x * 255.0f;          // __fmul_rn: a rounded product ...
    t = t + 0.5f;                  // __fadd_rn: ... and a rounded sum, never fma(x, 255, 0.5) (the pragma at the top of the file)
    return fexp_byte(t);
}
__device__ __forceinline__ uint32_t fexp_truncate(float x) { return fexp_byte(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f); }
__device__ __forceinline__ uint32_t fexp_normal(float x)
{
    float t = (x + 1.0f) / 2.0f;
    t = t * 255.0f;
    return fexp_byte(t);
}
__device__ __forceinline__ uint32_t fexp_residual(float x, float m) { return m == 0.0f ? 0u : fexp_round(fabsf(x) / m); }
__device__ __forceinline__ uint32_t fexp_plain(int mode, float x, float m)
{
    return mode == IBGS_FEXP_ROUND ? fexp_round(x) : mode == IBGS_FEXP_TRUNCATE ? fexp_truncate(x) : mode == IBGS_FEXP_NORMAL ? fexp_normal(x) : fexp_residual(x, m);
}

struct FexpImage { const float* src; uint8_t* dst; int mode, channels, bgr, reserved; };
struct FexpWrite {
    FexpImage img[IBGS_FEXP_MAX_IMAGES];
    const uint8_t* lut; const uint8_t* mask; const uint32_t* words;
    size_t plane;
    int use_invalid_val; float invalid_val;
    int have_vmin, have_vmax; float vmin, vmax;
    uint32_t background;          // r | g << 8 | b << 16
};

// -> r | g << 8 | b << 16 of one COLORIZE pixel
__device__ __forceinline__ uint32_t fexp_colour(const FexpWrite& a, const uint32_t* s_lut, float v, uint32_t mask_byte, float vmin, float vmax)
{
    if (!(v == v) || (a.use_invalid_val && v == a.invalid_val) || mask_byte != 0u) return a.background;
    const float x = vmin != vmax ? (v - vmin) / (vmax - vmin) : v * 0.0f;
    const float xa = x * 256.0f;
    if (!(xa == xa)) return 0u;
    const int entry = xa == 256.0f ? 255 : xa < 0.0f ? 0 : xa >= 256.0f ? 255 : (int)xa;
    return s_lut[entry];
}

__global__ void __launch_bounds__(FT) fexp_write_kernel(const FexpWrite a)
{
    __shared__ uint32_t s_lut[256];
    const FexpImage im = a.img[blockIdx.y];
    const size_t plane = a.plane, quads = plane / 4;
    const size_t q = (size_t)blockIdx.x * FT + threadIdx.x;
    uint8_t* const dst = im.dst;
    if (im.mode == IBGS_FEXP_COLORIZE) {          // (the mode is the workgroup's: every thread takes the same side)
        static_assert(FT == 256, "one entry of the table per thread");
        s_lut[threadIdx.x] = (uint32_t)a.lut[3 * threadIdx.x] | ((uint32_t)a.lut[3 * threadIdx.x + 1] << 8) | ((uint32_t)a.lut[3 * threadIdx.x + 2] << 16);
        __syncthreads();
        const float vmin = a.have_vmin ? a.vmin : __uint_as_float(a.words[FX_RESULT]), vmax = a.have_vmax ? a.vmax : __uint_as_float(a.words[FX_RESULT + 1]);
        if (q < quads) {
            const fexp_f4 v = *reinterpret_cast<const fexp_f4*>(im.src + 4 * q);
            const uint32_t m = a.mask ? *reinterpret_cast<const fexp_u32*>(a.mask + 4 * q) : 0u;
            const uint32_t p0 = fexp_colour(a, s_lut, v.x, m & 0xFFu, vmin, vmax), p1 = fexp_colour(a, s_lut, v.y, (m >> 8) & 0xFFu, vmin, vmax);
            const uint32_t p2 = fexp_colour(a, s_lut, v.z, (m >> 16) & 0xFFu, vmin, vmax), p3 = fexp_colour(a, s_lut, v.w, m >> 24, vmin, vmax);
            uint32_t* o = reinterpret_cast<uint32_t*>(dst + 12 * q);
            o[0] = p0 | (p1 << 24);
            o[1] = (p1 >> 8) | (p2 << 16);
            o[2] = (p2 >> 16) | (p3 << 8);
        } else if (q == quads) {
            for (size_t e = 4 * quads; e < plane; ++e) {
                const uint32_t p = fexp_colour(a, s_lut, im.src[e], a.mask ? a.mask[e] : 0u, vmin, vmax);
                dst[3 * e] = (uint8_t)p; dst[3 * e + 1] = (uint8_t)(p >> 8); dst[3 * e + 2] = (uint8_t)(p >> 16);
            }
        }
        return;
    }
    const float m = im.mode == IBGS_FEXP_RESIDUAL ? __uint_as_float(a.words[FX_MAX]) : 0.0f;
    if (im.channels == 1) {
        if (q < quads) {
            const fexp_f4 v = *reinterpret_cast<const fexp_f4*>(im.src + 4 * q);
            *reinterpret_cast<uint32_t*>(dst + 4 * q) = fexp_plain(im.mode, v.x, m) | (fexp_plain(im.mode, v.y, m) << 8) | (fexp_plain(im.mode, v.z, m) << 16) | (fexp_plain(im.mode, v.w, m) << 24);
        } else if (q == quads) {
            for (size_t e = 4 * quads; e < plane; ++e) dst[e] = (uint8_t)fexp_plain(im.mode, im.src[e], m);
        }
        return;
    }
    const float* const c0 = im.src + (im.bgr ? 2 * plane : 0), * const c1 = im.src + plane, * const c2 = im.src + (im.bgr ? 0 : 2 * plane);
    if (q < quads) {
        const fexp_f4 x = *reinterpret_cast<const fexp_f4*>(c0 + 4 * q), y = *reinterpret_cast<const fexp_f4*>(c1 + 4 * q), z = *reinterpret_cast<const fexp_f4*>(c2 + 4 * q);
        const int mode = im.mode;
        uint32_t* o = reinterpret_cast<uint32_t*>(dst + 12 * q);
        o[0] = fexp_plain(mode, x.x, m) | (fexp_plain(mode, y.x, m) << 8) | (fexp_plain(mode, z.x, m) << 16) | (fexp_plain(mode, x.y, m) << 24);
        o[1] = fexp_plain(mode, y.y, m) | (fexp_plain(mode, z.y, m) << 8) | (fexp_plain(mode, x.z, m) << 16) | (fexp_plain(mode, y.z, m) << 24);
        o[2] = fexp_plain(mode, z.z, m) | (fexp_plain(mode, x.w, m) << 8) | (fexp_plain(mode, y.w, m) << 16) | (fexp_plain(mode, z.w, m) << 24);
    } else if (q == quads) {
        for (size_t e = 4 * quads; e < plane; ++e) {
            dst[3 * e] = (uint8_t)fexp_plain(im.mode, c0[e], m);
            dst[3 * e + 1] = (uint8_t)fexp_plain(im.mode, c1[e], m);
            dst[3 * e + 2] = (uint8_t)fexp_plain(im.mode, c2[e], m);
        }
    }
}

__global__ void __launch_bounds__(FT) fexp_quantize_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n)
{
    const size_t quads = n / 4, q = (size_t)blockIdx.x * FT + threadIdx.x;
    if (q < quads) {
        const fexp_f4 v = *reinterpret_cast<const fexp_f4*>(in + 4 * q);
        fexp_f4 r;
        r.x = (float)fexp_round(v.x) / 255.0f; r.y = (float)fexp_round(v.y) / 255.0f; r.z = (float)fexp_round(v.z) / 255.0f; r.w = (float)fexp_round(v.w) / 255.0f;
        *reinterpret_cast<fexp_f4*>(out + 4 * q) = r;
    } else if (q == quads) {
        for (size_t e = 4 * quads; e < n; ++e) out[e] = (float)fexp_round(in[e]) / 255.0f;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
static size_t fexp_arena_bytes() { return ((size_t)FX_WORDS + FX_NWORDS) * sizeof(uint32_t) + 128; }

static bool fexp_shape_ok(const char* who, int64_t H, int64_t W)
{
    if (H < 1 || W < 1 || H > IBGS_FEXP_MAX_SIDE || W > IBGS_FEXP_MAX_SIDE || H * W > (int64_t)IBGS_FEXP_MAX_PIXELS) {
        if (who) set_error("%s: a frame of %lld x %lld is out of range (sides 1 .. %d, %d pixels at most)", who, (long long)H, (long long)W, IBGS_FEXP_MAX_SIDE, IBGS_FEXP_MAX_PIXELS);
        return false;
    }
    return true;
}

static unsigned fexp_hist_groups(size_t n, size_t rn)
{
    const size_t quads = (n > rn ? n : rn) / 4 + 1, g = (quads + FT - 1) / FT;
    return (unsigned)(g < (size_t)FX_HIST_GROUPS ? g : (size_t)FX_HIST_GROUPS);
}

// the chain in front of the writer: zero, pass 0 (with the residual's maximum), and with nq > 0 the scans and passes 1, 2.  tab: the arena's words.
static int32_t fexp_stats(hipStream_t st, const FexpSel& sel, const FexpQ& q, const float* residual, size_t rn, uint32_t* tab, float* out, int32_t* status)
{
    IBGS_HIP(hipMemsetAsync(tab, 0, FX_ZEROED * sizeof(uint32_t), st));
    FexpSel s = sel;
    if (q.nq == 0) s.n = 0;
    const unsigned groups = fexp_hist_groups(s.n, rn);
    const int R = 2 * q.nq;
    hipLaunchKernelGGL((fexp_hist_kernel<0>), dim3(groups), dim3(FT), 0, st, s, tab, R, residual, rn);
    IBGS_HIP(hipGetLastError());
    if (q.nq == 0) {
        hipLaunchKernelGGL(fexp_status_kernel, dim3(1), dim3(64), 0, st, tab, status);
        IBGS_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL((fexp_narrow_kernel<0>), dim3(1), dim3(FT), 0, st, tab, q, out, status, residual != nullptr);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL((fexp_hist_kernel<1>), dim3(groups), dim3(FT), 0, st, s, tab, R, (const float*)nullptr, (size_t)0);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL((fexp_narrow_kernel<1>), dim3(1), dim3(FT), 0, st, tab, q, out, status, residual != nullptr);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL((fexp_hist_kernel<2>), dim3(groups), dim3(FT), 0, st, s, tab, R, (const float*)nullptr, (size_t)0);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL((fexp_narrow_kernel<2>), dim3(1), dim3(FT), 0, st, tab, q, out, status, residual != nullptr);
    IBGS_HIP(hipGetLastError());
    return 0;
}

static bool fexp_q_ok(const char* who, int nq, const float* q32)
{
    for (int k = 0; k < nq; ++k)
        if (!(q32[k] >= 0.0f && q32[k] <= 1.0f)) { set_error("%s: q32[%d] = %g is outside [0, 1]", who, k, (double)q32[k]); return false; }
    return true;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_fexp_sizeof_frame(void) { return sizeof(ibgs_fexp_frame); }

size_t ibgs_required_export(int64_t H, int64_t W)
{
    if (!fexp_shape_ok(nullptr, H, W)) return 0;
    return fexp_arena_bytes();
}

int32_t ibgs_fexp_frame_u8(void* stream, const ibgs_fexp_frame* f)
{
    const char* who = "fexp_frame_u8";
    if (!f) { set_error("%s: null frame", who); return -IBGS_ERR_INVALID; }
    if (!fexp_shape_ok(who, f->H, f->W)) return -IBGS_ERR_INVALID;
    if (f->n_images < 1 || f->n_images > IBGS_FEXP_MAX_IMAGES) { set_error("%s: %d images (1 .. %d)", who, f->n_images, IBGS_FEXP_MAX_IMAGES); return -IBGS_ERR_INVALID; }
    if (!f->status) { set_error("%s: null status", who); return -IBGS_ERR_INVALID; }
    const size_t plane = (size_t)f->H * (size_t)f->W;
    const ibgs_fexp_image* residual = nullptr;
    const ibgs_fexp_image* colorize = nullptr;
    FexpWrite w = {};
    for (int i = 0; i < f->n_images; ++i) {
        const ibgs_fexp_image& im = f->images[i];
        if (!im.src || !im.dst) { set_error("%s: image %d: null %s", who, i, im.src ? "dst" : "src"); return -IBGS_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(im.dst) & 3) { set_error("%s: image %d: dst is not 4-byte aligned", who, i); return -IBGS_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(im.src) & 3) { set_error("%s: image %d: src is not 4-byte aligned", who, i); return -IBGS_ERR_INVALID; }
        if (im.mode < IBGS_FEXP_ROUND || im.mode > IBGS_FEXP_COLORIZE) { set_error("%s: image %d: mode %d is none of IBGS_FEXP_ROUND .. IBGS_FEXP_COLORIZE", who, i, im.mode); return -IBGS_ERR_INVALID; }
        if (im.channels != 1 && im.channels != 3) { set_error("%s: image %d: %d channels (1 or 3)", who, i, im.channels); return -IBGS_ERR_INVALID; }
        if (im.mode == IBGS_FEXP_COLORIZE && im.channels != 1) { set_error("%s: image %d: COLORIZE reads one plane, not %d", who, i, im.channels); return -IBGS_ERR_INVALID; }
        if (im.bgr && im.channels != 3) { set_error("%s: image %d: bgr needs 3 channels", who, i); return -IBGS_ERR_INVALID; }
        if (im.mode == IBGS_FEXP_RESIDUAL) {
            if (residual) { set_error("%s: more than one RESIDUAL image", who); return -IBGS_ERR_INVALID; }
            residual = &im;
        }
        if (im.mode == IBGS_FEXP_COLORIZE) {
            if (colorize) { set_error("%s: more than one COLORIZE image", who); return -IBGS_ERR_INVALID; }
            colorize = &im;
        }
        w.img[i] = FexpImage{im.src, im.dst, im.mode, im.channels, im.bgr ? 1 : 0, 0};
    }
    if (colorize && !f->lut) { set_error("%s: null lut: a COLORIZE image needs the 256 x 3 table", who); return -IBGS_ERR_INVALID; }
    const bool select = colorize && !(f->have_vmin && f->have_vmax);
    FexpQ q = {};
    if (select) {
        if (plane > (size_t)IBGS_FEXP_MAX_SELECT) { set_error("%s: percentiles of %zu values (limit: %d, so that n - 1 is exact in float32)", who, plane, IBGS_FEXP_MAX_SELECT); return -IBGS_ERR_INVALID; }
        q.nq = 2; q.q32[0] = f->q32[0]; q.q32[1] = f->q32[1];
        if (!fexp_q_ok(who, 2, q.q32)) return -IBGS_ERR_INVALID;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint32_t* tab = nullptr;
    if (select || residual) {
        Carver c(static_cast<char*>(f->scratch));
        tab = c.take<uint32_t>((size_t)FX_WORDS + FX_NWORDS);
        if (!arena_ok(who, "scratch", f->scratch, f->scratch_bytes, c.cur - reinterpret_cast<uintptr_t>(f->scratch) + 128)) return -IBGS_ERR_INVALID;
        FexpSel sel = {colorize ? colorize->src : nullptr, f->invalid_mask, colorize ? plane : 0, f->invalid_val, f->use_invalid_val ? 1 : 0};
        const int32_t rc = fexp_stats(st, sel, q, residual ? residual->src : nullptr, residual ? plane * (size_t)residual->channels : 0, tab, reinterpret_cast<float*>(tab + FX_WORDS + FX_RESULT), f->status);
        if (rc < 0) return rc;
    } else {
        IBGS_HIP(hipMemsetAsync(f->status, 0, sizeof(int32_t), st));
    }
    w.lut = f->lut; w.mask = f->invalid_mask; w.words = tab ? tab + FX_WORDS : nullptr;
    w.plane = plane;
    w.use_invalid_val = f->use_invalid_val ? 1 : 0; w.invalid_val = f->invalid_val;
    w.have_vmin = select ? (f->have_vmin ? 1 : 0) : 1; w.have_vmax = select ? (f->have_vmax ? 1 : 0) : 1;
    w.vmin = f->vmin; w.vmax = f->vmax;
    w.background = (uint32_t)f->background[0] | ((uint32_t)f->background[1] << 8) | ((uint32_t)f->background[2] << 16);
    hipLaunchKernelGGL(fexp_write_kernel, dim3(grid_for(plane / 4 + 1, FT), (unsigned)f->n_images), dim3(FT), 0, st, w);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_fexp_percentile(void* stream, int64_t n, const float* values, const uint8_t* invalid_mask, int32_t use_invalid_val, float invalid_val,
                             int32_t nq, const float* q32, float* out, int32_t* status, void* scratch, size_t scratch_bytes)
{
    const char* who = "fexp_percentile";
    if (n < 0 || n > (int64_t)IBGS_FEXP_MAX_SELECT) { set_error("%s: %lld values (limit: %d, so that n - 1 is exact in float32)", who, (long long)n, IBGS_FEXP_MAX_SELECT); return -IBGS_ERR_INVALID; }
    if (nq < 1 || nq > IBGS_FEXP_MAX_Q) { set_error("%s: %d percentiles (1 .. %d)", who, nq, IBGS_FEXP_MAX_Q); return -IBGS_ERR_INVALID; }
    if (!q32) { set_error("%s: null q32", who); return -IBGS_ERR_INVALID; }
    if (n > 0 && !values) { set_error("%s: null values", who); return -IBGS_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(values) & 3) { set_error("%s: values is not 4-byte aligned", who); return -IBGS_ERR_INVALID; }
    if (!out || !status) { set_error("%s: null outputs: out and status are required", who); return -IBGS_ERR_INVALID; }
    FexpQ q = {};
    q.nq = nq;
    for (int k = 0; k < nq; ++k) q.q32[k] = q32[k];
    if (!fexp_q_ok(who, nq, q.q32)) return -IBGS_ERR_INVALID;
    Carver c(static_cast<char*>(scratch));
    uint32_t* tab = c.take<uint32_t>((size_t)FX_WORDS + FX_NWORDS);
    if (!arena_ok(who, "scratch", scratch, scratch_bytes, c.cur - reinterpret_cast<uintptr_t>(scratch) + 128)) return -IBGS_ERR_INVALID;
    const FexpSel sel = {values, invalid_mask, (size_t)n, invalid_val, use_invalid_val ? 1 : 0};
    return fexp_stats(reinterpret_cast<hipStream_t>(stream), sel, q, nullptr, 0, tab, out, status);
}

int32_t ibgs_fexp_quantize(void* stream, int64_t n, const float* in, float* out)
{
    const char* who = "fexp_quantize";
    if (n < 1 || n > (int64_t)1 << 40) { set_error("%s: %lld values", who, (long long)n); return -IBGS_ERR_INVALID; }
    if (!in || !out) { set_error("%s: null %s", who, in ? "out" : "in"); return -IBGS_ERR_INVALID; }
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3) { set_error("%s: in or out is not 4-byte aligned", who); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(fexp_quantize_kernel, dim3(grid_for((size_t)n / 4 + 1, FT)), dim3(FT), 0, reinterpret_cast<hipStream_t>(stream), in, out, (size_t)n);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
