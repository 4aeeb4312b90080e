// DTU evaluation front end on the device (C ABI: include/ibgs_dtu.h; Python: ibgs_amd/dtu.py): the host stages of the reference's DTU scripts that sit
// between a mesh and its Chamfer distance -- the dilation of the object masks, the culling of the mesh against them and its compaction
// (scripts/eval_dtu/evaluate_single_scene.py:53-95: cv2 / skimage, torch CPU grid_sample, trimesh), the observation-mask filter of the sampled cloud and
// the ground-plane filter of the ground truth (eval.py:98-110, 126-130: numpy).  This is the project's own statement of those stages (DESIGN.md section 11,
// "DTU evaluation"); tests/dtu_ref.py restates it with numpy.  Compiled with -ffp-contract=off: the operation orders below ARE the contract.
//
// CONTRACT
//   dilate     out[y, x] = OR of in[y + dy, x + dx] over the integer (dx, dy) with dx dx + dy dy <= r r and (y + dy, x + dx) inside the image: skimage's
//              binary_dilation with a disc footprint, zero outside the image.  Bits: bit (x & 63) of word (x >> 6) of the row, zero at x >= W.
//   cull       vertex (x, y, z), view i with rows P0, P1, P2, all f32, one rounding per operation, left to right:
//                c_r = ((P_r[0] x + P_r[1] y) + P_r[2] z) + P_r[3];  u = c_0 / (c_2 + 1e-6f), v = c_1 / (c_2 + 1e-6f)
//                gx = (u / (W - 1) - 0.5f) * 2, gy = (v / (H - 1) - 0.5f) * 2;  valid = -1 < gx < 1 and -1 < gy < 1 (false when either is NaN)
//                ix = rint(((gx + 1) / 2) * (W - 1)), iy = rint(((gy + 1) / 2) * (H - 1)), ties to even
//                pass_i = not valid, or bit (i, iy, ix);  keep = AND over the views (no view keeps everything)
//              -- torch's CPU grid_sample(mode = "nearest", align_corners = True) round trip of the reference, reproduced rather than simplified to rint(u).
//   compact    the kept vertices in index order (referenced by a surviving face or not), position v * scale + offset in f32 (a multiply, then an add), colours
//              and normals copied; a face survives iff its three indices are kept; order kept, indices re-mapped.
//   obs        in f64 from the f32 point: inbound = all_k (p_k >= lo_k and p_k < hi_k) with the f32 bounds lo, hi; g_k = rint((p_k - bb0_k) / res), ties to even;
//              in_obs = inbound and all_k (0 <= g_k < shape_k) and obs_mask[g_0, g_1, g_2] != 0.
//   plane      ((P_0 x + P_1 y) + P_2 z) + P_3 > 0 in f64 from the f32 point.
//
// KERNELS
//   dtu_pack_kernel            one wave per 64 pixels of a row: its ballot is the word of undilated bits
//   dtu_dilate_kernel          one wave per output word.  The disc is the union over |dy| <= r of the row spans |dx| <= w(dy) = floor(sqrt(r r - dy dy)), so the
//                              output row is the OR over dy of row y + dy dilated horizontally by w(dy).  Lane l takes dy = l - r (64 rows at a time when
//                              2 r + 1 > 64): it loads the words of its row that can reach the output word (ceil(r / 64) on either side), ORs them with themselves
//                              shifted by 1, 2, 4, .. -- after k steps a word holds the OR of the shifts 0 .. 2^k - 1, a last shorter step completes 0 .. w -- once
//                              towards higher and once towards lower x, and the OR of the lanes' centre words (wave_reduce, block_ops.h) is the output word.
//                              5 steps at r = 24.  No LDS, no atomics, no per-pixel work at all: every instruction handles 64 pixels of one row.
//   dtu_cull_vertices_kernel   one thread per vertex, looping over the views (their 12 matrix entries are wave-uniform); a thread stops at the first view that
//                              rejects its vertex.  One 8-byte gather into the mask bits per (vertex, view that sees it).
//   dtu_mark_kernel            keep flag per vertex and per face (u32, for the scans); exclusive_scan_u32 (scan_sort.hip) turns both into output rows
//   dtu_totals_kernel          V', F' into the state words
//   dtu_emit_faces_kernel / dtu_emit_vertices_kernel (one thread per float)
//   dtu_obs_filter_kernel / dtu_above_plane_kernel      one thread per point
// Indices outside their range are never dereferenced; out-of-range conditions are counted in the state words and the caller fails the call.
#include <cmath>
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_dtu.h"

namespace ibgs {

constexpr int DT = 256;                              // threads per workgroup of every kernel here
constexpr int DTU_MAX_K = (IBGS_DTU_MAX_RADIUS + 63) / 64;          // words on either side of an output word that a disc can reach
constexpr int DTU_MAX_STEP = 32;                     // longest shift of one doubling step (so that 64 - step is a shift too)

struct op_or { __device__ __forceinline__ unsigned long long operator()(unsigned long long x, unsigned long long y, int = 0) const { return x | y; } };

struct DtuScratch {
    uint32_t* vpos;                          // V + 1: keep flags, then output row of every vertex; [V] = V'
    uint32_t* fpos;                          // F + 1: keep flags, then output row of every face; [F] = F'
    uint32_t* scan; size_t scan_elems;
    static DtuScratch carve(char* base, int64_t V, int64_t F, size_t* total)
    {
        DtuScratch d;
        Carver c(base);
        d.vpos = c.take<uint32_t>((size_t)V + 1);
        d.fpos = c.take<uint32_t>((size_t)F + 1);
        d.scan_elems = scan_scratch_elems((size_t)(V > F ? V : F) + 1);
        d.scan = c.take<uint32_t>(d.scan_elems);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return d;
    }
};

// ---- dilation ------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT) dtu_pack_kernel(const uint8_t* __restrict__ masks, uint32_t W, uint32_t WW, size_t nwords, unsigned long long* __restrict__ bits)
{
    const size_t word = (size_t)blockIdx.x * (DT / 64) + (threadIdx.x >> 6);          // (wave-uniform)
    if (word >= nwords) return;
    const size_t row = word / WW;
    const uint32_t x = (uint32_t)(word - row * WW) * 64u + (threadIdx.x & 63);
    const bool set = x < W && masks[row * W + x] != 0;
    const unsigned long long b = __ballot(set);
    if ((threadIdx.x & 63) == 0) bits[word] = b;
}

// floor(sqrt(v)) for 0 <= v <= 255 * 255 (exact in f32; the two loops settle the rounding of the root)
__device__ __forceinline__ int dtu_isqrt(int v)
{
    int w = (int)sqrtf((float)v);
    while (w * w > v) --w;
    while ((w + 1) * (w + 1) <= v) ++w;
    return w;
}

// K = words on either side of the output word that the radius can reach (r <= 64 K)
template <int K>
__global__ void __launch_bounds__(DT) dtu_dilate_kernel(const unsigned long long* __restrict__ bits, int H, int W, int WW, int r, size_t nwords,
                                                        unsigned long long* __restrict__ out)
{
    const size_t word = (size_t)blockIdx.x * (DT / 64) + (threadIdx.x >> 6);          // (wave-uniform: whole waves leave here)
    if (word >= nwords) return;
    const int lane = threadIdx.x & 63;
    const size_t row = word / (size_t)WW;
    const int wx = (int)(word - row * (size_t)WW);
    const size_t view = row / (size_t)H;
    const int y = (int)(row - view * (size_t)H);
    unsigned long long acc = 0;
    for (int base = -r; base <= r; base += 64) {
        const int dy = base + lane, yy = y + dy;
        if (dy > r || yy < 0 || yy >= H) continue;
        const unsigned long long* __restrict__ src = bits + (view * (size_t)H + (size_t)yy) * (size_t)WW;
        // lo[j] = word wx - K + j (j = K: the centre), spreading towards higher x; hi[j] = word wx + j (j = 0: the centre), spreading towards lower x
        unsigned long long lo[K + 1], hi[K + 1];
#pragma unroll
        for (int j = 0; j <= K; ++j) {
            const int a = wx - K + j, b = wx + j;
            lo[j] = a >= 0 ? src[a] : 0ull;
            hi[j] = b < WW ? src[b] : 0ull;
        }
        const int w = dtu_isqrt(r * r - dy * dy);
        int cover = 1;                              // the words hold the OR of the shifts 0 .. cover - 1
        while (cover < w + 1) {
            const int s = min(min(cover, w + 1 - cover), DTU_MAX_STEP);          // 1 <= s <= 32
#pragma unroll
            for (int j = K; j >= 1; --j) lo[j] |= (lo[j] << s) | (lo[j - 1] >> (64 - s));
            lo[0] |= lo[0] << s;                    // (what would come in from word wx - K - 1 is more than r pixels from the output word)
#pragma unroll
            for (int j = 0; j < K; ++j) hi[j] |= (hi[j] >> s) | (hi[j + 1] << (64 - s));
            hi[K] |= hi[K] >> s;
            cover += s;
        }
        acc |= lo[K] | hi[0];
    }
    acc = wave_reduce(acc, op_or());
    if (lane == 0) {
        const int left = W - wx * 64;               // pixels of the row from this word on: bits at x >= W stay zero
        out[word] = left >= 64 ? acc : acc & ((1ull << left) - 1ull);
    }
}

// ---- vertex culling ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT) dtu_cull_vertices_kernel(const float* __restrict__ vert, uint32_t V, const float* __restrict__ proj, int n, int H, int W, int WW,
                                                               const unsigned long long* __restrict__ bits, uint8_t* __restrict__ keep, uint32_t* state)
{
    const uint32_t t = blockIdx.x * DT + threadIdx.x;
    if (t >= V) return;
    const float x = vert[(size_t)t * 3], y = vert[(size_t)t * 3 + 1], z = vert[(size_t)t * 3 + 2];
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    bool kept = true;
    for (int i = 0; i < n && kept; ++i) {
        const float* __restrict__ P = proj + (size_t)i * 12;
        const float c0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
        const float c1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
        const float c2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
        const float den = c2 + 1e-6f;
        const float u = c0 / den, v = c1 / den;
        const float gx = (u / wm1 - 0.5f) * 2.0f, gy = (v / hm1 - 0.5f) * 2.0f;
        if (!(gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f)) continue;          // not seen (NaN lands here): the view does not reject
        const int ix = (int)rintf(((gx + 1.0f) / 2.0f) * wm1), iy = (int)rintf(((gy + 1.0f) / 2.0f) * hm1);
        if ((unsigned)ix >= (unsigned)W || (unsigned)iy >= (unsigned)H) { atomicAdd(state + IBGS_DTU_OVERRUN, 1u); continue; }          // (cannot happen: -1 < g < 1)
        const unsigned long long word = bits[((size_t)i * (size_t)H + (size_t)iy) * (size_t)WW + (size_t)(ix >> 6)];
        kept = ((word >> (ix & 63)) & 1ull) != 0ull;
    }
    keep[t] = kept ? 1 : 0;
}

// ---- compaction ----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT) dtu_mark_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep, uint32_t V, uint32_t F,
                                                      uint32_t* __restrict__ vflag, uint32_t* __restrict__ fflag, uint32_t* state)
{
    const uint32_t t = blockIdx.x * DT + threadIdx.x;
    if (t < V) vflag[t] = keep[t] != 0 ? 1u : 0u;
    if (t < F) {
        const uint32_t a = (uint32_t)faces[(size_t)t * 3], b = (uint32_t)faces[(size_t)t * 3 + 1], c = (uint32_t)faces[(size_t)t * 3 + 2];
        bool k = false;
        if (a >= V || b >= V || c >= V) atomicAdd(state + IBGS_DTU_BAD_FACES, 1u);
        else k = keep[a] != 0 && keep[b] != 0 && keep[c] != 0;
        fflag[t] = k ? 1u : 0u;
    }
}

__global__ void dtu_totals_kernel(const uint32_t* __restrict__ vpos, const uint32_t* __restrict__ fpos, uint32_t V, uint32_t F, uint32_t* __restrict__ state)
{
    state[IBGS_DTU_VERTICES_OUT] = vpos[V];
    state[IBGS_DTU_FACES_OUT] = fpos[F];
}

__global__ void __launch_bounds__(DT) dtu_emit_faces_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F, const uint32_t* __restrict__ vpos,
                                                            const uint32_t* __restrict__ fpos, uint32_t V_out, uint32_t F_out, int32_t* __restrict__ faces_out,
                                                            uint32_t* state)
{
    const uint32_t t = blockIdx.x * DT + threadIdx.x;
    if (t >= F) return;
    const uint32_t o = fpos[t];
    if (fpos[t + 1] == o) return;
    uint32_t v[3] = {(uint32_t)faces[(size_t)t * 3], (uint32_t)faces[(size_t)t * 3 + 1], (uint32_t)faces[(size_t)t * 3 + 2]};
    bool ok = o < F_out && v[0] < V && v[1] < V && v[2] < V;          // (a kept face's indices passed this test in the mark kernel already)
    if (ok) {
        for (int k = 0; k < 3; ++k) v[k] = vpos[v[k]];
        ok = v[0] < V_out && v[1] < V_out && v[2] < V_out;
    }
    if (!ok) { atomicAdd(state + IBGS_DTU_OVERRUN, 1u); return; }
    for (int k = 0; k < 3; ++k) faces_out[(size_t)o * 3 + k] = (int32_t)v[k];
}

struct DtuMove { float scale, off[3]; };

// one thread per float of a vertex row: the reads are contiguous, the writes contiguous up to the gaps of the dropped rows
__global__ void __launch_bounds__(DT) dtu_emit_vertices_kernel(const float* __restrict__ vert, const uint32_t* __restrict__ colors, const uint32_t* __restrict__ normals,
                                                               uint32_t V, const uint32_t* __restrict__ vpos, uint32_t V_out, DtuMove mv, float* __restrict__ vert_out,
                                                               uint32_t* __restrict__ colors_out, uint32_t* __restrict__ normals_out, uint32_t* state)
{
    const size_t i = (size_t)blockIdx.x * DT + threadIdx.x;
    if (i >= (size_t)V * 3) return;
    const uint32_t v = (uint32_t)(i / 3), k = (uint32_t)(i - (size_t)v * 3);
    const uint32_t o = vpos[v];
    if (vpos[v + 1] == o) return;
    if (o >= V_out) { if (k == 0) atomicAdd(state + IBGS_DTU_OVERRUN, 1u); return; }
    const float off = k == 0 ? mv.off[0] : (k == 1 ? mv.off[1] : mv.off[2]);
    const float scaled = vert[i] * mv.scale;
    vert_out[(size_t)o * 3 + k] = scaled + off;
    if (colors_out) colors_out[(size_t)o * 3 + k] = colors[i];          // words, not floats: bit for bit
    if (normals_out) normals_out[(size_t)o * 3 + k] = normals[i];
}

// ---- the point filters ---------------------------------------------------------------------------------------------------------------------------
struct DtuBox { float lo[3], hi[3]; double bb0[3], res; int shape[3]; };

__global__ void __launch_bounds__(DT) dtu_obs_filter_kernel(const float* __restrict__ pts, uint32_t N, const uint8_t* __restrict__ obs, DtuBox bx,
                                                            uint8_t* __restrict__ inbound, uint8_t* __restrict__ in_obs, uint32_t* state)
{
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i >= N) return;
    bool finite = true, in = true, on_grid = true;
    size_t cell = 0;
    for (int k = 0; k < 3; ++k) {
        const float pf = pts[(size_t)i * 3 + k];
        finite = finite && isfinite(pf);
        const double p = (double)pf;
        in = in && p >= (double)bx.lo[k] && p < (double)bx.hi[k];
        const double g = rint((p - bx.bb0[k]) / bx.res);
        if (g >= 0.0 && g < (double)bx.shape[k]) cell = cell * (size_t)bx.shape[k] + (size_t)(int)g;          // (NaN fails both)
        else on_grid = false;
    }
    if (!finite) { atomicAdd(state + IBGS_DTU_BAD_POINTS, 1u); in = false; }
    inbound[i] = in ? 1 : 0;
    in_obs[i] = (in && on_grid && obs[cell] != 0) ? 1 : 0;
}

struct DtuPlane { double p[4]; };

__global__ void __launch_bounds__(DT) dtu_above_plane_kernel(const float* __restrict__ pts, uint32_t N, DtuPlane pl, uint8_t* __restrict__ out, uint32_t* state)
{
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i >= N) return;
    const float xf = pts[(size_t)i * 3], yf = pts[(size_t)i * 3 + 1], zf = pts[(size_t)i * 3 + 2];
    if (!(isfinite(xf) && isfinite(yf) && isfinite(zf))) { atomicAdd(state + IBGS_DTU_BAD_POINTS, 1u); out[i] = 0; return; }
    const double d = ((pl.p[0] * (double)xf + pl.p[1] * (double)yf) + pl.p[2] * (double)zf) + pl.p[3];
    out[i] = d > 0.0 ? 1 : 0;
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------------------------
static bool dtu_image_ok(const char* who, int64_t n, int64_t H, int64_t W, size_t* nwords)
{
    if (n < 0 || n >= (int64_t(1) << 31) || H < 2 || W < 2 || H > IBGS_DTU_MAX_SIDE || W > IBGS_DTU_MAX_SIDE) {
        if (who) set_error("%s: n %lld / H %lld / W %lld out of range (0 <= n < 2^31, 2 <= H, W <= %d)", who, (long long)n, (long long)H, (long long)W, IBGS_DTU_MAX_SIDE);
        return false;
    }
    const unsigned long long words = (unsigned long long)n * (unsigned long long)H * (unsigned long long)((W + 63) / 64);
    if (words >= (1ull << 32)) {
        if (who) set_error("%s: %llu mask words (limit: n H ceil(W / 64) < 2^32)", who, words);
        return false;
    }
    *nwords = (size_t)words;
    return true;
}

static bool dtu_mesh_ok(const char* who, int32_t V, int32_t F)
{
    if (V < 0 || F < 0 || F >= (1 << 30)) { set_error("%s: V %d / F %d out of range (V >= 0, 0 <= F < 2^30)", who, V, F); return false; }
    return true;
}

template <int K>
static void dtu_launch_dilate(hipStream_t s, const unsigned long long* bits, int H, int W, int WW, int r, size_t nwords, unsigned long long* out)
{
    hipLaunchKernelGGL(dtu_dilate_kernel<K>, dim3(grid_for(nwords, DT / 64)), dim3(DT), 0, s, bits, H, W, WW, r, nwords, out);
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_dtu_required_dilate_scratch(int64_t n, int64_t H, int64_t W)
{
    size_t nwords = 0;
    if (!dtu_image_ok(nullptr, n, H, W, &nwords)) return 0;
    return nwords * sizeof(uint64_t) + 128;
}

int32_t ibgs_dtu_dilate(void* stream, int32_t n, int32_t H, int32_t W, int32_t radius, const uint8_t* masks, void* scratch, size_t scratch_bytes, uint64_t* out)
{
    size_t nwords = 0;
    if (!dtu_image_ok("dtu_dilate", n, H, W, &nwords)) return -IBGS_ERR_INVALID;
    if (radius < 0 || radius > IBGS_DTU_MAX_RADIUS) { set_error("dtu_dilate: radius %d out of range (0 .. %d)", radius, IBGS_DTU_MAX_RADIUS); return -IBGS_ERR_INVALID; }
    if (nwords == 0) return 0;
    if (!masks || !out) { set_error("dtu_dilate: null masks or output"); return -IBGS_ERR_INVALID; }
    if (!arena_ok("dtu_dilate", "scratch", scratch, scratch_bytes, nwords * sizeof(uint64_t) + 128)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* bits = static_cast<unsigned long long*>(scratch);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(out);
    const int WW = (W + 63) / 64;
    hipLaunchKernelGGL(dtu_pack_kernel, dim3(grid_for(nwords, DT / 64)), dim3(DT), 0, s, masks, (uint32_t)W, (uint32_t)WW, nwords, radius == 0 ? dst : bits);
    IBGS_HIP(hipGetLastError());
    if (radius == 0) return 0;
    static_assert(DTU_MAX_K == 4, "one instantiation per reach");
    switch ((radius + 63) / 64) {
    case 1: dtu_launch_dilate<1>(s, bits, H, W, WW, radius, nwords, dst); break;
    case 2: dtu_launch_dilate<2>(s, bits, H, W, WW, radius, nwords, dst); break;
    case 3: dtu_launch_dilate<3>(s, bits, H, W, WW, radius, nwords, dst); break;
    default: dtu_launch_dilate<4>(s, bits, H, W, WW, radius, nwords, dst); break;
    }
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_dtu_cull_vertices(void* stream, int32_t V, const float* vertices, int32_t n, const float* projections, int32_t H, int32_t W, const uint64_t* bits,
                               uint8_t* keep, uint32_t* state)
{
    size_t nwords = 0;
    if (V < 0) { set_error("dtu_cull_vertices: V %d out of range", V); return -IBGS_ERR_INVALID; }
    if (!dtu_image_ok("dtu_cull_vertices", n, H, W, &nwords)) return -IBGS_ERR_INVALID;
    if (V == 0) return 0;
    if (!vertices || !keep || !state || (n > 0 && (!projections || !bits))) { set_error("dtu_cull_vertices: null array"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(dtu_cull_vertices_kernel, dim3(grid_for((size_t)V, DT)), dim3(DT), 0, reinterpret_cast<hipStream_t>(stream), vertices, (uint32_t)V, projections, n, H, W,
                       (W + 63) / 64, reinterpret_cast<const unsigned long long*>(bits), keep, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

size_t ibgs_dtu_required_cull_scratch(int64_t V, int64_t F)
{
    if (V < 0 || F < 0 || V >= (int64_t(1) << 31) || F >= (int64_t(1) << 30)) return 0;
    size_t total = 0;
    DtuScratch::carve(nullptr, V, F, &total);
    return total;
}

int32_t ibgs_dtu_cull_count(void* stream, int32_t V, int32_t F, const int32_t* faces, const uint8_t* keep, void* scratch, size_t scratch_bytes, uint32_t* state)
{
    if (!dtu_mesh_ok("dtu_cull_count", V, F)) return -IBGS_ERR_INVALID;
    if ((V > 0 && !keep) || (F > 0 && !faces) || !state) { set_error("dtu_cull_count: null array"); return -IBGS_ERR_INVALID; }
    size_t need = 0;
    const DtuScratch sc = DtuScratch::carve(static_cast<char*>(scratch), V, F, &need);
    if (!arena_ok("dtu_cull_count", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t items = (size_t)(V > F ? V : F);
    if (items > 0) {
        hipLaunchKernelGGL(dtu_mark_kernel, dim3(grid_for(items, DT)), dim3(DT), 0, s, faces, keep, (uint32_t)V, (uint32_t)F, sc.vpos, sc.fpos, state);
        IBGS_HIP(hipGetLastError());
    }
    int rc = exclusive_scan_u32(s, sc.vpos, sc.vpos, (size_t)V, sc.scan, sc.scan_elems, true);          // (writes the total to [V], for V = 0 too)
    if (rc) return rc;
    rc = exclusive_scan_u32(s, sc.fpos, sc.fpos, (size_t)F, sc.scan, sc.scan_elems, true);
    if (rc) return rc;
    hipLaunchKernelGGL(dtu_totals_kernel, dim3(1), dim3(1), 0, s, sc.vpos, sc.fpos, (uint32_t)V, (uint32_t)F, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_dtu_cull_emit(void* stream, int32_t V, int32_t F, const float* vertices, const int32_t* faces, const float* colors, const float* normals,
                           const void* scratch, size_t scratch_bytes, float scale, const float* host_offset, int32_t V_out, int32_t F_out, float* vertices_out,
                           int32_t* faces_out, float* colors_out, float* normals_out, uint32_t* state)
{
    if (!dtu_mesh_ok("dtu_cull_emit", V, F)) return -IBGS_ERR_INVALID;
    if (V_out < 0 || F_out < 0 || V_out > V || F_out > F) { set_error("dtu_cull_emit: V' %d / F' %d out of range (V %d, F %d)", V_out, F_out, V, F); return -IBGS_ERR_INVALID; }
    if (!host_offset || !state || (V > 0 && !vertices) || (F > 0 && !faces) || (V_out > 0 && !vertices_out) || (F_out > 0 && !faces_out)
        || (colors_out && !colors) || (normals_out && !normals)) {
        set_error("dtu_cull_emit: null array"); return -IBGS_ERR_INVALID;
    }
    size_t need = 0;
    const DtuScratch sc = DtuScratch::carve(static_cast<char*>(const_cast<void*>(scratch)), V, F, &need);
    if (!arena_ok("dtu_cull_emit", "scratch", scratch, scratch_bytes, need)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (F > 0 && F_out > 0) {
        hipLaunchKernelGGL(dtu_emit_faces_kernel, dim3(grid_for((size_t)F, DT)), dim3(DT), 0, s, faces, (uint32_t)V, (uint32_t)F, sc.vpos, sc.fpos, (uint32_t)V_out,
                           (uint32_t)F_out, faces_out, state);
        IBGS_HIP(hipGetLastError());
    }
    if (V > 0 && V_out > 0) {
        DtuMove mv;
        mv.scale = scale;
        for (int k = 0; k < 3; ++k) mv.off[k] = host_offset[k];
        hipLaunchKernelGGL(dtu_emit_vertices_kernel, dim3(grid_for((size_t)V * 3, DT)), dim3(DT), 0, s, vertices, reinterpret_cast<const uint32_t*>(colors),
                           reinterpret_cast<const uint32_t*>(normals), (uint32_t)V, sc.vpos, (uint32_t)V_out, mv, vertices_out, reinterpret_cast<uint32_t*>(colors_out),
                           reinterpret_cast<uint32_t*>(normals_out), state);
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

int32_t ibgs_dtu_obs_filter(void* stream, int32_t N, const float* points, const uint8_t* obs_mask, int32_t X, int32_t Y, int32_t Z, const float* host_lo,
                            const float* host_hi, const double* host_bb0, double res, uint8_t* inbound, uint8_t* in_obs, uint32_t* state)
{
    if (N < 0) { set_error("dtu_obs_filter: N %d out of range", N); return -IBGS_ERR_INVALID; }
    if (X < 1 || Y < 1 || Z < 1 || (unsigned long long)X * (unsigned long long)Y * (unsigned long long)Z >= (1ull << 40)) {
        set_error("dtu_obs_filter: obs_mask shape %d x %d x %d out of range", X, Y, Z); return -IBGS_ERR_INVALID;
    }
    if (!host_lo || !host_hi || !host_bb0) { set_error("dtu_obs_filter: null bounds"); return -IBGS_ERR_INVALID; }
    if (!(res > 0.0) || !std::isfinite(res)) { set_error("dtu_obs_filter: res must be a finite positive number"); return -IBGS_ERR_INVALID; }
    DtuBox bx;
    for (int k = 0; k < 3; ++k) {
        if (!(std::isfinite(host_lo[k]) && std::isfinite(host_hi[k]) && std::isfinite(host_bb0[k]))) { set_error("dtu_obs_filter: non-finite bounds"); return -IBGS_ERR_INVALID; }
        bx.lo[k] = host_lo[k]; bx.hi[k] = host_hi[k]; bx.bb0[k] = host_bb0[k];
    }
    bx.res = res; bx.shape[0] = X; bx.shape[1] = Y; bx.shape[2] = Z;
    if (N == 0) return 0;
    if (!points || !obs_mask || !inbound || !in_obs || !state) { set_error("dtu_obs_filter: null array"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(dtu_obs_filter_kernel, dim3(grid_for((size_t)N, DT)), dim3(DT), 0, reinterpret_cast<hipStream_t>(stream), points, (uint32_t)N, obs_mask, bx, inbound,
                       in_obs, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_dtu_above_plane(void* stream, int32_t N, const float* points, const double* host_plane, uint8_t* out, uint32_t* state)
{
    if (N < 0) { set_error("dtu_above_plane: N %d out of range", N); return -IBGS_ERR_INVALID; }
    if (!host_plane) { set_error("dtu_above_plane: null plane"); return -IBGS_ERR_INVALID; }
    DtuPlane pl;
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(host_plane[k])) { set_error("dtu_above_plane: non-finite plane"); return -IBGS_ERR_INVALID; }
        pl.p[k] = host_plane[k];
    }
    if (N == 0) return 0;
    if (!points || !out || !state) { set_error("dtu_above_plane: null array"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(dtu_above_plane_kernel, dim3(grid_for((size_t)N, DT)), dim3(DT), 0, reinterpret_cast<hipStream_t>(stream), points, (uint32_t)N, pl, out, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
