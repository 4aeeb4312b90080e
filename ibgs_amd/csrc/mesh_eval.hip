// Mesh evaluation on the device (C ABI: include/ibgs_mesh_eval.h; Python: ibgs_amd/mesh_eval.py): the stages of the reference's DTU script
// (scripts/eval_dtu/eval.py: sample the mesh, thin the cloud, nearest distances both ways) and the counts of its TnT script
// (scripts/tnt_eval/evaluation.py:176-180), which run on the host through Open3D, a multiprocessing pool and sklearn's kd-tree.  This is the project's own
// statement of those stages ("Mesh evaluation"); tests/mesh_eval_ref.py restates it with numpy / scipy / sklearn.
// Compiled with -ffp-contract=off: the operation orders below ARE the contract.
//
// CONTRACT
//   sample     triangle (p0, p1, p2), f32 vertices widened to f64, v1 = p1 - p0, v2 = p2 - p0, l = sqrt((x x + y y) + z z),
//              c = (v1y v2z - v1z v2y, v1z v2x - v1x v2z, v1x v2y - v1y v2x), A = |c|; if !(A > 0): none.  thr = density sqrt(l1 l2 / A),
//              n1 = floor(l1 / thr), n2 = floor(l2 / thr); n1 = 0 or n2 = 0: none.  a = (i + 0.5) / n1, b = (j + 0.5) / n2 for i = 0..n1, j = 0..n2 with
//              a + b < 1; sample = ((v1 a) + (v2 b)) + p0 per component, all in f64, rounded once to f32.  i-major in a triangle, triangles in index order.
//   thin       point i (visited in ascending rank) is kept iff no kept j of smaller rank has d2(i, j) <= r r: the lexicographically first maximal
//              independent set of the radius graph.  d2 = (dx dx + dy dy) + dz dz in f32, r r formed in f32.
//   nearest    best = min over the targets of d2 (same f32 formula); dist = the correctly rounded f32 square root of best, index = the smallest target
//              index attaining best; best >= max_dist max_dist (f32): dist = +inf, index = -1.
//   reduce     f64 sum and count of the dist < threshold (f32 compare).
//
// SEARCH STRUCTURE (thin and nearest share it; the Python layer orders the points with torch.sort on the Morton keys of meval_keys_kernel)
//   The points in Morton order as float4 {x, y, z, tag}; over them a hierarchy of axis-aligned boxes with a fan-out of 8: a leaf box bounds 8 consecutive
//   points, a box of level l + 1 bounds 8 consecutive boxes of level l, up to a level of at most 8 boxes.  Boxes are the min / max of the f32 coordinates, so
//   they are exact whatever the keys are: the keys decide speed alone.  The lower bound of a query to a box uses the SAME f32 formula with
//   dx = max(lo - q, q - hi, 0); f32 subtraction, product and sum are monotone, so it never exceeds the d2 of a point inside: pruning on it is exact.
//   A walk is a depth-first descent with one cursor per level.  A query with nothing within max_dist is pruned at the top levels (a few dozen box tests),
//   whatever max_dist is in units of the point spacing: no cell lists are enumerated.
//
// KERNELS
//   meval_sample_count_kernel   one thread per triangle: its sample count.  Triangles of up to 256 candidates (i, j) are walked by their thread; larger ones
//                               by the whole wave afterwards, 64 candidates at a time (ballot + popcount keep the i-major order), so one triangle with
//                               10^5 samples among thousands with none costs 3 000 wave steps, not 10^5 thread steps.  Workgroup sums in 64 bits.
//   meval_scan_blocks_kernel    exclusive 64-bit scan of the workgroup sums (one workgroup), total to total[0]
//   meval_sample_emit_kernel    the same walk, writing; a triangle's first row = its workgroup's offset + the scan of the counts inside the workgroup
//   meval_keys_kernel           Morton keys; counts non-finite points
//   meval_gather_kernel / meval_leaf_box_kernel / meval_box_kernel       the hierarchy
//   meval_thin_round_kernel     one round: an undecided point walks its radius neighbourhood; an earlier kept neighbour removes it, no earlier undecided
//                               neighbour keeps it.  Both decisions are final, so reading statuses that the same launch is writing only ever decides
//                               sooner, never differently: the fixed point is unique and the mask bit-identical from run to run.
//   meval_nearest_kernel        greedy descent to the nearest leaf for a first bound, then the pruned walk
//   meval_reduce_kernel
// Face indices outside [0, V) are never dereferenced; out-of-range conditions are counted in the state words and the caller fails the call.
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_mesh_eval.h"

namespace ibgs {

constexpr int ET = 256;                              // threads per workgroup of every kernel here but the block scan
constexpr int MEVAL_LEVELS = 12;                     // 8^11 leaves > 2^31 / 8
constexpr uint32_t MEVAL_SMALL = 256;                // candidates a single thread walks
constexpr uint32_t LEAF = IBGS_MEVAL_LEAF;

struct MevalTree {
    const float4* pts;                               // N, Morton order: {x, y, z, tag}
    const float4* box[MEVAL_LEVELS];                 // two float4 per box: {lo x, lo y, lo z, hi x}, {hi y, hi z, -, -}
    uint32_t n[MEVAL_LEVELS];
    int L;
    uint32_t N;
};

// carve (or size, base == nullptr) the hierarchy of N > 0 points
static MevalTree meval_tree_carve(char* base, int64_t N, size_t* total)
{
    MevalTree t;
    Carver c(base);
    t.N = (uint32_t)N;
    t.pts = c.take<float4>((size_t)N);
    t.L = 0;
    for (size_t n = ((size_t)N + LEAF - 1) / LEAF;; n = (n + LEAF - 1) / LEAF) {
        t.n[t.L] = (uint32_t)n;
        t.box[t.L] = c.take<float4>(n * 2);
        ++t.L;
        if (n <= LEAF || t.L == MEVAL_LEVELS) break;
    }
    for (int l = t.L; l < MEVAL_LEVELS; ++l) { t.n[l] = 0; t.box[l] = nullptr; }
    if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
    return t;
}

__device__ __forceinline__ uint32_t meval_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void meval_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ float meval_d2(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }

// lower bound of d2 over the box (see SEARCH STRUCTURE)
__device__ __forceinline__ float meval_box_d2(const float4* __restrict__ box, uint32_t node, float qx, float qy, float qz)
{
    const float4 a = box[(size_t)node * 2], b = box[(size_t)node * 2 + 1];
    const float dx = fmaxf(fmaxf(a.x - qx, qx - a.w), 0.0f);
    const float dy = fmaxf(fmaxf(a.y - qy, qy - b.x), 0.0f);
    const float dz = fmaxf(fmaxf(a.z - qz, qz - b.y), 0.0f);
    return meval_d2(dx, dy, dz);
}

// Depth-first walk: prune(lower bound) -> skip the box; visit(point, d2, position) -> true ends the walk.
template <typename Prune, typename Visit>
__device__ __forceinline__ void meval_walk(const MevalTree& t, float qx, float qy, float qz, Prune prune, Visit visit)
{
    uint32_t cur[MEVAL_LEVELS], end[MEVAL_LEVELS];
    int lvl = t.L - 1;
    cur[lvl] = 0; end[lvl] = t.n[lvl];
    while (lvl < t.L) {
        if (cur[lvl] == end[lvl]) { ++lvl; continue; }
        const uint32_t node = cur[lvl]++;
        if (prune(meval_box_d2(t.box[lvl], node, qx, qy, qz))) continue;
        const uint32_t b = node * LEAF;
        if (lvl == 0) {
            const uint32_t e = min(t.N, b + LEAF);
            for (uint32_t k = b; k < e; ++k) {
                const float4 p = t.pts[k];
                if (visit(p, meval_d2(qx - p.x, qy - p.y, qz - p.z), k)) return;
            }
        } else {
            --lvl;
            cur[lvl] = b; end[lvl] = min(t.n[lvl], b + LEAF);
        }
    }
}

// ---- surface sampling ----------------------------------------------------------------------------------------------------------------------------
struct TriSetup { double p0[3], v1[3], v2[3]; uint32_t n1, n2; };          // n1 = 0: no samples

__device__ __forceinline__ void tri_setup(const float* __restrict__ vert, const int32_t* __restrict__ faces, uint32_t V, uint32_t t, double density,
                                          TriSetup& s, uint32_t* state /* null: do not count */)
{
    s.n1 = s.n2 = 0;
    const uint32_t a = (uint32_t)faces[(size_t)t * 3], b = (uint32_t)faces[(size_t)t * 3 + 1], c = (uint32_t)faces[(size_t)t * 3 + 2];
    if (a >= V || b >= V || c >= V) { if (state) atomicAdd(state + IBGS_MEVAL_BAD_FACES, 1u); return; }          // (negative indices wrap above V)
    for (int k = 0; k < 3; ++k) {
        s.p0[k] = (double)vert[(size_t)a * 3 + k];
        s.v1[k] = (double)vert[(size_t)b * 3 + k] - s.p0[k];
        s.v2[k] = (double)vert[(size_t)c * 3 + k] - s.p0[k];
    }
    const double l1 = sqrt((s.v1[0] * s.v1[0] + s.v1[1] * s.v1[1]) + s.v1[2] * s.v1[2]);
    const double l2 = sqrt((s.v2[0] * s.v2[0] + s.v2[1] * s.v2[1]) + s.v2[2] * s.v2[2]);
    const double cx = s.v1[1] * s.v2[2] - s.v1[2] * s.v2[1], cy = s.v1[2] * s.v2[0] - s.v1[0] * s.v2[2], cz = s.v1[0] * s.v2[1] - s.v1[1] * s.v2[0];
    const double area2 = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(area2 > 0.0)) return;
    const double thr = density * sqrt(l1 * l2 / area2);
    const double f1 = floor(l1 / thr), f2 = floor(l2 / thr);
    if (!(f1 >= 1.0 && f2 >= 1.0)) return;          // (NaN lands here too)
    if (f1 > (double)IBGS_MEVAL_MAX_SIDE || f2 > (double)IBGS_MEVAL_MAX_SIDE) { if (state) atomicAdd(state + IBGS_MEVAL_SAMPLE_OVERFLOW, 1u); return; }
    s.n1 = (uint32_t)f1; s.n2 = (uint32_t)f2;
}

__device__ __forceinline__ void tri_emit(const TriSetup& s, double a, double b, uint64_t row, uint64_t n_out, float* __restrict__ out, uint32_t* state)
{
    if (row >= n_out) { atomicAdd(state + IBGS_MEVAL_OVERRUN, 1u); return; }
    for (int k = 0; k < 3; ++k) out[row * 3 + k] = (float)((s.v1[k] * a + s.v2[k] * b) + s.p0[k]);
}

// one thread, one triangle: a + b < 1 is monotone in j (b grows with j and the f64 sum is monotone), so a row ends at its first failure
template <bool EMIT>
__device__ __forceinline__ uint32_t tri_walk_serial(const TriSetup& s, uint64_t row0, uint64_t n_out, float* __restrict__ out, uint32_t* state)
{
    uint32_t n = 0;
    const double d1 = (double)s.n1, d2 = (double)s.n2;
    for (uint32_t i = 0; i <= s.n1; ++i) {
        const double a = ((double)i + 0.5) / d1;
        for (uint32_t j = 0; j <= s.n2; ++j) {
            const double b = ((double)j + 0.5) / d2;
            if (!(a + b < 1.0)) break;
            if (EMIT) tri_emit(s, a, b, row0 + n, n_out, out, state);
            ++n;
        }
    }
    return n;
}

// the whole wave, one triangle (s is wave-uniform): candidate c = i (n2 + 1) + j, 64 at a time
template <bool EMIT>
__device__ __forceinline__ uint32_t tri_walk_wave(const TriSetup& s, uint64_t row0, uint64_t n_out, float* __restrict__ out, uint32_t* state)
{
    const int lane = threadIdx.x & 63;
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint64_t w = (uint64_t)s.n2 + 1, cand = ((uint64_t)s.n1 + 1) * w;
    const double d1 = (double)s.n1, d2 = (double)s.n2;
    uint32_t n = 0;
    for (uint64_t base = 0; base < cand; base += 64) {
        const uint64_t c = base + lane;
        const uint64_t i = c / w, j = c - i * w;
        const double a = ((double)i + 0.5) / d1, b = ((double)j + 0.5) / d2;
        const bool ok = c < cand && a + b < 1.0;
        const uint64_t m = __ballot(ok);
        if (EMIT && ok) tri_emit(s, a, b, row0 + n + (uint32_t)__popcll(m & lt_mask), n_out, out, state);
        n += (uint32_t)__popcll(m);
    }
    return n;
}

template <bool EMIT>
__device__ __forceinline__ void meval_sample_body(const float* __restrict__ vert, const int32_t* __restrict__ faces, uint32_t V, uint32_t F, double density,
                                                  uint32_t* __restrict__ counts, uint64_t* __restrict__ blocksum, uint64_t n_out, float* __restrict__ out,
                                                  uint32_t* state)
{
    __shared__ uint64_t lds[ET / 64];
    const int lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * ET + threadIdx.x;
    const bool valid = t < F;
    TriSetup s;
    s.n1 = s.n2 = 0;
    if (valid) tri_setup(vert, faces, V, t, density, s, EMIT ? nullptr : state);
    const bool big = s.n1 != 0 && ((uint64_t)s.n1 + 1) * ((uint64_t)s.n2 + 1) > MEVAL_SMALL;
    uint64_t row0 = 0;
    if (EMIT) {
        uint64_t total;
        row0 = blocksum[blockIdx.x] + block_exclusive_scan<ET>((uint64_t)(valid ? counts[t] : 0u), &total, lds);
    }
    uint32_t n = 0;
    if (s.n1 != 0 && !big) n = tri_walk_serial<EMIT>(s, row0, n_out, out, state);
    for (uint64_t rem = __ballot(big); rem != 0ull; rem &= rem - 1) {
        const int src = __ffsll((long long)rem) - 1;
        const uint32_t tt = (uint32_t)__shfl((int)t, src, WAVE);
        TriSetup b;
        tri_setup(vert, faces, V, tt, density, b, nullptr);          // (the same arithmetic on the same inputs: the same n1, n2 in every lane)
        const uint64_t r0 = EMIT ? (uint64_t)__shfl((long long)row0, src, WAVE) : 0ull;
        const uint32_t c = tri_walk_wave<EMIT>(b, r0, n_out, out, state);
        if (lane == src) n = c;
    }
    if (!EMIT) {
        if (valid) counts[t] = n;
        uint64_t total;
        block_exclusive_scan<ET>((uint64_t)n, &total, lds);
        if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(ET) meval_sample_count_kernel(const float* __restrict__ vert, const int32_t* __restrict__ faces, uint32_t V, uint32_t F,
                                                               double density, uint32_t* __restrict__ counts, uint64_t* __restrict__ blocksum, uint32_t* state)
{
    meval_sample_body<false>(vert, faces, V, F, density, counts, blocksum, 0, nullptr, state);
}

__global__ void __launch_bounds__(ET) meval_sample_emit_kernel(const float* __restrict__ vert, const int32_t* __restrict__ faces, uint32_t V, uint32_t F,
                                                              double density, const uint32_t* __restrict__ counts, const uint64_t* __restrict__ blocksum,
                                                              uint64_t n_out, float* __restrict__ out, uint32_t* state)
{
    meval_sample_body<true>(vert, faces, V, F, density, const_cast<uint32_t*>(counts), const_cast<uint64_t*>(blocksum), n_out, out, state);
}

constexpr int SCAN_T = 1024;
// exclusive scan of x[0, n) in place by ONE workgroup (n = F / 256 words: 65 536 for a 16.7 M-face mesh); the sum goes to *total
__global__ void __launch_bounds__(SCAN_T) meval_scan_blocks_kernel(uint64_t* x, uint32_t n, uint64_t* __restrict__ total)
{
    __shared__ uint64_t part[SCAN_T];
    const uint32_t per = (n + SCAN_T - 1) / SCAN_T;
    const uint32_t b = min(n, threadIdx.x * per), e = min(n, b + per);
    uint64_t sum = 0;
    for (uint32_t i = b; i < e; ++i) sum += x[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_T; d <<= 1) {
        const uint64_t o = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += o;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - sum;
    for (uint32_t i = b; i < e; ++i) { const uint64_t v = x[i]; x[i] = run; run += v; }
    if (threadIdx.x == SCAN_T - 1) *total = part[SCAN_T - 1];
}

// ---- the hierarchy -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t meval_spread21(uint32_t v)          // bit k of v -> bit 3 k
{
    uint64_t x = v & 0x1FFFFFu;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ void __launch_bounds__(ET) meval_keys_kernel(const float* __restrict__ pts, uint32_t N, const float* __restrict__ bounds, int64_t* __restrict__ keys,
                                                        uint32_t* state)
{
    const uint32_t i = blockIdx.x * ET + threadIdx.x;
    if (i >= N) return;
    uint64_t key = 0;
    bool finite = true;
    for (int k = 0; k < 3; ++k) {
        const float p = pts[(size_t)i * 3 + k], lo = bounds[k], hi = bounds[3 + k];
        finite = finite && isfinite(p);
        const float ext = hi - lo;
        float u = ext > 0.0f ? (p - lo) / ext * 2097151.0f : 0.0f;
        u = u >= 0.0f ? (u <= 2097151.0f ? u : 2097151.0f) : 0.0f;          // (NaN -> 0)
        key |= meval_spread21((uint32_t)u) << k;
    }
    if (!finite) atomicAdd(state + IBGS_MEVAL_BAD_POINTS, 1u);
    keys[i] = (int64_t)key;
}

__global__ void __launch_bounds__(ET) meval_gather_kernel(const float* __restrict__ pts, uint32_t N, const int64_t* __restrict__ order, const int32_t* __restrict__ tag,
                                                          float4* __restrict__ sorted, uint32_t* state)
{
    const uint32_t k = blockIdx.x * ET + threadIdx.x;
    if (k >= N) return;
    const uint64_t i = (uint64_t)order[k];
    if (i >= N) {          // not a permutation: never dereferenced; a point no walk can reach, and the caller fails the call
        atomicAdd(state + IBGS_MEVAL_OVERRUN, 1u);
        sorted[k] = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), __uint_as_float(0xFFFFFFFFu));
        return;
    }
    sorted[k] = make_float4(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], __uint_as_float(tag ? (uint32_t)tag[i] : (uint32_t)i));
}

__global__ void __launch_bounds__(ET) meval_leaf_box_kernel(const float4* __restrict__ sorted, uint32_t N, float4* __restrict__ box, uint32_t n)
{
    const uint32_t node = blockIdx.x * ET + threadIdx.x;
    if (node >= n) return;
    const uint32_t b = node * LEAF, e = min(N, b + LEAF);
    float4 p = sorted[b];
    float lx = p.x, ly = p.y, lz = p.z, hx = p.x, hy = p.y, hz = p.z;
    for (uint32_t k = b + 1; k < e; ++k) {
        p = sorted[k];
        lx = fminf(lx, p.x); ly = fminf(ly, p.y); lz = fminf(lz, p.z);
        hx = fmaxf(hx, p.x); hy = fmaxf(hy, p.y); hz = fmaxf(hz, p.z);
    }
    box[(size_t)node * 2] = make_float4(lx, ly, lz, hx);
    box[(size_t)node * 2 + 1] = make_float4(hy, hz, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(ET) meval_box_kernel(const float4* __restrict__ child, uint32_t nchild, float4* __restrict__ box, uint32_t n)
{
    const uint32_t node = blockIdx.x * ET + threadIdx.x;
    if (node >= n) return;
    const uint32_t b = node * LEAF, e = min(nchild, b + LEAF);
    float4 lo = child[(size_t)b * 2], hi = child[(size_t)b * 2 + 1];
    for (uint32_t k = b + 1; k < e; ++k) {
        const float4 a = child[(size_t)k * 2], c = child[(size_t)k * 2 + 1];
        lo.x = fminf(lo.x, a.x); lo.y = fminf(lo.y, a.y); lo.z = fminf(lo.z, a.z);
        lo.w = fmaxf(lo.w, a.w); hi.x = fmaxf(hi.x, c.x); hi.y = fmaxf(hi.y, c.y);
    }
    box[(size_t)node * 2] = lo;
    box[(size_t)node * 2 + 1] = hi;
}

// ---- thinning ------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ET) meval_thin_round_kernel(MevalTree t, float radius, uint32_t* status, uint32_t* undecided /* null: do not count */)
{
    const uint32_t k = blockIdx.x * ET + threadIdx.x;
    if (k >= t.N || meval_ld(status + k) != IBGS_MEVAL_THIN_UNDECIDED) return;
    const float4 q = t.pts[k];
    const uint32_t rank = __float_as_uint(q.w);
    const float r2 = radius * radius;
    bool removed = false, blocked = false;
    meval_walk(t, q.x, q.y, q.z, [&](float lb) { return lb > r2; },
               [&](const float4& p, float d2, uint32_t pos) {
                   if (!(d2 <= r2) || __float_as_uint(p.w) >= rank) return false;          // (ranks are distinct: this skips the point itself)
                   const uint32_t s = meval_ld(status + pos);
                   if (s == IBGS_MEVAL_THIN_KEPT) { removed = true; return true; }
                   if (s == IBGS_MEVAL_THIN_UNDECIDED) blocked = true;
                   return false;
               });
    if (removed) meval_st(status + k, IBGS_MEVAL_THIN_REMOVED);
    else if (!blocked) meval_st(status + k, IBGS_MEVAL_THIN_KEPT);
    else if (undecided) atomicAdd(undecided, 1u);
}

// ---- nearest -------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ET) meval_nearest_kernel(const float* __restrict__ query, uint32_t Q, const int64_t* __restrict__ qorder, MevalTree t,
                                                           float max_dist, float* __restrict__ dist, int32_t* __restrict__ index, uint32_t* state)
{
    const uint32_t slot = blockIdx.x * ET + threadIdx.x;
    if (slot >= Q) return;
    uint64_t qi = slot;
    if (qorder) {
        qi = (uint64_t)qorder[slot];
        if (qi >= Q) { atomicAdd(state + IBGS_MEVAL_OVERRUN, 1u); return; }
    }
    const float qx = query[qi * 3], qy = query[qi * 3 + 1], qz = query[qi * 3 + 2];
    const float maxd2 = max_dist * max_dist;
    float best = maxd2;
    uint32_t bidx = 0xFFFFFFFFu;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) atomicAdd(state + IBGS_MEVAL_BAD_POINTS, 1u);
    else {
        auto take = [&](const float4& p, float d2, uint32_t) {
            const uint32_t id = __float_as_uint(p.w);
            if (d2 < best || (d2 == best && id < bidx && bidx != 0xFFFFFFFFu)) { best = d2; bidx = id; }
            return false;
        };
        // a first bound: down to the leaf whose boxes are nearest at every level
        uint32_t b = 0, e = t.n[t.L - 1];
        for (int lvl = t.L - 1; lvl >= 0; --lvl) {
            uint32_t node = b;
            float lbmin = __builtin_inff();
            for (uint32_t c = b; c < e; ++c) {
                const float lb = meval_box_d2(t.box[lvl], c, qx, qy, qz);
                if (lb < lbmin) { lbmin = lb; node = c; }
            }
            if (!(lbmin < maxd2)) { b = e = 0; break; }
            b = node * LEAF;
            e = min(lvl > 0 ? t.n[lvl - 1] : t.N, b + LEAF);
        }
        for (uint32_t k = b; k < e; ++k) { const float4 p = t.pts[k]; take(p, meval_d2(qx - p.x, qy - p.y, qz - p.z), k); }
        // the exact answer: every box that can hold a smaller d2, or an equal one with a smaller index
        meval_walk(t, qx, qy, qz, [&](float lb) { return lb > best || lb >= maxd2; }, take);
    }
    const bool found = bidx != 0xFFFFFFFFu;
    dist[qi] = found ? (float)sqrt((double)best) : __builtin_inff();          // (f64 root rounded to f32 = the correctly rounded f32 root: 53 >= 2 x 24 + 2)
    index[qi] = found ? (int32_t)bidx : -1;
}

__global__ void __launch_bounds__(ET) meval_reduce_kernel(const float* __restrict__ dist, uint32_t Q, float threshold, double* sum, unsigned long long* count)
{
    double a = 0.0;
    unsigned long long n = 0;
    for (size_t i = (size_t)blockIdx.x * ET + threadIdx.x; i < Q; i += (size_t)gridDim.x * ET) {
        const float d = dist[i];
        if (d < threshold) { a += (double)d; ++n; }
    }
    double an[2] = {a, (double)n};          // (a workgroup's count is below 2^31: exact in f64, whatever the order)
    const double v = block_reduce<ET, 2>(an, op_add());
    if (threadIdx.x == 0 && v != 0.0) atomicAdd(sum, v);          // (a sum of 0 leaves *sum as it is: no count, or distances of 0 alone)
    if (threadIdx.x == 1 && v != 0.0) atomicAdd(count, (unsigned long long)v);
}

struct SampleScratch {
    uint32_t* counts; uint64_t* blocksum; uint32_t nblocks;
    static SampleScratch carve(char* base, int64_t F, size_t* total)
    {
        SampleScratch s;
        Carver c(base);
        s.nblocks = grid_for((size_t)F, ET);
        s.counts = c.take<uint32_t>((size_t)F);
        s.blocksum = c.take<uint64_t>((size_t)s.nblocks + 1);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return s;
    }
};

static bool sample_ok(const char* who, int32_t V, int32_t F, const float* vertices, const int32_t* faces, double density, const void* scratch, size_t scratch_bytes,
                      uint32_t* state, SampleScratch* sc)
{
    if (V < 0 || F < 0 || F >= (1 << 30)) { set_error("%s: V %d / F %d out of range (0 <= V < 2^31, 0 <= F < 2^30)", who, V, F); return false; }
    if (!(density > 0.0) || !(density < 1e300)) { set_error("%s: density must be positive and finite", who); return false; }
    if ((V > 0 && !vertices) || (F > 0 && !faces) || !state || !scratch) { set_error("%s: null array", who); return false; }
    size_t need = 0;
    *sc = SampleScratch::carve(static_cast<char*>(const_cast<void*>(scratch)), F, &need);
    return arena_ok(who, "scratch", scratch, scratch_bytes, need);
}

static bool tree_ok(const char* who, int32_t N, const void* tree, size_t tree_bytes, MevalTree* t)
{
    if (N <= 0) { set_error("%s: N %d out of range (0 < N < 2^31)", who, N); return false; }
    size_t need = 0;
    *t = meval_tree_carve(static_cast<char*>(const_cast<void*>(tree)), N, &need);
    return arena_ok(who, "hierarchy", tree, tree_bytes, need);
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_meval_required_sample_scratch(int64_t F)
{
    if (F < 0 || F >= (int64_t(1) << 30)) return 0;
    size_t total = 0;
    SampleScratch::carve(nullptr, F, &total);
    return total;
}

int32_t ibgs_meval_sample_count(void* stream, int32_t V, int32_t F, const float* vertices, const int32_t* faces, double density, void* scratch,
                                size_t scratch_bytes, uint64_t* total, uint32_t* state)
{
    SampleScratch sc;
    if (!sample_ok("meval_sample_count", V, F, vertices, faces, density, scratch, scratch_bytes, state, &sc)) return -IBGS_ERR_INVALID;
    if (!total) { set_error("meval_sample_count: null total"); return -IBGS_ERR_INVALID; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (F == 0) { IBGS_HIP(hipMemsetAsync(total, 0, sizeof(uint64_t), s)); return 0; }
    hipLaunchKernelGGL(meval_sample_count_kernel, dim3(sc.nblocks), dim3(ET), 0, s, vertices, faces, (uint32_t)V, (uint32_t)F, density, sc.counts, sc.blocksum, state);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(meval_scan_blocks_kernel, dim3(1), dim3(SCAN_T), 0, s, sc.blocksum, sc.nblocks, total);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_meval_sample_emit(void* stream, int32_t V, int32_t F, const float* vertices, const int32_t* faces, double density, const void* scratch,
                               size_t scratch_bytes, int64_t n_out, float* out, uint32_t* state)
{
    SampleScratch sc;
    if (!sample_ok("meval_sample_emit", V, F, vertices, faces, density, scratch, scratch_bytes, state, &sc)) return -IBGS_ERR_INVALID;
    if (n_out < 0 || (n_out > 0 && !out)) { set_error("meval_sample_emit: bad n_out or null output"); return -IBGS_ERR_INVALID; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (F == 0 || n_out == 0) return 0;
    hipLaunchKernelGGL(meval_sample_emit_kernel, dim3(sc.nblocks), dim3(ET), 0, s, vertices, faces, (uint32_t)V, (uint32_t)F, density, sc.counts, sc.blocksum,
                       (uint64_t)n_out, out, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_meval_keys(void* stream, int32_t N, const float* points, const float* bounds, int64_t* keys, uint32_t* state)
{
    if (N < 0) { set_error("meval_keys: N %d out of range", N); return -IBGS_ERR_INVALID; }
    if (N == 0) return 0;
    if (!points || !bounds || !keys || !state) { set_error("meval_keys: null array"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(meval_keys_kernel, dim3(grid_for((size_t)N, ET)), dim3(ET), 0, reinterpret_cast<hipStream_t>(stream), points, (uint32_t)N, bounds, keys, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

size_t ibgs_meval_required_tree(int64_t N)
{
    if (N <= 0 || N >= (int64_t(1) << 31)) return 0;
    size_t total = 0;
    meval_tree_carve(nullptr, N, &total);
    return total;
}

int32_t ibgs_meval_build(void* stream, int32_t N, const float* points, const int64_t* order, const int32_t* tag, void* tree, size_t tree_bytes, uint32_t* state)
{
    MevalTree t;
    if (!tree_ok("meval_build", N, tree, tree_bytes, &t)) return -IBGS_ERR_INVALID;
    if (!points || !order || !state) { set_error("meval_build: null array"); return -IBGS_ERR_INVALID; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(meval_gather_kernel, dim3(grid_for((size_t)N, ET)), dim3(ET), 0, s, points, (uint32_t)N, order, tag, const_cast<float4*>(t.pts), state);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(meval_leaf_box_kernel, dim3(grid_for(t.n[0], ET)), dim3(ET), 0, s, t.pts, t.N, const_cast<float4*>(t.box[0]), t.n[0]);
    IBGS_HIP(hipGetLastError());
    for (int l = 1; l < t.L; ++l) {
        hipLaunchKernelGGL(meval_box_kernel, dim3(grid_for(t.n[l], ET)), dim3(ET), 0, s, t.box[l - 1], t.n[l - 1], const_cast<float4*>(t.box[l]), t.n[l]);
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

int32_t ibgs_meval_thin_rounds(void* stream, int32_t N, const void* tree, size_t tree_bytes, float radius, uint32_t* status, int32_t rounds, uint32_t* state)
{
    MevalTree t;
    if (!tree_ok("meval_thin_rounds", N, tree, tree_bytes, &t)) return -IBGS_ERR_INVALID;
    if (!status || !state) { set_error("meval_thin_rounds: null array"); return -IBGS_ERR_INVALID; }
    if (!(radius >= 0.0f) || !(radius < 1e18f) || rounds < 1 || rounds > 65536) { set_error("meval_thin_rounds: bad radius or rounds"); return -IBGS_ERR_INVALID; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IBGS_HIP(hipMemsetAsync(state + IBGS_MEVAL_UNDECIDED, 0, sizeof(uint32_t), s));
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(meval_thin_round_kernel, dim3(grid_for((size_t)N, ET)), dim3(ET), 0, s, t, radius, status,
                           r == rounds - 1 ? state + IBGS_MEVAL_UNDECIDED : nullptr);
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

int32_t ibgs_meval_nearest(void* stream, int32_t Q, const float* query, const int64_t* qorder, int32_t N, const void* tree, size_t tree_bytes,
                           float max_dist, float* dist, int32_t* index, uint32_t* state)
{
    MevalTree t;
    if (Q < 0) { set_error("meval_nearest: Q %d out of range", Q); return -IBGS_ERR_INVALID; }
    if (!tree_ok("meval_nearest", N, tree, tree_bytes, &t)) return -IBGS_ERR_INVALID;
    if (!(max_dist >= 0.0f) || !(max_dist < 1e18f)) { set_error("meval_nearest: max_dist must be finite and >= 0"); return -IBGS_ERR_INVALID; }
    if (Q == 0) return 0;
    if (!query || !dist || !index || !state) { set_error("meval_nearest: null array"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(meval_nearest_kernel, dim3(grid_for((size_t)Q, ET)), dim3(ET), 0, reinterpret_cast<hipStream_t>(stream), query, (uint32_t)Q, qorder, t, max_dist,
                       dist, index, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_meval_reduce(void* stream, int32_t Q, const float* dist, float threshold, double* sum, uint64_t* count)
{
    if (Q < 0) { set_error("meval_reduce: Q %d out of range", Q); return -IBGS_ERR_INVALID; }
    if (Q == 0) return 0;
    if (!dist || !sum || !count) { set_error("meval_reduce: null array"); return -IBGS_ERR_INVALID; }
    const unsigned g = grid_for((size_t)Q, ET);
    hipLaunchKernelGGL(meval_reduce_kernel, dim3(g < 2048u ? g : 2048u), dim3(ET), 0, reinterpret_cast<hipStream_t>(stream), dist, (uint32_t)Q, threshold, sum,
                       reinterpret_cast<unsigned long long*>(count));
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
