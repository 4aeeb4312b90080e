// Point-cloud registration on the device (C ABI: include/ibgs_registration.h; Python: ibgs_amd/registration.py): the Open3D stages of the reference's
// Tanks-and-Temples script (scripts/tnt_eval/registration.py:106-195, evaluation.py:74-91) that sit between a reconstruction and its F-score -- transform,
// crop to the scene's selection volume, voxel_down_sample, and the sums inside registration_icp with TransformationEstimationPointToPoint(True).  ICP's
// correspondence search is mesh_eval.hip's meval_nearest_kernel.  This is the project's own statement of those stages (DESIGN.md section 11,
// "Registration"); tests/registration_ref.py restates it with numpy.  Compiled with -ffp-contract=off: the operation orders below ARE the contract.
//
// CONTRACT
//   transform  T = 4 x 4 f64, last row 0 0 0 1, by value.  x' = ((T00 x + T01 y) + T02 z) + T03 in f64 from the f32 coordinates, rounded once to f32; the
//              other two rows likewise.
//   crop       SelectionPolygonVolume.crop_point_cloud.  orthogonal_axis X: (w; u, v) = (0; 1, 2), Y: (1; 0, 2), Z: (2; 0, 1).  A point is kept iff
//              axis_min <= p[w] <= axis_max and the number of crossings with node < p[u] is odd.  Edge (i, j = i + 1 mod n) crosses when
//              (v_i < p[v] and v_j >= p[v]) or (v_j < p[v] and v_i >= p[v]); node = u_i + ((p[v] - v_i) / (v_j - v_i)) (u_j - u_i).  All in f64, polygon in f64.
//              With T the point is transformed first, rounding to f32 included: crop(points, vol, T) = crop(transform(points, T), vol) bit for bit.
//   voxel      lo = per-axis minimum of the cloud (f32); origin = f64(lo) - v / 2; index = floor((f64(p) - origin) / v) per axis; key = ix << 42 | iy << 21 | iz.
//              An index above 2^21 - 1 is counted (the call fails).  Output: one point per occupied voxel IN ASCENDING KEY ORDER (Open3D's order is a hash
//              map's: a stated deviation): the f64 sum of the members divided by their number, rounded once to f32.  The restatement sums in point-index
//              order; so do the kernels for voxels of up to 64 members (the sort is stable); larger voxels are summed by a wave in a fixed tree order.
//   moments    over the queries with a correspondence, s = f32 query, t = its f32 target, pivot c (f64): n, sum(s - c), sum(t - c), sum (s - c)(t - c)^T,
//              sum |s - c|^2 with |.|^2 = (x x + y y) + z z, sum d^2 with d = s - t widened, d^2 = (dx dx + dy dy) + dz dz.  Per-workgroup partials, then one
//              workgroup (block_reduce: block_ops.h states the order of the additions); no atomics: 18 words that are the same bits on every run.
//
// KERNELS
//   pcreg_bounds_kernel / pcreg_bounds_final_kernel      per-axis min / max: workgroup partials, then one workgroup
//   pcreg_transform_kernel
//   pcreg_crop_kernel           the polygon staged once per workgroup in LDS (16 KB at 1024 vertices); a division only for an edge that crosses
//   pcreg_voxel_keys_kernel
//   pcreg_voxel_heads_kernel    marks the first sorted point of every voxel; exclusive_scan_u32 (scan_sort.hip) numbers the voxels
//   pcreg_voxel_mean_kernel     one thread per sorted point; a head walks its voxel.  Voxels of more than 64 points are walked by the whole wave afterwards,
//                               64 members at a time (ballot finds the end), so one voxel of 10^6 points costs 16 000 wave steps, not 10^6 thread steps
//   pcreg_moments_kernel / pcreg_moments_final_kernel
// Indices outside their range are never dereferenced; out-of-range conditions are counted in the state words and the caller fails the call.
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_registration.h"

namespace ibgs {

constexpr int RT = 256;                              // threads per workgroup of every kernel here
constexpr int PCREG_PARTS = 1024;                    // most workgroups of a partial-sum kernel
constexpr int NM = IBGS_PCREG_MOMENTS;

struct PcregT { double m[12]; };                     // rows 0..2 of the 4 x 4

struct PcregScratch {
    float* bpart;          // PCREG_PARTS x 6
    double* mpart;         // PCREG_PARTS x 18
    uint32_t* flag;        // N      1 = first sorted point of a voxel
    uint32_t* pos;         // N + 1  exclusive scan of flag; [N] = voxels
    uint32_t* scan; size_t scan_elems;
    static PcregScratch carve(char* base, int64_t N, size_t* total)
    {
        PcregScratch s;
        Carver c(base);
        s.bpart = c.take<float>((size_t)PCREG_PARTS * 6);          // (the fixed-size parts first: their place does not depend on N)
        s.mpart = c.take<double>((size_t)PCREG_PARTS * NM);
        s.flag = c.take<uint32_t>((size_t)N);
        s.pos = c.take<uint32_t>((size_t)N + 1);
        s.scan_elems = scan_scratch_elems((size_t)N + 1);
        s.scan = c.take<uint32_t>(s.scan_elems);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return s;
    }
};

__device__ __forceinline__ float pcreg_sel(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// stage 1 of the contract: f64 from the f32 coordinates, one rounding
__device__ __forceinline__ void pcreg_apply(const PcregT& T, float& x, float& y, float& z)
{
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    x = (float)(((T.m[0] * dx + T.m[1] * dy) + T.m[2] * dz) + T.m[3]);
    y = (float)(((T.m[4] * dx + T.m[5] * dy) + T.m[6] * dz) + T.m[7]);
    z = (float)(((T.m[8] * dx + T.m[9] * dy) + T.m[10] * dz) + T.m[11]);
}

// ---- bounds --------------------------------------------------------------------------------------------------------------------------------------
// per-axis min (components 0..2) and max (3..5): the op of block_reduce
struct PcregMinMax { __device__ __forceinline__ float operator()(float x, float y, int k) const { return k < 3 ? fminf(x, y) : fmaxf(x, y); } };

__global__ void __launch_bounds__(RT) pcreg_bounds_kernel(const float* __restrict__ pts, uint32_t N, float* __restrict__ part, uint32_t* state)
{
    const float inf = __builtin_inff();
    float b[6] = {inf, inf, inf, -inf, -inf, -inf};
    uint32_t bad = 0;
    for (size_t i = (size_t)blockIdx.x * RT + threadIdx.x; i < N; i += (size_t)gridDim.x * RT) {
        const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) { ++bad; continue; }
        b[0] = fminf(b[0], x); b[1] = fminf(b[1], y); b[2] = fminf(b[2], z);
        b[3] = fmaxf(b[3], x); b[4] = fmaxf(b[4], y); b[5] = fmaxf(b[5], z);
    }
    if (bad) atomicAdd(state + IBGS_PCREG_BAD_POINTS, bad);
    block_reduce<RT, 6>(b, part + (size_t)blockIdx.x * 6, PcregMinMax());
}

__global__ void __launch_bounds__(RT) pcreg_bounds_final_kernel(const float* __restrict__ part, uint32_t nparts, float* __restrict__ bounds)
{
    const float inf = __builtin_inff();
    float b[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (uint32_t p = threadIdx.x; p < nparts; p += RT)
        for (int k = 0; k < 6; ++k) b[k] = PcregMinMax()(b[k], part[(size_t)p * 6 + k], k);
    block_reduce<RT, 6>(b, bounds, PcregMinMax());
}

// ---- transform and crop --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RT) pcreg_transform_kernel(const float* __restrict__ pts, uint32_t N, PcregT T, float* __restrict__ out, uint32_t* state)
{
    const uint32_t i = blockIdx.x * RT + threadIdx.x;
    if (i >= N) return;
    float x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    pcreg_apply(T, x, y, z);
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicAdd(state + IBGS_PCREG_BAD_POINTS, 1u);
    out[(size_t)i * 3] = x; out[(size_t)i * 3 + 1] = y; out[(size_t)i * 3 + 2] = z;
}

__global__ void __launch_bounds__(RT) pcreg_crop_kernel(const float* __restrict__ pts, uint32_t N, PcregT T, int has_T, int w, int u, int v, double axis_min,
                                                        double axis_max, const double* __restrict__ polygon, int n_poly, uint8_t* __restrict__ mask, uint32_t* state)
{
    __shared__ double2 s_poly[IBGS_PCREG_MAX_POLYGON];          // {u, v}
    for (int k = threadIdx.x; k < n_poly; k += RT) s_poly[k] = make_double2(polygon[2 * k], polygon[2 * k + 1]);
    __syncthreads();
    const uint32_t i = blockIdx.x * RT + threadIdx.x;
    if (i >= N) return;
    float x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    if (has_T) pcreg_apply(T, x, y, z);
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) { atomicAdd(state + IBGS_PCREG_BAD_POINTS, 1u); mask[i] = 0; return; }
    const double pw = (double)pcreg_sel(x, y, z, w), pu = (double)pcreg_sel(x, y, z, u), pv = (double)pcreg_sel(x, y, z, v);
    bool in = pw >= axis_min && pw <= axis_max;
    if (in) {
        uint32_t left = 0;
        double2 a = s_poly[0];
        for (int e = 0; e < n_poly; ++e) {
            const double2 b = s_poly[e + 1 == n_poly ? 0 : e + 1];
            if ((a.y < pv && b.y >= pv) || (b.y < pv && a.y >= pv)) {
                const double node = a.x + ((pv - a.y) / (b.y - a.y)) * (b.x - a.x);
                if (node < pu) ++left;
            }
            a = b;
        }
        in = (left & 1u) != 0u;
    }
    mask[i] = in ? 1 : 0;
}

// ---- voxel thinning ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RT) pcreg_voxel_keys_kernel(const float* __restrict__ pts, uint32_t N, const float* __restrict__ bounds, double voxel,
                                                              int64_t* __restrict__ keys, uint32_t* state)
{
    const uint32_t i = blockIdx.x * RT + threadIdx.x;
    if (i >= N) return;
    uint64_t key = 0;
    bool finite = true, fits = true;
    for (int k = 0; k < 3; ++k) {
        const float p = pts[(size_t)i * 3 + k];
        finite = finite && isfinite(p);
        const double origin = (double)bounds[k] - voxel / 2;
        const double idx = floor(((double)p - origin) / voxel);
        if (!(idx >= 0.0 && idx <= (double)IBGS_PCREG_MAX_INDEX)) { fits = false; continue; }          // (NaN lands here too)
        key = key << 21 | (uint64_t)idx;
    }
    if (!finite) atomicAdd(state + IBGS_PCREG_BAD_POINTS, 1u);
    else if (!fits) atomicAdd(state + IBGS_PCREG_KEY_OVERFLOW, 1u);
    keys[i] = finite && fits ? (int64_t)key : INT64_MAX;
}

__global__ void __launch_bounds__(RT) pcreg_voxel_heads_kernel(const int64_t* __restrict__ keys, uint32_t N, uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * RT + threadIdx.x;
    if (i >= N) return;
    flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

struct PcregSum { double x, y, z; uint32_t n; };

__device__ __forceinline__ void pcreg_add_member(PcregSum& a, const float* __restrict__ pts, const int64_t* __restrict__ order, uint32_t N, uint32_t k, uint32_t* state)
{
    const uint64_t i = (uint64_t)order[k];
    if (i >= N) { atomicAdd(state + IBGS_PCREG_BAD_INDEX, 1u); return; }
    a.x += (double)pts[i * 3]; a.y += (double)pts[i * 3 + 1]; a.z += (double)pts[i * 3 + 2];
    ++a.n;
}

__device__ __forceinline__ void pcreg_write_mean(const PcregSum& a, uint32_t seg, uint32_t M, int64_t key, float* __restrict__ out, int64_t* __restrict__ out_keys,
                                                 uint32_t* state)
{
    if (seg >= M) { atomicAdd(state + IBGS_PCREG_OVERRUN, 1u); return; }
    const double n = (double)a.n;
    out[(size_t)seg * 3] = (float)(a.x / n); out[(size_t)seg * 3 + 1] = (float)(a.y / n); out[(size_t)seg * 3 + 2] = (float)(a.z / n);
    if (out_keys) out_keys[seg] = key;
}

__global__ void __launch_bounds__(RT) pcreg_voxel_mean_kernel(const float* __restrict__ pts, uint32_t N, const int64_t* __restrict__ order,
                                                              const int64_t* __restrict__ keys, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                              uint32_t M, float* __restrict__ out, int64_t* __restrict__ out_keys, uint32_t* state)
{
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * RT + threadIdx.x;
    const bool head = i < N && flag[i] != 0u;          // (no early return: the whole wave takes part in the ballots below)
    const uint32_t seg = head ? pos[i] : 0u;
    bool big = false;
    if (head) {
        PcregSum a = {0.0, 0.0, 0.0, 0u};
        uint32_t walked = 0;
        for (uint32_t k = i; k < N && (k == i || flag[k] == 0u); ++k) {
            if (walked == IBGS_PCREG_LONG_SEGMENT) { big = true; break; }
            pcreg_add_member(a, pts, order, N, k, state);          // sorted order = index order inside a voxel (stable sort)
            ++walked;
        }
        if (!big && a.n) pcreg_write_mean(a, seg, M, keys[i], out, out_keys, state);
    }
    for (uint64_t rem = __ballot(big); rem != 0ull; rem &= rem - 1) {
        const int src = __ffsll((long long)rem) - 1;
        const uint32_t start = (uint32_t)__shfl((int)i, src, WAVE), sg = (uint32_t)__shfl((int)seg, src, WAVE);
        PcregSum a = {0.0, 0.0, 0.0, 0u};
        for (uint64_t base = start;; base += 64) {
            const uint64_t k = base + lane;
            const bool in = k < N && (k == start || flag[k] == 0u);
            const uint64_t stop = __ballot(!in);
            const int first = stop ? __ffsll((long long)stop) - 1 : 64;
            if (lane < first) pcreg_add_member(a, pts, order, N, (uint32_t)k, state);
            if (stop) break;
        }
        a.x = wave_reduce(a.x, op_add()); a.y = wave_reduce(a.y, op_add()); a.z = wave_reduce(a.z, op_add());          // a fixed tree: the same bits on every run
        a.n = wave_reduce(a.n, op_add());
        if (lane == 0 && a.n) pcreg_write_mean(a, sg, M, keys[start], out, out_keys, state);
    }
}

// ---- moments -------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RT) pcreg_moments_kernel(const float* __restrict__ query, const int32_t* __restrict__ index, uint32_t Q,
                                                           const float* __restrict__ target, uint32_t N, double cx, double cy, double cz,
                                                           double* __restrict__ part, uint32_t* state)
{
    double a[NM];
    for (int k = 0; k < NM; ++k) a[k] = 0.0;
    for (size_t i = (size_t)blockIdx.x * RT + threadIdx.x; i < Q; i += (size_t)gridDim.x * RT) {
        const int32_t j = index[i];
        if (j < 0) continue;
        if ((uint32_t)j >= N) { atomicAdd(state + IBGS_PCREG_BAD_INDEX, 1u); continue; }
        const double s[3] = {(double)query[i * 3], (double)query[i * 3 + 1], (double)query[i * 3 + 2]};
        const double t[3] = {(double)target[(size_t)j * 3], (double)target[(size_t)j * 3 + 1], (double)target[(size_t)j * 3 + 2]};
        const double sc[3] = {s[0] - cx, s[1] - cy, s[2] - cz}, tc[3] = {t[0] - cx, t[1] - cy, t[2] - cz};
        const double dx = s[0] - t[0], dy = s[1] - t[1], dz = s[2] - t[2];
        a[0] += 1.0;
        for (int r = 0; r < 3; ++r) {
            a[1 + r] += sc[r];
            a[4 + r] += tc[r];
            for (int c = 0; c < 3; ++c) a[7 + 3 * r + c] += sc[r] * tc[c];
        }
        a[16] += (sc[0] * sc[0] + sc[1] * sc[1]) + sc[2] * sc[2];
        a[17] += (dx * dx + dy * dy) + dz * dz;
    }
    block_reduce<RT, NM>(a, part + (size_t)blockIdx.x * NM, op_add());          // (block_ops.h states the order of this sum)
}

__global__ void __launch_bounds__(RT) pcreg_moments_final_kernel(const double* __restrict__ part, uint32_t nparts, double* __restrict__ out)
{
    double a[NM];
    for (int k = 0; k < NM; ++k) a[k] = 0.0;
    for (uint32_t b = threadIdx.x; b < nparts; b += RT)
        for (int k = 0; k < NM; ++k) a[k] += part[(size_t)b * NM + k];
    block_reduce<RT, NM>(a, out, op_add());
}

static inline unsigned pcreg_parts(size_t n) { const unsigned g = grid_for(n, RT); return g < (unsigned)PCREG_PARTS ? g : (unsigned)PCREG_PARTS; }

static bool scratch_ok(const char* who, int32_t N, const void* scratch, size_t scratch_bytes, PcregScratch* sc)
{
    size_t need = 0;
    *sc = PcregScratch::carve(static_cast<char*>(const_cast<void*>(scratch)), N, &need);
    return arena_ok(who, "scratch", scratch, scratch_bytes, need);
}

static bool transform_ok(const char* who, const double* host_T, PcregT* T)
{
    for (int k = 0; k < 16; ++k)
        if (!(host_T[k] - host_T[k] == 0.0)) { set_error("%s: T holds a non-finite entry", who); return false; }
    if (host_T[12] != 0.0 || host_T[13] != 0.0 || host_T[14] != 0.0 || host_T[15] != 1.0) { set_error("%s: the last row of T must be 0 0 0 1", who); return false; }
    for (int k = 0; k < 12; ++k) T->m[k] = host_T[k];
    return true;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_pcreg_required_scratch(int64_t N)
{
    if (N < 0 || N >= (int64_t(1) << 31)) return 0;
    size_t total = 0;
    PcregScratch::carve(nullptr, N, &total);
    return total;
}

int32_t ibgs_pcreg_bounds(void* stream, int32_t N, const float* points, void* scratch, size_t scratch_bytes, float* bounds, uint32_t* state)
{
    PcregScratch sc;
    if (N <= 0) { set_error("pcreg_bounds: N %d out of range (0 < N < 2^31)", N); return -IBGS_ERR_INVALID; }
    if (!points || !bounds || !state) { set_error("pcreg_bounds: null array"); return -IBGS_ERR_INVALID; }
    if (!scratch_ok("pcreg_bounds", N, scratch, scratch_bytes, &sc)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned g = pcreg_parts((size_t)N);
    hipLaunchKernelGGL(pcreg_bounds_kernel, dim3(g), dim3(RT), 0, s, points, (uint32_t)N, sc.bpart, state);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(pcreg_bounds_final_kernel, dim3(1), dim3(RT), 0, s, sc.bpart, g, bounds);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_pcreg_transform(void* stream, int32_t N, const float* points, const double* host_T, float* out, uint32_t* state)
{
    PcregT T;
    if (N < 0) { set_error("pcreg_transform: N %d out of range", N); return -IBGS_ERR_INVALID; }
    if (!host_T) { set_error("pcreg_transform: null T"); return -IBGS_ERR_INVALID; }
    if (!transform_ok("pcreg_transform", host_T, &T)) return -IBGS_ERR_INVALID;
    if (N == 0) return 0;
    if (!points || !out || !state) { set_error("pcreg_transform: null array"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(pcreg_transform_kernel, dim3(grid_for((size_t)N, RT)), dim3(RT), 0, reinterpret_cast<hipStream_t>(stream), points, (uint32_t)N, T, out, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_pcreg_crop(void* stream, int32_t N, const float* points, const double* host_T, int32_t axis, double axis_min, double axis_max, int32_t n_poly,
                        const double* polygon, uint8_t* mask, uint32_t* state)
{
    PcregT T = {};
    if (N < 0) { set_error("pcreg_crop: N %d out of range", N); return -IBGS_ERR_INVALID; }
    if (axis < 0 || axis > 2) { set_error("pcreg_crop: axis %d is not 0, 1 or 2", axis); return -IBGS_ERR_INVALID; }
    if (n_poly < 3 || n_poly > IBGS_PCREG_MAX_POLYGON) { set_error("pcreg_crop: a polygon of %d vertices (3 .. %d)", n_poly, IBGS_PCREG_MAX_POLYGON); return -IBGS_ERR_INVALID; }
    if (!(axis_min <= axis_max)) { set_error("pcreg_crop: axis_min must not exceed axis_max"); return -IBGS_ERR_INVALID; }
    if (host_T && !transform_ok("pcreg_crop", host_T, &T)) return -IBGS_ERR_INVALID;
    if (N == 0) return 0;
    if (!points || !polygon || !mask || !state) { set_error("pcreg_crop: null array"); return -IBGS_ERR_INVALID; }
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
    hipLaunchKernelGGL(pcreg_crop_kernel, dim3(grid_for((size_t)N, RT)), dim3(RT), 0, reinterpret_cast<hipStream_t>(stream), points, (uint32_t)N, T, host_T ? 1 : 0,
                       (int)axis, u, v, axis_min, axis_max, polygon, (int)n_poly, mask, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_pcreg_voxel_keys(void* stream, int32_t N, const float* points, const float* bounds, double voxel, int64_t* keys, uint32_t* state)
{
    if (N < 0) { set_error("pcreg_voxel_keys: N %d out of range", N); return -IBGS_ERR_INVALID; }
    if (!(voxel > 0.0) || !(voxel < 1e300)) { set_error("pcreg_voxel_keys: voxel must be positive and finite"); return -IBGS_ERR_INVALID; }
    if (N == 0) return 0;
    if (!points || !bounds || !keys || !state) { set_error("pcreg_voxel_keys: null array"); return -IBGS_ERR_INVALID; }
    hipLaunchKernelGGL(pcreg_voxel_keys_kernel, dim3(grid_for((size_t)N, RT)), dim3(RT), 0, reinterpret_cast<hipStream_t>(stream), points, (uint32_t)N, bounds, voxel,
                       keys, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_pcreg_voxel_count(void* stream, int32_t N, const int64_t* sorted_keys, void* scratch, size_t scratch_bytes, uint32_t* total, uint32_t* state)
{
    PcregScratch sc;
    if (N <= 0) { set_error("pcreg_voxel_count: N %d out of range (0 < N < 2^31)", N); return -IBGS_ERR_INVALID; }
    if (!sorted_keys || !total || !state) { set_error("pcreg_voxel_count: null array"); return -IBGS_ERR_INVALID; }
    if (!scratch_ok("pcreg_voxel_count", N, scratch, scratch_bytes, &sc)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pcreg_voxel_heads_kernel, dim3(grid_for((size_t)N, RT)), dim3(RT), 0, s, sorted_keys, (uint32_t)N, sc.flag);
    IBGS_HIP(hipGetLastError());
    const int rc = exclusive_scan_u32(s, sc.flag, sc.pos, (size_t)N, sc.scan, sc.scan_elems, true);
    if (rc) return rc;
    IBGS_HIP(hipMemcpyAsync(total, sc.pos + N, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return 0;
}

int32_t ibgs_pcreg_voxel_emit(void* stream, int32_t N, const float* points, const int64_t* order, const int64_t* sorted_keys, const void* scratch,
                              size_t scratch_bytes, int32_t M, float* out, int64_t* out_keys, uint32_t* state)
{
    PcregScratch sc;
    if (N <= 0 || M < 0 || M > N) { set_error("pcreg_voxel_emit: N %d / M %d out of range (0 < N < 2^31, 0 <= M <= N)", N, M); return -IBGS_ERR_INVALID; }
    if (!points || !order || !sorted_keys || !state || (M > 0 && !out)) { set_error("pcreg_voxel_emit: null array"); return -IBGS_ERR_INVALID; }
    if (!scratch_ok("pcreg_voxel_emit", N, scratch, scratch_bytes, &sc)) return -IBGS_ERR_INVALID;
    if (M == 0) return 0;
    hipLaunchKernelGGL(pcreg_voxel_mean_kernel, dim3(grid_for((size_t)N, RT)), dim3(RT), 0, reinterpret_cast<hipStream_t>(stream), points, (uint32_t)N, order, sorted_keys,
                       sc.flag, sc.pos, (uint32_t)M, out, out_keys, state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_pcreg_moments(void* stream, int32_t Q, const float* query, const int32_t* index, int32_t N, const float* target, const double* host_pivot,
                           void* scratch, size_t scratch_bytes, double* out, uint32_t* state)
{
    PcregScratch sc;
    if (Q <= 0 || N <= 0) { set_error("pcreg_moments: Q %d / N %d out of range (0 < Q, N < 2^31)", Q, N); return -IBGS_ERR_INVALID; }
    if (!query || !index || !target || !host_pivot || !out || !state) { set_error("pcreg_moments: null array"); return -IBGS_ERR_INVALID; }
    for (int k = 0; k < 3; ++k)
        if (!(host_pivot[k] - host_pivot[k] == 0.0)) { set_error("pcreg_moments: the pivot must be finite"); return -IBGS_ERR_INVALID; }
    if (!scratch_ok("pcreg_moments", 0, scratch, scratch_bytes, &sc)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned g = pcreg_parts((size_t)Q);
    hipLaunchKernelGGL(pcreg_moments_kernel, dim3(g), dim3(RT), 0, s, query, index, (uint32_t)Q, target, (uint32_t)N, host_pivot[0], host_pivot[1], host_pivot[2],
                       sc.mpart, state);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(pcreg_moments_final_kernel, dim3(1), dim3(RT), 0, s, sc.mpart, g, out);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
