// The exposure correction of the colour aggregation network (include/ibgs_exposure.h; the reference's compute_exposure_affine_matrix,
// color_aggregation_network.py:136-153, 182-185): a 3 x 4 affine colour map fitted by least squares on the pixels of use_first_src_frame_mask, and that map
// applied to the rendered image.  The contract is a tolerance against a float64 restatement (tests/exposure_ref.py): no contraction
// flag -- the moments add products of two f32 values in f64, which are exact, so their bits depend on the order of the additions alone, and the
// application is an f32 fma chain.
//
// KERNELS
//   expo_moments_kernel  a capped grid (IBGS_EXPO_MAX_GROUPS x IBGS_EXPO_THREADS) walks the frame in quads of 4 consecutive pixels, one quad per thread and
//                        step: seven 16-byte loads (3 render planes, 3 warped planes, the mask) where the planes allow them, the same quads through 4-byte
//                        loads where they do not -- the same additions in the same order either way.  22 f64 sums per thread; block_reduce; one partial
//                        per workgroup.  Masked-out pixels are skipped by a branch, not by a factor 0.
//   expo_solve_kernel    one workgroup: the partials into LDS with one load wave, 22 threads add them in index order, thread 0 solves the 4 x 4 system
//                        in registers.
//   expo_apply_kernel    the element-wise application (forward: rows of A and the offset; backward: columns of its 3 x 3 block), 3 planes in, 3 out.
// What bounds them: DESIGN.md section 18 (profiles/exposure.txt).
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_exposure.h"

namespace ibgs {

constexpr int ET = IBGS_EXPO_THREADS;
constexpr int ES = IBGS_EXPO_SUMS;
constexpr int EQ = IBGS_EXPO_PIXELS_PER_THREAD;
constexpr int EXPO_APPLY_MAX_GROUPS = 2048;
static_assert(EQ == 4 && ES == 22 && ET % 64 == 0, "the quad loads and the layout of the sums below");
static_assert((size_t)IBGS_EXPO_MAX_GROUPS * ES * sizeof(double) <= 48 * 1024 && (IBGS_EXPO_MAX_GROUPS * ES) % ET == 0, "the solve kernel keeps every partial in LDS, a whole number per thread");

// the sums: [0] n, [1..3] r, [4..9] r r^T (00 01 02 11 12 22), [10..12] s, [13 + 3 i + j] s_i r_j
__device__ __forceinline__ void expo_accumulate(double (&a)[ES], float r0, float r1, float r2, float s0, float s1, float s2)
{
    const double x0 = r0, x1 = r1, x2 = r2, y0 = s0, y1 = s1, y2 = s2;
    a[0] += 1.0;
    a[1] += x0; a[2] += x1; a[3] += x2;
    a[4] += x0 * x0; a[5] += x0 * x1; a[6] += x0 * x2; a[7] += x1 * x1; a[8] += x1 * x2; a[9] += x2 * x2;
    a[10] += y0; a[11] += y1; a[12] += y2;
    a[13] += y0 * x0; a[14] += y0 * x1; a[15] += y0 * x2;
    a[16] += y1 * x0; a[17] += y1 * x1; a[18] += y1 * x2;
    a[19] += y2 * x0; a[20] += y2 * x1; a[21] += y2 * x2;
}

// VEC: plane % 4 == 0 and the three base pointers are 16-byte aligned.  Thread t of the grid takes the quads t, t + grid threads, ... and the pixels of a
// quad in order: the order of its additions, whichever way the quad was loaded.  A pixel outside the mask is skipped by a branch: its values meet no arithmetic.
template <bool VEC>
__global__ void __launch_bounds__(ET) expo_moments_kernel(const float* __restrict__ render, const float* __restrict__ warped, const int32_t* __restrict__ mask, size_t plane,
                                                          size_t quads, double* __restrict__ partials)
{
    double a[ES];
#pragma unroll
    for (int k = 0; k < ES; ++k) a[k] = 0.0;
    const size_t stride = (size_t)gridDim.x * ET;
    for (size_t q = (size_t)blockIdx.x * ET + threadIdx.x; q < quads; q += stride) {
        const size_t p = q * EQ;
        if (VEC) {
            const int4 m = *reinterpret_cast<const int4*>(mask + p);
            const float4 r0 = *reinterpret_cast<const float4*>(render + p), r1 = *reinterpret_cast<const float4*>(render + plane + p),
                         r2 = *reinterpret_cast<const float4*>(render + 2 * plane + p);
            const float4 s0 = *reinterpret_cast<const float4*>(warped + p), s1 = *reinterpret_cast<const float4*>(warped + plane + p),
                         s2 = *reinterpret_cast<const float4*>(warped + 2 * plane + p);
            if (m.x == 1) expo_accumulate(a, r0.x, r1.x, r2.x, s0.x, s1.x, s2.x);
            if (m.y == 1) expo_accumulate(a, r0.y, r1.y, r2.y, s0.y, s1.y, s2.y);
            if (m.z == 1) expo_accumulate(a, r0.z, r1.z, r2.z, s0.z, s1.z, s2.z);
            if (m.w == 1) expo_accumulate(a, r0.w, r1.w, r2.w, s0.w, s1.w, s2.w);
        } else {
#pragma unroll
            for (int k = 0; k < EQ; ++k) {
                const size_t e = p + k;
                if (e < plane && mask[e] == 1)
                    expo_accumulate(a, render[e], render[plane + e], render[2 * plane + e], warped[e], warped[plane + e], warped[2 * plane + e]);
            }
        }
    }
    block_reduce<ET, ES>(a, partials + (size_t)blockIdx.x * ES, op_add());
}

// Row p of a 4 x 7 matrix kept in registers, p known only at run time: selects over the four rows (no indexed access, which would live in scratch or LDS).
__device__ __forceinline__ double expo_pick(int p, double v0, double v1, double v2, double v3) { return p == 0 ? v0 : p == 1 ? v1 : p == 2 ? v2 : v3; }

__global__ void __launch_bounds__(ET) expo_solve_kernel(const double* __restrict__ partials, int groups, float* __restrict__ affine, int32_t* __restrict__ status)
{
    __shared__ double s_part[IBGS_EXPO_MAX_GROUPS * ES];
    __shared__ double s_sum[ES];
    // every load of the partials is issued before the first is awaited: one memory latency, not one per round of the workgroup
    const int total = groups * ES;
    double v[IBGS_EXPO_MAX_GROUPS * ES / ET];
#pragma unroll
    for (int i = 0; i < IBGS_EXPO_MAX_GROUPS * ES / ET; ++i) {
        const int e = i * ET + threadIdx.x;
        v[i] = e < total ? partials[e] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < IBGS_EXPO_MAX_GROUPS * ES / ET; ++i) {
        const int e = i * ET + threadIdx.x;
        if (e < total) s_part[e] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < ES) {
        double v = s_part[threadIdx.x];
#pragma unroll 16          // (the reads of a batch are issued together; the additions stay in index order)
        for (int g = 1; g < groups; ++g) v += s_part[g * ES + threadIdx.x];
        s_sum[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double S[ES];
#pragma unroll
    for (int k = 0; k < ES; ++k) S[k] = s_sum[k];
    const double n = S[0];
    // columns of the design matrix: r0, r1, r2, 1
    const double gram[4][4] = {{S[4], S[5], S[6], S[1]}, {S[5], S[7], S[8], S[2]}, {S[6], S[8], S[9], S[3]}, {S[1], S[2], S[3], n}};
    const double rhs[3][4] = {{S[13], S[14], S[15], S[10]}, {S[16], S[17], S[18], S[11]}, {S[19], S[20], S[21], S[12]}};
    bool ok = n >= 4.0;
    double d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double g = gram[j][j];
        if (!(g > 0.0 && g < __builtin_inf())) ok = false;          // a zero column, or a NaN / Inf under the mask
        d[j] = ok ? 1.0 / sqrt(g) : 0.0;
    }
    // M = [unit-diagonal Gram matrix | three right-hand sides], in registers.  Gauss-Jordan with DIAGONAL pivoting and no exchanges: each step takes the
    // largest diagonal entry among the rows not yet used (the lowest index among equals) -- on those rows the matrix is the Schur complement an
    // elimination with exchanges would hold -- and clears its column from every other row.  After four steps row j holds M[j][j] x_j = M[j][4 + i].
    double M[4][7];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) M[j][k] = j == k ? 1.0 : gram[j][k] * d[j] * d[k];
#pragma unroll
        for (int i = 0; i < 3; ++i) M[j][4 + i] = rhs[i][j] * d[j];
    }
    int used = 0;
#pragma unroll
    for (int step = 0; step < 4; ++step) {
        int p = -1;
        double best = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!((used >> j) & 1) && (p < 0 || M[j][j] > best)) { best = M[j][j]; p = j; }
        if (!(best > IBGS_EXPO_PIVOT_MIN)) ok = false;          // (NaN included; the steps go on, their result is dropped)
        used |= 1 << p;
        double row[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) row[c] = expo_pick(p, M[0][c], M[1][c], M[2][c], M[3][c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double f = expo_pick(p, M[j][0], M[j][1], M[j][2], M[j][3]) / best;
#pragma unroll
            for (int c = 0; c < 7; ++c) M[j][c] = j == p ? M[j][c] : M[j][c] - f * row[c];
        }
    }
    float out[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = M[j][4 + i] / M[j][j] * d[j];
            if (!(fabs(v) < __builtin_inf())) ok = false;          // a NaN / Inf among the warped colours under the mask
            out[i][j] = (float)v;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) affine[i * 4 + j] = ok ? out[i][j] : (i == j ? 1.0f : 0.0f);
    *status = ok ? 1 : 0;
}

template <bool BWD>
__device__ __forceinline__ float expo_map(const float (&c)[4], float x0, float x1, float x2)
{
    float v = BWD ? c[0] * x0 : fmaf(c[0], x0, c[3]);
    v = fmaf(c[1], x1, v);
    return fmaf(c[2], x2, v);
}

// VEC: plane % 4 == 0 and both base pointers are 16-byte aligned
template <bool BWD, bool VEC>
__global__ void __launch_bounds__(ET) expo_apply_kernel(const float* __restrict__ affine, const int32_t* __restrict__ status, const float* __restrict__ in, float* __restrict__ out,
                                                        size_t plane, size_t quads)
{
    const bool identity = *status == 0;
    float c[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i][j] = BWD ? affine[j * 4 + i] : affine[i * 4 + j];
        c[i][3] = BWD ? 0.0f : affine[i * 4 + 3];
    }
    const size_t stride = (size_t)gridDim.x * ET;
    for (size_t q = (size_t)blockIdx.x * ET + threadIdx.x; q < quads; q += stride) {
        const size_t p = q * EQ;
        if (VEC) {
            const float4 x0 = *reinterpret_cast<const float4*>(in + p), x1 = *reinterpret_cast<const float4*>(in + plane + p), x2 = *reinterpret_cast<const float4*>(in + 2 * plane + p);
            float4 y0 = x0, y1 = x1, y2 = x2;
            if (!identity) {
                y0 = make_float4(expo_map<BWD>(c[0], x0.x, x1.x, x2.x), expo_map<BWD>(c[0], x0.y, x1.y, x2.y), expo_map<BWD>(c[0], x0.z, x1.z, x2.z), expo_map<BWD>(c[0], x0.w, x1.w, x2.w));
                y1 = make_float4(expo_map<BWD>(c[1], x0.x, x1.x, x2.x), expo_map<BWD>(c[1], x0.y, x1.y, x2.y), expo_map<BWD>(c[1], x0.z, x1.z, x2.z), expo_map<BWD>(c[1], x0.w, x1.w, x2.w));
                y2 = make_float4(expo_map<BWD>(c[2], x0.x, x1.x, x2.x), expo_map<BWD>(c[2], x0.y, x1.y, x2.y), expo_map<BWD>(c[2], x0.z, x1.z, x2.z), expo_map<BWD>(c[2], x0.w, x1.w, x2.w));
            }
            *reinterpret_cast<float4*>(out + p) = y0;
            *reinterpret_cast<float4*>(out + plane + p) = y1;
            *reinterpret_cast<float4*>(out + 2 * plane + p) = y2;
        } else {
#pragma unroll
            for (int k = 0; k < EQ; ++k) {
                const size_t e = p + k;
                if (e >= plane) break;
                const float x0 = in[e], x1 = in[plane + e], x2 = in[2 * plane + e];
                out[e] = identity ? x0 : expo_map<BWD>(c[0], x0, x1, x2);
                out[plane + e] = identity ? x1 : expo_map<BWD>(c[1], x0, x1, x2);
                out[2 * plane + e] = identity ? x2 : expo_map<BWD>(c[2], x0, x1, x2);
            }
        }
    }
}

// who == nullptr: silent (the size query)
static bool expo_shape_ok(const char* who, int64_t H, int64_t W, size_t* plane, size_t* quads)
{
    if (H < 1 || W < 1 || H > IBGS_EXPO_MAX_SIDE || W > IBGS_EXPO_MAX_SIDE) {
        if (who) set_error("%s: a frame of %lld x %lld is out of range (sides 1 .. %d)", who, (long long)H, (long long)W, IBGS_EXPO_MAX_SIDE);
        return false;
    }
    *plane = (size_t)H * (size_t)W;
    *quads = (*plane + EQ - 1) / EQ;
    return true;
}

static unsigned expo_groups(size_t quads, int cap)
{
    const size_t g = (quads + ET - 1) / ET;
    return (unsigned)(g < (size_t)cap ? g : (size_t)cap);
}

static bool expo_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool BWD>
static int32_t expo_apply(const char* who, void* stream, int32_t H, int32_t W, const float* affine, const int32_t* status, const float* in, float* out)
{
    size_t plane = 0, quads = 0;
    if (!expo_shape_ok(who, H, W, &plane, &quads)) return -IBGS_ERR_INVALID;
    if (!affine || !status) { set_error("%s: null affine or status: the device words of expo_fit are required", who); return -IBGS_ERR_INVALID; }
    if (!in) { set_error("%s: null image", who); return -IBGS_ERR_INVALID; }
    if (!out) { set_error("%s: null outputs", who); return -IBGS_ERR_INVALID; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned groups = expo_groups(quads, EXPO_APPLY_MAX_GROUPS);
    if (plane % EQ == 0 && expo_aligned16(in) && expo_aligned16(out))
        hipLaunchKernelGGL((expo_apply_kernel<BWD, true>), dim3(groups), dim3(ET), 0, st, affine, status, in, out, plane, quads);
    else
        hipLaunchKernelGGL((expo_apply_kernel<BWD, false>), dim3(groups), dim3(ET), 0, st, affine, status, in, out, plane, quads);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_expo_required_scratch(int64_t H, int64_t W)
{
    size_t plane = 0, quads = 0;
    if (!expo_shape_ok(nullptr, H, W, &plane, &quads)) return 0;
    Carver c(nullptr);
    c.take<double>((size_t)expo_groups(quads, IBGS_EXPO_MAX_GROUPS) * ES);
    return c.cur + 128;
}

int32_t ibgs_expo_fit(void* stream, int32_t H, int32_t W, const float* render, const float* warped, const int32_t* mask, float* affine_out, int32_t* status_out,
                      void* scratch, size_t scratch_bytes, int32_t phases)
{
    size_t plane = 0, quads = 0;
    if (!expo_shape_ok("expo_fit", H, W, &plane, &quads)) return -IBGS_ERR_INVALID;
    if (phases < 1 || phases > IBGS_EXPO_FIT) { set_error("expo_fit: phases %d is none of IBGS_EXPO_MOMENTS, IBGS_EXPO_SOLVE, IBGS_EXPO_FIT", phases); return -IBGS_ERR_INVALID; }
    const bool moments = phases & IBGS_EXPO_MOMENTS, solve = phases & IBGS_EXPO_SOLVE;
    if (moments && (!render || !warped || !mask)) { set_error("expo_fit: null image"); return -IBGS_ERR_INVALID; }
    if (solve && (!affine_out || !status_out)) { set_error("expo_fit: null outputs: affine_out and status_out are required"); return -IBGS_ERR_INVALID; }
    const unsigned groups = expo_groups(quads, IBGS_EXPO_MAX_GROUPS);
    Carver c(static_cast<char*>(scratch));
    double* partials = c.take<double>((size_t)groups * ES);
    if (!arena_ok("expo_fit", "scratch", scratch, scratch_bytes, c.cur - reinterpret_cast<uintptr_t>(scratch) + 128)) return -IBGS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (moments) {
        if (plane % EQ == 0 && expo_aligned16(render) && expo_aligned16(warped) && expo_aligned16(mask))
            hipLaunchKernelGGL((expo_moments_kernel<true>), dim3(groups), dim3(ET), 0, st, render, warped, mask, plane, quads, partials);
        else
            hipLaunchKernelGGL((expo_moments_kernel<false>), dim3(groups), dim3(ET), 0, st, render, warped, mask, plane, quads, partials);
        IBGS_HIP(hipGetLastError());
    }
    if (solve) {
        hipLaunchKernelGGL(expo_solve_kernel, dim3(1), dim3(ET), 0, st, partials, (int)groups, affine_out, status_out);
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

int32_t ibgs_expo_apply(void* stream, int32_t H, int32_t W, const float* affine, const int32_t* status, const float* image, float* out)
{
    return expo_apply<false>("expo_apply", stream, H, W, affine, status, image, out);
}

int32_t ibgs_expo_apply_backward(void* stream, int32_t H, int32_t W, const float* affine, const int32_t* status, const float* grad_out, float* grad_image)
{
    return expo_apply<true>("expo_apply_backward", stream, H, W, affine, status, grad_out, grad_image);
}

}  // extern "C"
