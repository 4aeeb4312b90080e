// The workgroup helpers of ibgs_amd/csrc/block_ops.h against host restatements, one workgroup per case:
//   block_reduce<256, 18> on doubles   the device's 18 words must equal, BIT FOR BIT, the host's walk of the stated tree (xor steps 32 .. 1 inside each wave,
//                                      then the waves 0, 1, 2, 3 in order).  The table spans 2^-30 .. 2^30 with mixed signs, and the program refuses to pass
//                                      unless the plain index-order sum differs in bits from the tree sum for at least 12 of the 18 components: the input can
//                                      tell the orders apart.  This is what pins the order of registration.hip's moments.
//   block_reduce<256, 6>               min of components 0..2, max of 3..5, +-inf in some lanes
//   wave_reduce                        the result is in every lane
//   block_exclusive_scan               (256, uint64_t), (512, int), (256, uint32_t): every thread's prefix and total against a host loop
// Build + run: hipcc --offload-arch=gfx950 -O2 -I ibgs_amd/csrc -o /tmp/tbo tests/csrc/test_block_ops.hip && /tmp/tbo   (prints "block ops ok")
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "block_ops.h"

using namespace ibgs;

#define CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { printf("%s failed: %s\n", #expr, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int RN = 256;          // threads of the reduce cases
constexpr int NM = 18;

struct MinMax { __device__ __forceinline__ float operator()(float x, float y, int k) const { return k < 3 ? fminf(x, y) : fmaxf(x, y); } };

template <int N, typename T, typename Op>
__global__ void __launch_bounds__(RN) reduce_kernel(const T* __restrict__ in /* RN x N */, T* __restrict__ out /* N */)
{
    T a[N];
    for (int k = 0; k < N; ++k) a[k] = in[threadIdx.x * N + k];
    block_reduce<RN, N>(a, out, Op());
}

__global__ void __launch_bounds__(RN) wave_sum_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out)
{
    out[threadIdx.x] = wave_reduce(in[threadIdx.x], op_add());
}

template <int NT, typename T>
__global__ void __launch_bounds__(NT) scan_kernel(const T* __restrict__ in, T* __restrict__ prefix, T* __restrict__ total)
{
    __shared__ T row[NT / 64];
    T tot;
    prefix[threadIdx.x] = block_exclusive_scan<NT>(in[threadIdx.x], &tot, row);
    total[threadIdx.x] = tot;
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// the stated order on the host: xor tree per wave (every lane adds its partner's value to its own), then the waves in order
static double tree_sum(const double* v /* RN, stride NM */)
{
    double rows[RN / 64];
    for (int w = 0; w < RN / 64; ++w) {
        double a[64], b[64];
        for (int l = 0; l < 64; ++l) a[l] = v[(w * 64 + l) * NM];
        for (int d = 32; d >= 1; d >>= 1) {
            for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ d];
            memcpy(a, b, sizeof(a));
        }
        rows[w] = a[0];
    }
    double s = rows[0];
    for (int w = 1; w < RN / 64; ++w) s += rows[w];
    return s;
}

static bool same_bits(double x, double y) { return memcmp(&x, &y, sizeof(double)) == 0; }

template <int NT, typename T>
static int scan_case(const char* name, const std::vector<T>& in, T* d_in, T* d_prefix, T* d_total)
{
    std::vector<T> prefix(NT), total(NT);
    if (hipMemcpy(d_in, in.data(), NT * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 1;
    hipLaunchKernelGGL((scan_kernel<NT, T>), dim3(1), dim3(NT), 0, 0, d_in, d_prefix, d_total);
    if (hipMemcpy(prefix.data(), d_prefix, NT * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (hipMemcpy(total.data(), d_total, NT * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    T run = 0, all = 0;
    for (int i = 0; i < NT; ++i) all += in[i];
    int wrong = 0;
    for (int i = 0; i < NT; ++i) { wrong += prefix[i] != run || total[i] != all; run += in[i]; }
    if (wrong) printf("scan <%d, %zu-byte> %s: %d of %d threads wrong\n", NT, sizeof(T), name, wrong, NT);
    return wrong ? 1 : 0;
}

template <int NT, typename T>
static int scan_cases(bool is_u64)
{
    T *d_in, *d_prefix, *d_total;
    if (hipMalloc(&d_in, NT * sizeof(T)) != hipSuccess || hipMalloc(&d_prefix, NT * sizeof(T)) != hipSuccess || hipMalloc(&d_total, NT * sizeof(T)) != hipSuccess) return 1;
    int bad = 0;
    std::vector<T> v(NT, T(0));
    bad += scan_case<NT, T>("zeros", v, d_in, d_prefix, d_total);
    v.assign(NT, T(1));
    bad += scan_case<NT, T>("ones", v, d_in, d_prefix, d_total);
    v.assign(NT, T(0)); v[NT - 1] = T(7);
    bad += scan_case<NT, T>("last thread", v, d_in, d_prefix, d_total);
    v.assign(NT, T(0)); v[63] = T(5);
    bad += scan_case<NT, T>("thread 63", v, d_in, d_prefix, d_total);
    uint32_t s = 12345u + NT;
    for (int i = 0; i < NT; ++i) v[i] = T(lcg(s) % 1000u);
    bad += scan_case<NT, T>("random", v, d_in, d_prefix, d_total);
    if (is_u64) {
        // the prefix passes 2^32 at thread 2, inside wave 0; wave 0 sums to 32 * 2^32 - 1, so the next value carries into bit 37 right at the wave boundary
        for (int i = 0; i < NT; ++i) v[i] = T((1ull << 31) + (unsigned)i);
        for (int i = 0; i < 63; ++i) v[i] = T(1ull << 31);
        v[63] = T((1ull << 31) - 1); v[64] = T(1);
        bad += scan_case<NT, T>("across 2^32", v, d_in, d_prefix, d_total);
    }
    (void)hipFree(d_in); (void)hipFree(d_prefix); (void)hipFree(d_total);
    return bad;
}

int main()
{
    // ---- the f64 table, and whether it can tell the orders apart (host only) ----
    std::vector<double> tab(RN * NM), tree(NM);
    uint32_t seed = 2024u;
    for (int i = 0; i < RN * NM; ++i) {
        const uint32_t h = lcg(seed), g = lcg(seed);
        const double m = 1.0 + (double)(g & 0xFFFFFu) / 1048576.0;
        tab[i] = ((h & 1u) ? -1.0 : 1.0) * ldexp(m, (int)((h >> 1) % 61u) - 30);
    }
    int differ = 0;
    for (int k = 0; k < NM; ++k) {
        tree[k] = tree_sum(tab.data() + k);
        double plain = 0.0;
        for (int i = 0; i < RN; ++i) plain += tab[i * NM + k];
        differ += !same_bits(tree[k], plain);
    }
    printf("index-order sum differs from the tree sum in %d of %d components\n", differ, NM);
    if (differ < 12) { printf("block ops WRONG: the table cannot tell the summation orders apart\n"); return 1; }

    int bad = 0;
    // ---- block_reduce<256, 18>, doubles: bit for bit ----
    {
        double *d_in, *d_out;
        CHECK(hipMalloc(&d_in, tab.size() * sizeof(double)));
        CHECK(hipMalloc(&d_out, NM * sizeof(double)));
        CHECK(hipMemcpy(d_in, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL((reduce_kernel<NM, double, op_add>), dim3(1), dim3(RN), 0, 0, d_in, d_out);
        std::vector<double> out(NM);
        CHECK(hipMemcpy(out.data(), d_out, NM * sizeof(double), hipMemcpyDeviceToHost));
        int wrong = 0;
        for (int k = 0; k < NM; ++k) wrong += !same_bits(out[k], tree[k]);
        if (wrong) { printf("block_reduce<256, 18> f64: %d of %d words differ from the stated tree\n", wrong, NM); ++bad; }
        (void)hipFree(d_in); (void)hipFree(d_out);
    }
    // ---- block_reduce<256, 6>, min / max with infinities ----
    {
        std::vector<float> in(RN * 6), want(6);
        uint32_t s = 99u;
        for (int i = 0; i < RN * 6; ++i) in[i] = ((float)(lcg(s) % 20001u) - 10000.5f) * 0.25f;
        in[5 * 6 + 0] = INFINITY; in[70 * 6 + 0] = -INFINITY;          // a -inf wins the min
        in[130 * 6 + 1] = INFINITY;                                    // a +inf does not
        in[200 * 6 + 4] = INFINITY; in[255 * 6 + 4] = -INFINITY;       // a +inf wins the max
        in[0 * 6 + 5] = -INFINITY;                                     // a -inf does not
        for (int k = 0; k < 6; ++k) {
            want[k] = in[k];
            for (int i = 1; i < RN; ++i) want[k] = k < 3 ? fminf(want[k], in[i * 6 + k]) : fmaxf(want[k], in[i * 6 + k]);
        }
        float *d_in, *d_out;
        CHECK(hipMalloc(&d_in, in.size() * sizeof(float)));
        CHECK(hipMalloc(&d_out, 6 * sizeof(float)));
        CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL((reduce_kernel<6, float, MinMax>), dim3(1), dim3(RN), 0, 0, d_in, d_out);
        std::vector<float> out(6);
        CHECK(hipMemcpy(out.data(), d_out, 6 * sizeof(float), hipMemcpyDeviceToHost));
        if (memcmp(out.data(), want.data(), 6 * sizeof(float)) != 0) { printf("block_reduce<256, 6> min / max differs from the host's\n"); ++bad; }
        (void)hipFree(d_in); (void)hipFree(d_out);
    }
    // ---- wave_reduce: every lane holds its wave's sum ----
    {
        std::vector<uint32_t> in(RN), out(RN);
        uint32_t s = 7u;
        for (int i = 0; i < RN; ++i) in[i] = lcg(s);
        uint32_t *d_in, *d_out;
        CHECK(hipMalloc(&d_in, RN * sizeof(uint32_t)));
        CHECK(hipMalloc(&d_out, RN * sizeof(uint32_t)));
        CHECK(hipMemcpy(d_in, in.data(), RN * sizeof(uint32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(wave_sum_kernel, dim3(1), dim3(RN), 0, 0, d_in, d_out);
        CHECK(hipMemcpy(out.data(), d_out, RN * sizeof(uint32_t), hipMemcpyDeviceToHost));
        int wrong = 0;
        for (int w = 0; w < RN / 64; ++w) {
            uint32_t sum = 0;
            for (int l = 0; l < 64; ++l) sum += in[w * 64 + l];
            for (int l = 0; l < 64; ++l) wrong += out[w * 64 + l] != sum;
        }
        if (wrong) { printf("wave_reduce: %d of %d lanes do not hold their wave's sum\n", wrong, RN); ++bad; }
        (void)hipFree(d_in); (void)hipFree(d_out);
    }
    // ---- block_exclusive_scan ----
    bad += scan_cases<256, uint64_t>(true);
    bad += scan_cases<512, int>(false);
    bad += scan_cases<256, uint32_t>(false);
    CHECK(hipDeviceSynchronize());
    printf(bad ? "block ops WRONG in %d case(s)\n" : "block ops ok (%d cases wrong)\n", bad);
    return bad ? 1 : 0;
}
