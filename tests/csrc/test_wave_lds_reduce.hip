// Stand-alone check of wave_lds_reduce12 (wave_reduce.h): the 12-value wave sum of the colour backward with the transposition done through LDS.
// Build + run on the GPU box: hipcc --offload-arch=gfx950 -O3 -o /tmp/t tests/csrc/test_wave_lds_reduce.hip && /tmp/t
// One launch, one wave per data set; every input is finite.  Checked per data set:
//   * the LDS reducer against the float64 sum of the same 64 x 12 inputs, and against the butterfly (wave_transpose_reduce12), each within the
//     rounding bound of a depth-6 float32 summation tree: every input passes through six additions, each rounding by at most 2^-24 of a partial
//     sum that is at most sum|x| in magnitude -- BOUND = 8 * 2^-24 * sum|x| leaves two additions of margin and is independent of any measured value;
//   * the column map lane by lane against its definition restated here, and that each of the 12 columns has exactly one owner.
// Data sets: random values; heavy cancellation (large values that cancel in pairs of lanes, small ones riding on them); three quarters of the lanes zero
// (what a wave sees when most pixels fail the alpha test); all lanes zero.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <cstdint>
#include "../../ibgs_amd/csrc/wave_reduce.h"

constexpr int NSET = 4;

__global__ void __launch_bounds__(64) k_sets(const float* in, float* out_lds, float* out_bfly, int* col_lds, int* col_bfly)
{
    __shared__ __align__(16) float buf[ibgs::LDS_REDUCE12_BYTES / sizeof(float)];
    const int lane = threadIdx.x, set = blockIdx.x;
    float v[12], w[12];
    for (int i = 0; i < 12; i++) v[i] = w[i] = in[(set * 64 + lane) * 12 + i];
    out_lds[set * 64 + lane] = ibgs::wave_lds_reduce12(v, lane, buf);
    out_bfly[set * 64 + lane] = ibgs::wave_transpose_reduce12(w, lane);
    col_lds[set * 64 + lane] = ibgs::lds_reduce12_column(lane);
    col_bfly[set * 64 + lane] = ibgs::reduce12_column(lane);
}

static uint32_t rng_state = 12345u;
static float urand()          // [-1, 1)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((rng_state >> 8) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

static int expected_lds_column(int lane)          // the definition, restated: row r = lane / 16 owns columns r, 4 + r, 8 + r in its lanes 0, 8, 1
{
    const int row = lane / 16, l = lane % 16;
    if (l == 0) return row;
    if (l == 8) return 4 + row;
    if (l == 1) return 8 + row;
    return -1;
}

int main()
{
    static float h[NSET * 64 * 12];
    for (int l = 0; l < 64; l++)
        for (int i = 0; i < 12; i++) {
            h[(0 * 64 + l) * 12 + i] = urand() * (float)(1 << (i % 5));                                         // random
            h[(1 * 64 + l) * 12 + i] = ((l & 1) ? -1.0f : 1.0f) * 1.0e6f * (float)(1 + ((l >> 1) * 7 + i) % 13) + urand();          // lanes 2m, 2m + 1 cancel to the small parts
            h[(2 * 64 + l) * 12 + i] = (l % 4 == (i % 4)) ? urand() * 3.0f : 0.0f;                              // three quarters of the lanes zero, a different quarter per column
            h[(3 * 64 + l) * 12 + i] = 0.0f;
        }
    float *d, *o1, *o2; int *c1, *c2;
    static float r1[NSET * 64], r2[NSET * 64];
    static int k1[NSET * 64], k2[NSET * 64];
    hipMalloc(&d, sizeof(h)); hipMalloc(&o1, sizeof(r1)); hipMalloc(&o2, sizeof(r2)); hipMalloc(&c1, sizeof(k1)); hipMalloc(&c2, sizeof(k2));
    hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_sets, dim3(NSET), dim3(64), 0, 0, d, o1, o2, c1, c2);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 2; }
    hipMemcpy(r1, o1, sizeof(r1), hipMemcpyDeviceToHost); hipMemcpy(r2, o2, sizeof(r2), hipMemcpyDeviceToHost);
    hipMemcpy(k1, c1, sizeof(k1), hipMemcpyDeviceToHost); hipMemcpy(k2, c2, sizeof(k2), hipMemcpyDeviceToHost);

    static const char* names[NSET] = {"random", "cancellation", "masked lanes", "all zero"};
    int bad = 0;
    for (int s = 0; s < NSET; s++) {
        int seen[12] = {0}, sbad = 0;
        double worst = 0, worst_b = 0;
        for (int l = 0; l < 64; l++) {
            const int c = k1[s * 64 + l];
            if (c != expected_lds_column(l)) { sbad++; printf("%s: lane %d owns column %d, expected %d\n", names[s], l, c, expected_lds_column(l)); continue; }
            if (c < 0) continue;
            seen[c]++;
            double want = 0, mag = 0;
            for (int m = 0; m < 64; m++) { want += h[(s * 64 + m) * 12 + c]; mag += fabs((double)h[(s * 64 + m) * 12 + c]); }
            const double bound = 8.0 * ldexp(1.0, -24) * mag;
            const double e = fabs(want - (double)r1[s * 64 + l]);
            // the butterfly's total of the same column, in the butterfly's own lane
            int lb = -1;
            for (int m = 0; m < 64; m++) if (k2[s * 64 + m] == c) lb = m;
            const double eb = lb < 0 ? INFINITY : fabs((double)r2[s * 64 + lb] - (double)r1[s * 64 + l]);
            if (mag > 0) { worst = fmax(worst, e / bound); worst_b = fmax(worst_b, eb / (2 * bound)); }
            if (!(e <= bound)) { sbad++; printf("%s: lane %d column %d: got %.9g, float64 sum %.9g (bound %.3g)\n", names[s], l, c, r1[s * 64 + l], want, bound); }
            if (!(eb <= 2 * bound)) { sbad++; printf("%s: column %d: LDS %.9g, butterfly %.9g (bound %.3g)\n", names[s], c, r1[s * 64 + l], lb < 0 ? NAN : r2[s * 64 + lb], 2 * bound); }
        }
        for (int i = 0; i < 12; i++) if (seen[i] != 1) { sbad++; printf("%s: column %d owned by %d lanes\n", names[s], i, seen[i]); }
        printf("wave_lds_reduce12, %s: %s (%d bad; worst error %.3f of the bound vs float64, %.3f vs the butterfly)\n", names[s], sbad ? "FAIL" : "OK", sbad, worst, worst_b);
        bad += sbad;
    }
    return bad != 0;
}
