// Workgroup reduce and scan of one value (or a few) per thread: the one statement of what knn.hip, tsdf.hip, mesh.hip, mesh_eval.hip and registration.hip
// each used to spell out for themselves.  Device code only; tests/csrc/test_block_ops.hip pins every order below against a host restatement, bit for bit.
// Nothing here multiplies, so there is nothing to contract: the results do not depend on -ffp-contract.
#pragma once
#include <hip/hip_runtime.h>

namespace ibgs {

// op(x, y) for wave_reduce, op(x, y, k) for component k of block_reduce: these serve both
struct op_add { template <typename T> __device__ __forceinline__ T operator()(T x, T y, int = 0) const { return x + y; } };
struct op_min { __device__ __forceinline__ float operator()(float x, float y, int = 0) const { return fminf(x, y); } };
struct op_max { __device__ __forceinline__ float operator()(float x, float y, int = 0) const { return fmaxf(x, y); } };

// ---- wave ----------------------------------------------------------------------------------------------------------------------------------------
// The xor tree over the 64 lanes: for d = 32, 16, .., 1: v = op(v, v of lane ^ d).  Every lane ends with the same value, and for a float sum with the same
// bits on every run: lane l adds its partner's value to its own, the partner adds the same two numbers the other way round.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

// ---- workgroup reduce ----------------------------------------------------------------------------------------------------------------------------
// N values per thread over a workgroup of NT threads (a multiple of 64).  THE ORDER IS THE CONTRACT (registration.hip's moments promise the same 18 words
// on every run, and this is where their tree is written down):
//   1. component k through wave_reduce inside each wave, with (x, y) -> op(x, y, k);
//   2. lane 0 of each wave stores its N results as row `wave` of an LDS table of NT / 64 rows;
//   3. one __syncthreads;
//   4. thread k < N starts from row 0's component k and folds rows 1, 2, .. in that order: v = op(v, row w's, k).
// -> in thread k < N the result of component k (other threads: unspecified).  The second form stores it to dst[k].
// The LDS table is the function's own (NT / 64 x N values per instantiation).  Every caller calls it once per kernel; a kernel that called it twice
// would need a barrier between the calls (the second call's stores race the first call's step 4).
template <int NT, int N, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T (&a)[N], Op op)
{
    static_assert(NT % 64 == 0 && N <= NT, "whole waves, and a thread per component");
    __shared__ T s_row[NT / 64][N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = wave_reduce(a[k], [&](T x, T y) { return op(x, y, k); });
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < N; ++k) s_row[threadIdx.x >> 6][k] = a[k];
    __syncthreads();
    T v = T();
    if (threadIdx.x < N) {
        v = s_row[0][threadIdx.x];
        for (int w = 1; w < NT / 64; ++w) v = op(v, s_row[w][threadIdx.x], (int)threadIdx.x);
    }
    return v;
}
template <int NT, int N, typename T, typename Op>
__device__ __forceinline__ void block_reduce(T (&a)[N], T* dst, Op op)
{
    const T v = block_reduce<NT, N>(a, op);
    if (threadIdx.x < N) dst[threadIdx.x] = v;
}

// ---- workgroup exclusive scan --------------------------------------------------------------------------------------------------------------------
// Integers.  An inclusive shfl_up scan inside each wave; lane 63 stores the wave's total to lds_row[wave]; one __syncthreads; every thread adds up the rows
// before its wave, and all rows.  -> the sum of v over the threads before this one; *total = the workgroup's sum, in every thread.
// lds_row: NT / 64 values of LDS, the caller's.  A second scan may start without a barrier only into ANOTHER row (tsdf.hip keeps two in flight); before the
// same row is reused every thread must have passed a barrier.
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* total, T* lds_row)
{
    static_assert(NT % 64 == 0, "whole waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds_row[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
    for (int k = 0; k < NT / 64; ++k) { const T x = lds_row[k]; before += k < wave ? x : T(0); all += x; }
    *total = all;
    return before + inc - v;
}

}  // namespace ibgs
