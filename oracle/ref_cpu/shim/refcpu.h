/*
 * refcpu.h -- the part of the CUDA language, runtime, cooperative_groups and CUB that the reference rasterizer's three translation units
 * use, implemented for one CPU thread (TEST INFRASTRUCTURE ONLY; own code, nothing of the reference in it).
 *
 * oracle/ref_cpu/build.py compiles the reference's forward.cu / backward.cu / rasterizer_impl.cu against this header with g++; what then
 * runs is the reference's own arithmetic.  What this header decides, and the reference does not:
 *   - execution order: blocks run one after another (optionally last to first), the threads of a block are fibers that run in rank order
 *     and switch only at a barrier, so float atomicAdd sums in a fixed order and a run is reproducible bit for bit;
 *   - __expf is expf (the hardware approximation of the exponential is not modelled);
 *   - tex2DLayered restates NVIDIA's PUBLISHED formula for linear filtering (CUDA C++ Programming Guide, "Texture Fetching": xB = x - 0.5,
 *     i = floor(xB), alpha = frac(xB), clamp addressing) in one of two forms chosen by refcpu::tex_quant: alpha and beta exact in float32, or
 *     rounded to the documented 1.8 fixed point (8 fractional bits).  This is a restatement of the documentation, NOT a measurement of a
 *     texture unit.
 */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __shared__ static /* one OS thread, one block at a time: a function-local static is per-block storage */
#define __forceinline__ inline
#define __launch_bounds__(...)

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct uint2 { unsigned int x, y; };
struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
static inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

/* CUDA's min / max overload set in the global namespace, mixed signedness included (int against unsigned compares as unsigned) */
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
static inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
static inline unsigned int min(int a, unsigned int b) { return min((unsigned int)a, b); }
static inline unsigned int min(unsigned int a, int b) { return min(a, (unsigned int)b); }
static inline unsigned int max(int a, unsigned int b) { return max((unsigned int)a, b); }
static inline unsigned int max(unsigned int a, int b) { return max(a, (unsigned int)b); }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline double min(double a, double b) { return fmin(a, b); }
static inline double max(double a, double b) { return fmax(a, b); }
static inline double min(float a, double b) { return fmin((double)a, b); }
static inline double min(double a, float b) { return fmin(a, (double)b); }
static inline double max(float a, double b) { return fmax((double)a, b); }
static inline double max(double a, float b) { return fmax(a, (double)b); }

static inline float refcpu_expf(float x) { return expf(x); }
#define __expf refcpu_expf /* glibc's <math.h> declares a __expf of its own */
static inline void __trap() { abort(); }
static inline float atomicAdd(float* p, float v) { const float old = *p; *p = old + v; return old; }

/* ---- execution model (runtime.cpp) ---- */
extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;
namespace refcpu {
extern bool reverse_blocks; /* visit the blocks of every launch last to first */
extern bool tex_quant;      /* linear-filter weights in 1.8 fixed point */
void barrier();             /* yields until every thread of the block has arrived */
int barrier_count(int pred);
void run_grid(dim3 grid, dim3 block, void (*body)(void*), void* arg);

template <typename... P>
struct Launch {
    dim3 g, b;
    void (*k)(P...);
    template <typename... A>
    void operator()(A&&... a) const
    {
        auto call = [&]() { k(static_cast<P>(a)...); };
        run_grid(g, b, [](void* c) { (*static_cast<decltype(call)*>(c))(); }, &call);
    }
};
template <typename... P>
Launch<P...> make_launch(dim3 g, dim3 b, void (*k)(P...)) { return Launch<P...>{g, b, k}; }
} // namespace refcpu
/* `kernel<<<grid, block>>>(args)` is rewritten by build.py into REFCPU_LAUNCH(grid, block, kernel)(args) */
#define REFCPU_LAUNCH(g, b, ...) refcpu::make_launch(g, b, __VA_ARGS__)
static inline void __syncthreads() { refcpu::barrier(); }
static inline int __syncthreads_count(int pred) { return refcpu::barrier_count(pred); }

namespace cooperative_groups {
struct thread_block {
    static dim3 group_index() { return dim3(blockIdx.x, blockIdx.y, blockIdx.z); }
    static dim3 thread_index() { return dim3(threadIdx.x, threadIdx.y, threadIdx.z); }
    static unsigned int thread_rank() { return (threadIdx.z * blockDim.y + threadIdx.y) * blockDim.x + threadIdx.x; }
    static void sync() { refcpu::barrier(); }
};
struct grid_group {
    static unsigned long long thread_rank()
    {
        const unsigned long long blk = ((unsigned long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        return blk * ((unsigned long long)blockDim.x * blockDim.y * blockDim.z) + thread_block::thread_rank();
    }
};
static inline thread_block this_thread_block() { return thread_block(); }
static inline grid_group this_grid() { return grid_group(); }
} // namespace cooperative_groups

/* ---- runtime API ---- */
typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
static inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
static inline const char* cudaGetErrorString(cudaError_t) { return "no error"; }
static inline cudaError_t cudaMemcpy(void* d, const void* s, size_t n, cudaMemcpyKind) { memcpy(d, s, n); return cudaSuccess; }
static inline cudaError_t cudaMemset(void* d, int v, size_t n) { memset(d, v, n); return cudaSuccess; }
static inline cudaError_t cudaMalloc(void** p, size_t n) { *p = calloc(n ? n : 1, 1); return cudaSuccess; }
static inline cudaError_t cudaFree(void* p) { free(p); return cudaSuccess; }

/* ---- layered arrays and texture objects ---- */
struct cudaChannelFormatDesc { int channels; };
template <typename T> cudaChannelFormatDesc cudaCreateChannelDesc();
template <> inline cudaChannelFormatDesc cudaCreateChannelDesc<float4>() { return cudaChannelFormatDesc{4}; }
template <> inline cudaChannelFormatDesc cudaCreateChannelDesc<float>() { return cudaChannelFormatDesc{1}; }
struct cudaExtent { size_t width, height, depth; };
static inline cudaExtent make_cudaExtent(size_t w, size_t h, size_t d) { return cudaExtent{w, h, d}; }
struct cudaArray { int w, h, layers, channels; std::vector<float> data; };
typedef cudaArray* cudaArray_t;
enum { cudaArrayLayered = 1 };
static inline cudaError_t cudaMalloc3DArray(cudaArray_t* a, const cudaChannelFormatDesc* d, cudaExtent e, unsigned int)
{
    *a = new cudaArray{(int)e.width, (int)e.height, (int)e.depth, d->channels, std::vector<float>(e.width * e.height * e.depth * d->channels, 0.f)};
    return cudaSuccess;
}
static inline cudaError_t cudaFreeArray(cudaArray_t a) { delete a; return cudaSuccess; }
struct cudaPitchedPtr { void* ptr; size_t pitch, xsize, ysize; };
static inline cudaPitchedPtr make_cudaPitchedPtr(void* p, size_t pitch, size_t xs, size_t ys) { return cudaPitchedPtr{p, pitch, xs, ys}; }
struct cudaMemcpy3DParms { cudaPitchedPtr srcPtr; cudaArray_t dstArray; cudaExtent extent; cudaMemcpyKind kind; };
static inline cudaError_t cudaMemcpy3D(const cudaMemcpy3DParms* p)
{
    cudaArray* a = p->dstArray;
    const size_t row = (size_t)a->w * a->channels * sizeof(float);
    for (size_t z = 0; z < p->extent.depth; z++)
        for (size_t y = 0; y < p->extent.height; y++)
            memcpy(reinterpret_cast<char*>(a->data.data()) + (z * a->h + y) * row,
                   static_cast<const char*>(p->srcPtr.ptr) + (z * p->srcPtr.ysize + y) * p->srcPtr.pitch, row);
    return cudaSuccess;
}
enum cudaResourceType { cudaResourceTypeArray };
struct cudaResourceDesc { cudaResourceType resType; struct { struct { cudaArray_t array; } array; } res; };
enum cudaTextureAddressMode { cudaAddressModeWrap, cudaAddressModeClamp };
enum cudaTextureFilterMode { cudaFilterModePoint, cudaFilterModeLinear };
enum cudaTextureReadMode { cudaReadModeElementType };
struct cudaTextureDesc { cudaTextureAddressMode addressMode[3]; cudaTextureFilterMode filterMode; cudaTextureReadMode readMode; int normalizedCoords; };
typedef unsigned long long cudaTextureObject_t;
static inline cudaError_t cudaCreateTextureObject(cudaTextureObject_t* t, const cudaResourceDesc* r, const cudaTextureDesc* d, const void*)
{
    /* the one configuration the sampler below implements */
    if (d->addressMode[0] != cudaAddressModeClamp || d->addressMode[1] != cudaAddressModeClamp || d->filterMode != cudaFilterModeLinear || d->normalizedCoords)
        throw std::runtime_error("refcpu: texture mode not implemented");
    *t = (cudaTextureObject_t)(uintptr_t)r->res.array.array;
    return cudaSuccess;
}
static inline cudaError_t cudaDestroyTextureObject(cudaTextureObject_t) { return cudaSuccess; }

namespace refcpu {
/* the four texels and two weights of one linear fetch (header comment: the published formula, clamp addressing) */
struct Tap { int i0, i1, j0, j1; float a, b; };
static inline Tap tap(const cudaArray* t, float x, float y)
{
    const float xb = x - 0.5f, yb = y - 0.5f;
    const float fi = floorf(xb), fj = floorf(yb);
    float a = xb - fi, b = yb - fj;
    if (tex_quant) { a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f); b = floorf(b * 256.0f + 0.5f) * (1.0f / 256.0f); }
    const int i = (int)fi, j = (int)fj;
    return Tap{min(t->w - 1, max(0, i)), min(t->w - 1, max(0, i + 1)), min(t->h - 1, max(0, j)), min(t->h - 1, max(0, j + 1)), a, b};
}
static inline float filt(const Tap& k, float t00, float t10, float t01, float t11)
{
    return (1.f - k.a) * (1.f - k.b) * t00 + k.a * (1.f - k.b) * t10 + (1.f - k.a) * k.b * t01 + k.a * k.b * t11;
}
} // namespace refcpu
template <typename T> T tex2DLayered(cudaTextureObject_t tex, float x, float y, int layer);
template <> inline float tex2DLayered<float>(cudaTextureObject_t tex, float x, float y, int layer)
{
    const cudaArray* t = (const cudaArray*)(uintptr_t)tex;
    const refcpu::Tap k = refcpu::tap(t, x, y);
    const float* p = t->data.data() + (size_t)layer * t->w * t->h;
    return refcpu::filt(k, p[(size_t)k.j0 * t->w + k.i0], p[(size_t)k.j0 * t->w + k.i1], p[(size_t)k.j1 * t->w + k.i0], p[(size_t)k.j1 * t->w + k.i1]);
}
template <> inline float4 tex2DLayered<float4>(cudaTextureObject_t tex, float x, float y, int layer)
{
    const cudaArray* t = (const cudaArray*)(uintptr_t)tex;
    const refcpu::Tap k = refcpu::tap(t, x, y);
    const float* p = t->data.data() + (size_t)layer * t->w * t->h * 4;
    float o[4];
    for (int c = 0; c < 4; c++)
        o[c] = refcpu::filt(k, p[((size_t)k.j0 * t->w + k.i0) * 4 + c], p[((size_t)k.j0 * t->w + k.i1) * 4 + c],
                            p[((size_t)k.j1 * t->w + k.i0) * 4 + c], p[((size_t)k.j1 * t->w + k.i1) * 4 + c]);
    return float4{o[0], o[1], o[2], o[3]};
}

/* ---- CUB: one scan and one pair sort; a null temp-storage pointer is the size query, as in CUB ---- */
namespace cub {
struct DeviceScan {
    template <typename In, typename Out>
    static cudaError_t InclusiveSum(void* tmp, size_t& bytes, In in, Out out, int n)
    {
        if (!tmp) { bytes = 256; return cudaSuccess; }
        if (n > 0) { auto s = in[0]; out[0] = s; for (int i = 1; i < n; i++) { s = s + in[i]; out[i] = s; } }
        return cudaSuccess;
    }
};
struct DeviceRadixSort {
    template <typename K, typename V>
    static cudaError_t SortPairs(void* tmp, size_t& bytes, const K* kin, K* kout, const V* vin, V* vout, int n, int begin_bit = 0, int end_bit = sizeof(K) * 8)
    {
        if (!tmp) { bytes = 256; return cudaSuccess; }
        const int nb = end_bit - begin_bit;
        const K mask = nb >= (int)sizeof(K) * 8 ? ~K(0) : (K(1) << nb) - 1;
        std::vector<int> idx(n);
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return ((kin[a] >> begin_bit) & mask) < ((kin[b] >> begin_bit) & mask); });
        for (int i = 0; i < n; i++) { kout[i] = kin[idx[i]]; vout[i] = vin[idx[i]]; }
        return cudaSuccess;
    }
};
} // namespace cub
