/*
 * ibgs_lpips.h -- C ABI of LPIPS (VGG16, version 0.1) in libibgs_rast.so (ibgs_amd/csrc/lpips.hip): the third column of the reference's image evaluation
 * (metrics.py:82; lpipsPyTorch/modules/{lpips,networks,utils}.py with net_type 'vgg').  Python: ibgs_amd/lpips.py (`lpips`, `LPIPSNet`).
 *
 * x and y are 3 float32 planes of H x W each, contiguous, values as given (the reference feeds [0, 1] images; nothing is rescaled here either).
 *   z        = (v - mean_c) / std_c,  mean = (-.030, -.088, -.188), std = (.458, .448, .450); the zero padding of conv1_1 is zero in z-space
 *   features = the thirteen 3 x 3, padding-1 convolutions of vgg16.features, each followed by ReLU, channels
 *              3 -> 64 -> 64 | 128 -> 128 | 256 -> 256 -> 256 | 512 -> 512 -> 512 | 512 -> 512 -> 512, with a 2 x 2, stride-2 maximum at every `|` (an odd
 *              last row or column is dropped).  With H0 = H and H(k+1) = Hk / 2 (W alike) level k has Hk x Wk pixels.
 *   taps     = relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: 64, 128, 256, 512, 512 channels at levels 0 .. 4
 *   per tap k and pixel p:  n = f / (sqrt(sum_c f^2) + 1e-10);  m_k(p) = sum_c w_k[c] (n_x[c, p] - n_y[c, p])^2;  v_k = mean_p m_k(p);  lpips = sum_k v_k
 * The convolutions are float32 multiply-add chains on the matrix cores started from the bias, over k = 9 (input channel) + tap.  The head forms the two
 * norms and m_k(p) in double from the float32 features and rounds m_k(p) once to float32; v_k is the double sum of those float32 values, workgroup partials
 * added in a fixed order, divided by the pixel count; lpips is v_1 + .. + v_5 in double, rounded once.  The contract is a tolerance against a float64
 * restatement (tests/lpips_ref.py).  Promised bit for bit: the same arguments give the same results on every call and stream (no
 * atomics, nothing crosses a workgroup but through the partials).
 *
 * Parameters are in nn.Conv2d layout: conv_w[i] (Cout, Cin, 3, 3), conv_b[i] (Cout) for the thirteen convolutions in order, lin_w[k] (C_k) for the taps.
 * conv_w, conv_b, lin_w and maps are HOST arrays of device pointers.
 *
 * THE ARENA serves ONE pair (a batch loops on the host with the same arena).  A stage holds both images: [x: C planes of Hk x Wk | y: the same].  With
 * n(C, k) = 2 C Hk Wk floats the arena is two buffers of n(64, 0) floats and the head's partials:
 *   Q at 0:           relu1_2 (tap 1)
 *   P at n(64, 0):    relu1_1, and once that is dead, nested in the space of the stage that died last:
 *                       P + 0                      relu2_1, then relu3_1, then relu3_3 (tap 3)
 *                       P + n(128, 1)              relu2_2 (tap 2)
 *                       P + n(256, 2)              relu3_2, then relu4_1, then relu4_3 (tap 4)
 *                       P + n(256, 2) + n(512, 3)  relu4_2, then relu5_1 | relu5_2 | relu5_3 (tap 5) side by side
 *   partials at 2 n(64, 0) floats: sum_k ceil(Hk Wk / 256) doubles
 * (4 H(k+1) W(k+1) <= Hk Wk makes every nesting fit; every offset is a multiple of 512 bytes).  ibgs_lpips_required_scratch is the end of the partials
 * rounded up to 128 bytes: 2 123 452 800 bytes at 1080 x 1920 (2 123 366 400 of them the two full-resolution 64-channel stages of the two images),
 * 17 180 567 552 at 4096 x 4096.  After the call the ten tap tensors are in the arena at the places above.
 *
 * Conventions are those of ibgs_hourglass.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.  Arguments are validated before any HIP call.
 *
 * Limits: IBGS_LPIPS_MIN_SIDE <= H, W <= IBGS_LPIPS_MAX_SIDE (16 is the least that leaves a pixel after four pools; 4096 keeps the arena below 20 GB).
 */
#ifndef IBGS_LPIPS_H
#define IBGS_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_LPIPS_MIN_SIDE 16
#define IBGS_LPIPS_MAX_SIDE 4096
#define IBGS_LPIPS_CONVS 13
#define IBGS_LPIPS_TAPS 5

/* bytes of the arena of ibgs_lpips_forward for a pair of H x W (the layout above); 0 when an argument is out of range */
size_t ibgs_lpips_required_scratch(int64_t H, int64_t W);

/* One 3 x 3 convolution with bias and ReLU on BOTH images of a stage (what ibgs_lpips_forward launches thirteen times; tools/bench_lpips.py times each):
 * in_x, in_y: cin planes of hs x ws each; out: [x: cout planes of h x w | y: the same].  pool = 0: (h, w) = (hs, ws); pool = 1: (h, w) = (hs / 2, ws / 2)
 * and the input is max-pooled 2 x 2 while it is staged.  zscore = 1 (cin = 3, pool = 0 only): the z-score above is applied to in-frame values while they
 * are staged.  cout a multiple of 64; cin = 3 with zscore, else a multiple of 4; both at most 512.  1 <= h, w <= IBGS_LPIPS_MAX_SIDE. */
int32_t ibgs_lpips_conv3(void* stream, int32_t hs, int32_t ws, int32_t cin, int32_t cout, int32_t pool, int32_t zscore, const float* in_x,
                         const float* in_y, const float* weight, const float* bias, float* out);

/* lpips: 1 float; tap_values: v_1 .. v_5 (5 floats), or null; maps: null, or 5 device pointers (each may be null) to H0 W0, .., H4 W4 floats that receive
 * m_k(p).  Thirteen convolution launches, five head launches and the final sum on `stream`. */
int32_t ibgs_lpips_forward(void* stream, int32_t H, int32_t W, const float* x, const float* y, const float* const* conv_w, const float* const* conv_b,
                           const float* const* lin_w, float* lpips, float* tap_values /* may be null */, float* const* maps /* may be null */,
                           void* scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_LPIPS_H */
