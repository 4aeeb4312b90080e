/*
 * ibgs_ssim.h -- C ABI of the fused SSIM in libibgs_rast.so (ibgs_amd/csrc/ssim.hip): value, map and gradient of the reference's `ssim` /
 * `compute_photometric_ssim` (utils/loss_utils.py:34-91) and, from the same pass over the two images, the per-image MSE (-> PSNR,
 * utils/image_utils.py:18-20) and the L1.  Python: ibgs_amd/losses.py (`ssim`, `ssim_map`), ibgs_amd/image_eval.py.
 *
 * Images are float32, N x C x H x W, contiguous: planes = N C independent planes (the window is per channel and the same for every channel).
 * Window: 11 taps, sigma 1.5, the reference's float32 1-D weights applied separably, zero padding of 5 on every side of every plane.
 * With u, v = w*x, w*y;  p, q, r = w*x^2, w*y^2, w*xy;  s1 = p - u^2, s2 = q - v^2, s12 = r - uv;  C1 = 0.01^2, C2 = 0.03^2:
 *   A = 2uv + C1, B = 2 s12 + C2, C = u^2 + v^2 + C1, D = s1 + s2 + C2, m = A B / (C D).
 * m is bit-symmetric in (x, y), and m == 1 exactly where x == y over the window.  The contract is a tolerance against a float64 restatement
 * ("Fused SSIM"; tests/ssim_ref.py), not bits; what IS promised bit for bit: the same arguments give the same results on every call, and a
 * plane's map, sums and gradient do not depend on the other planes of the call.
 *
 * Conventions are those of ibgs_dtu.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.
 *
 * Limits: N, C >= 1; 1 <= H, W <= IBGS_SSIM_MAX_SIDE; N C ceil(H / tile_h) ceil(W / tile_w) < 2^31.
 */
#ifndef IBGS_SSIM_H
#define IBGS_SSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_SSIM_WINDOW 11
#define IBGS_SSIM_MAX_SIDE 65536

/* bytes of the scratch of ibgs_ssim_forward (three f64 partial sums per workgroup, three f64 sums per plane; 128-byte aligned); 0 when an argument is
 * out of range */
size_t ibgs_ssim_required_scratch(int64_t planes, int64_t H, int64_t W);

/* the tile of one workgroup (rows, columns) */
void ibgs_ssim_tile(int32_t* th, int32_t* tw);

/* map_out (N x C x H x W, or null): m.
 * dmaps_out (3 x N x C x H x W, or null): dm/du, dm/dp, dm/dr, what ibgs_ssim_backward needs for the gradient with respect to x.
 * out_mean (1 float, or null): mean of m over everything.  out_per_image (N, or null): mean of m over each image.  out_mse_per_image (N, or null): mean of
 * (x - y)^2 over each image.  out_l1 (1 float, or null): mean of |x - y| over everything.  out_l1_per_image (N, or null): mean of |x - y| over each image.
 * All five null: no sums are formed and no scratch is needed.
 * The sums are f64: one partial per workgroup, added in a fixed order by a one-workgroup kernel; no float atomics. */
int32_t ibgs_ssim_forward(void* stream, int32_t N, int32_t C, int32_t H, int32_t W, const float* x, const float* y, float* map_out, float* dmaps_out,
                          float* out_mean, float* out_per_image, float* out_mse_per_image, float* out_l1, float* out_l1_per_image, void* scratch,
                          size_t scratch_bytes);

/* grad_x[t] = (w * [G dm/du])(t) + 2 x(t) (w * [G dm/dp])(t) + y(t) (w * [G dm/dr])(t) with the upstream gradient G read on the device: exactly one of
 * plane_scale (N C floats: G is constant over a plane) and grad_map (N x C x H x W) is given.  dmaps: what ibgs_ssim_forward(x, y) wrote.  The gradient
 * with respect to the second image is the same call on ibgs_ssim_forward(y, x)'s dmaps, with x and y swapped. */
int32_t ibgs_ssim_backward(void* stream, int32_t N, int32_t C, int32_t H, int32_t W, const float* x, const float* y, const float* dmaps,
                           const float* plane_scale, const float* grad_map, float* grad_x);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_SSIM_H */
