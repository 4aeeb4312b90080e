/*
 * ibgs_geo_loss.h -- C ABI of the two geometry loss terms in libibgs_rast.so (ibgs_amd/csrc/geoloss.hip): the multi-view photometric term and the
 * normal-consistency term of the reference's steady-state iteration (train.py:308-338), each with its gradient.  Python: ibgs_amd/losses.py
 * (`photometric_loss`, `normal_consistency`).
 *
 * Images are float32, planes of H x W, contiguous.  The photometric term reads gt (3 planes), warped (S_total x 3 planes) and cam_feat (S_total x 4 planes)
 * and uses the first S sources:
 *   valid[s, p] = (((f0 + f1) + f2) + f3) > 0 in float32, in that order;   masked = valid ? warped : gt;
 *   m[s, c] = the structural-similarity map of (gt, masked[s]) exactly as include/ibgs_ssim.h defines it (same window, padding and per-pixel forms);
 *   Nv = sum valid;  ss = sum valid (1 - mean_c m) / Nv;  l1 = sum valid mean_c |gt - masked| / Nv;
 *   loss = photo_weight ((1 - photo_ssim_weight) l1 + photo_ssim_weight ss), and exactly 0 when Nv == 0 (decided on the device).
 * The normal-consistency term reads two images of 3 planes:
 *   loss = weight (0.4 mean_p sum_c |dn - n| + 0.6 mean_p (1 - sum_c dn n)).
 * The contract is a tolerance against a float64 restatement (tests/geoloss_ref.py).  Promised bit for bit: the same arguments give the
 * same results on every call and stream (f64 partial sums per workgroup added in a fixed order, no float atomics), and sources from S on are never read.
 *
 * Conventions are those of ibgs_ssim.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.  Arguments are validated before any HIP call.
 *
 * Limits: 1 <= S <= S_total <= IBGS_GEOLOSS_MAX_SRC; 1 <= H, W <= IBGS_GEOLOSS_MAX_SIDE.
 */
#ifndef IBGS_GEO_LOSS_H
#define IBGS_GEO_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_GEOLOSS_MAX_SRC 5
#define IBGS_GEOLOSS_MAX_SIDE 65536

/* bytes of the scratch of the two forward entry points for `sources` sources (1 for the normal term) of H x W (three f64 partial sums per workgroup;
 * 128-byte aligned); 0 when an argument is out of range */
size_t ibgs_geoloss_required_scratch(int64_t sources, int64_t H, int64_t W);

/* the tile of one workgroup of the photometric kernels (rows, columns) */
void ibgs_geoloss_tile(int32_t* th, int32_t* tw);

/* warped and cam_feat: the first S sources are read.  loss_out (1 float) and nv_out (1 double: Nv) are required.
 * dplanes_out (3 x S x 3 x H x W, or null): dm/dv, dm/dq, dm/dr -- the derivatives with respect to the masked side's statistics -- times valid: what
 * ibgs_geoloss_photo_backward needs. */
int32_t ibgs_geoloss_photo_forward(void* stream, int32_t S, int32_t H, int32_t W, const float* gt, const float* warped, const float* cam_feat, double photo_weight,
                                   double photo_ssim_weight, float* dplanes_out, float* loss_out, double* nv_out, void* scratch, size_t scratch_bytes);

/* grad_warped (S_total x 3 x H x W, every element written) = valid ? k_s combine(w*D0, w*D1, w*D2; warped, gt) + k_1 sign(warped - gt) : 0 in the first S
 * sources and 0 in the rest, with k_s = -go photo_weight photo_ssim_weight / (3 Nv), k_1 = go photo_weight (1 - photo_ssim_weight) / (3 Nv), both 0 when
 * Nv == 0, formed on the device from nv (what the forward wrote) and grad_out (1 float: the gradient arriving at the loss).  sign(0) = 0. */
int32_t ibgs_geoloss_photo_backward(void* stream, int32_t S, int32_t S_total, int32_t H, int32_t W, const float* gt, const float* warped, const float* cam_feat,
                                    const float* dplanes, const double* nv, const float* grad_out, double photo_weight, double photo_ssim_weight, float* grad_warped);

/* loss_out (1 float) is required.  grad_normal, grad_depth_normal (3 x H x W each, or null): the gradients of the loss under an incoming gradient of one,
 * weight / (H W) (-/+ 0.4 sign(dn - n) - 0.6 other), from the same pass over the six planes. */
int32_t ibgs_geoloss_normal_forward(void* stream, int32_t H, int32_t W, const float* normal, const float* depth_normal, double weight, float* grad_normal,
                                    float* grad_depth_normal, float* loss_out, void* scratch, size_t scratch_bytes);

/* grad[0 .. n) *= *scale_dev in place; moves no data when the device scalar is 1.0 */
int32_t ibgs_geoloss_rescale(void* stream, int64_t n, float* grad, const float* scale_dev);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_GEO_LOSS_H */
