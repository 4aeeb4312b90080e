/*
 * ibgs_resample_train.h -- C ABI of the reduced-resolution colour tail's BACKWARD in libibgs_rast.so (ibgs_amd/csrc/rsztrain.hip): the adjoints of the two
 * entry points of ibgs_resample.h, for TRAINING the colour network under `residual_resolution_scale != 1` (the reference's fuse_color,
 * color_aggregation_network.py:200-239, with train.py:227-228).  Python: ibgs_amd/resample_train.py (`resized_features_train`, `upsample_residual_train`,
 * `fuse_color_train_scaled`).  The forwards stay those of ibgs_resample.h; its SIZE, COORDINATE and VALUE rules are the ones meant below.
 *
 * ibgs_rzt_features_backward: the adjoint of ibgs_rsz_features_forward.  Arguments as there (without camera_ray) and grad_out (38 x Hr x Wr).  Requires
 * Hr <= H and Wr <= W (training an upscaled network is refused).  cam_feat and camera_ray get NO gradient: they are data, as in ibgs_color_agg.h.
 *   at reduced resolution   per reduced pixel q and slot k < levels the four masked taps, the blend and both layers are recomputed with the instructions of the
 *              forward (the same bits: the ReLU masks and the max-mode winner are those of the forward's own output); then, as ibgs_color_agg.h's backward,
 *                dz2 = g (h2 > 0), g = grad_out / levels (IBGS_RSZ_MEAN) or grad_out at the first slot attaining the maximum (IBGS_RSZ_MAX);
 *                dz1 = (w2^T dz2) (h1 > 0);  gx(k, c, q) = (w1^T dz1)[c] for c < 3.
 *              The products run on the f32 matrix cores (v_mfma_f32_32x32x2_f32).
 *   parameter gradients   dW2 = sum_q dz2 (x) h1, db2 = sum_q dz2, dW1 = sum_q dz1 (x) x, db1 = sum_q dz1, x the BLENDED slot.  Per-wave sums in a fixed order
 *              (dW2 as the matrix cores' f32 chain over one chunk of 32 pixels and its slots, from there on in f64; the other three in f64 throughout), the
 *              four waves of a workgroup in order, one f64 partial per workgroup in the scratch arena, a fixed-order final pass, ONE rounding to f32.
 *              No float atomics.
 *   image gradients   gx goes UNMASKED to scratch planes at Hr x Wr; a second kernel runs over the FULL-resolution pixels and gathers.  Because Hr <= H the
 *              integer tap y0(i) is strictly increasing in i: a full-resolution row y is tap y0 of at most one reduced row (weight u_y = 1 - t_y of that row)
 *              and tap y1 of at most one (weight t_y: the row whose y0 is y - 1), found in integers by the COORDINATE RULE; columns alike.  A pixel p so
 *              gathers from at most 2 x 2 reduced pixels with the weights w = {u_y u_x, u_y t_x, t_y u_x, t_y t_x} (float32 products of the forward's own t
 *              and u; a tap clamped onto its own row carries t = 0 and adds nothing):
 *                G(k, c, p) = sum_q w(q, p) gx(k, c, q)          an fma chain from 0, reduced rows ascending, then columns
 *                grad_warped[3k + c][p] = G(k, c, p) v(p, k)      v: p's own mask, (((f0 + f1) + f2) + f3) > 0; slots from `levels` on: zeros
 *                grad_render[c][p] = sum_q w(q, p) grad_out[35 + c][q] - sum_k G(k, c, p) v(p, k)          (k ascending)
 *              With grad_render and grad_warped both null neither the scratch planes nor this kernel are used.
 * Each of the six outputs may be null and is then not computed; at least one must be given.  Every element of a given output is written.
 *
 * ibgs_rzt_upsample_backward: the adjoint of ibgs_rsz_residual_upsample in residual_r, for ANY two sizes (Hr = 1, Wr = 1, H = 1, upscaling included):
 *   grad_residual_r[c][a][b] = sum_i sum_j w_y(i, a) w_x(j, b) g(c, i, j),   g = grad_residual_out + grad_image_pred (a float32 sum; either may be null, not
 *   both).  i runs over the full-resolution rows that have a among their two taps (weight u_y(i) where a is y0(i), t_y(i) where it is y1(i)); y0 is monotone
 *   in i, so they form a contiguous range, found in integers; columns alike.  ONE THREAD per reduced element adds its terms in ascending (i, j) order into an
 *   f64 accumulator (w_y w_x is exact there) and rounds once.  render's share, render_scale * grad_image_pred, is left to the caller.
 *
 * The contract is a tolerance against a float64 restatement (tests/resample_train_ref.py).  Promised bit for bit: the same arguments give
 * the same results on every call and stream, and every output element is written whatever the buffers (scratch included) held before.
 *
 * Conventions are those of ibgs_resample.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.  Arguments are validated before any HIP call.  scratch: 128-byte aligned, ibgs_rzt_required_scratch(S, H, W, Hr, Wr) bytes (0 for sizes out of
 * range); its contents on entry do not matter.
 *
 * Limits: those of ibgs_resample.h (1 <= S <= IBGS_RSZ_MAX_SRC; sides 1 .. IBGS_RSZ_MAX_SIDE).
 */
#ifndef IBGS_RESAMPLE_TRAIN_H
#define IBGS_RESAMPLE_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t ibgs_rzt_required_scratch(int64_t S, int64_t H, int64_t W, int64_t Hr, int64_t Wr);

/* grad_out: 38 x Hr x Wr.  grad_render: 3 x H x W; grad_warped: S x 3 x H x W; grad_w1 (32 x 7), grad_b1 (32), grad_w2 (32 x 32), grad_b2 (32). */
int32_t ibgs_rzt_features_backward(void* stream, int32_t S, int32_t H, int32_t W, int32_t Hr, int32_t Wr, int32_t mode, const float* render, const float* warped,
                                   const float* cam_feat, const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* levels,
                                   const float* grad_out, float* grad_render, float* grad_warped, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                                   void* scratch, size_t scratch_bytes);

/* grad_residual_out, grad_image_pred: 3 x H x W (either may be null); grad_residual_r: 3 x Hr x Wr. */
int32_t ibgs_rzt_upsample_backward(void* stream, int32_t H, int32_t W, int32_t Hr, int32_t Wr, const float* grad_residual_out, const float* grad_image_pred,
                                   float* grad_residual_r);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_RESAMPLE_TRAIN_H */
