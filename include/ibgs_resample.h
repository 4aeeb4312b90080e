/*
 * ibgs_resample.h -- C ABI of the reduced-resolution colour tail in libibgs_rast.so (ibgs_amd/csrc/resample.hip): the two resampling steps of the
 * reference's fuse_color under `residual_resolution_scale != 1` (color_aggregation_network.py:200-239), for TEST-TIME rendering (forward only).
 * Python: ibgs_amd/resample.py (`scaled_size`, `resized_features`, `upsample_residual`) and the keyword `residual_resolution_scale` of
 * `hourglass.fuse_color`.
 *
 * SIZE RULE        Hr = floor(H s), Wr = floor(W s) in double precision (Python's int(H * s); F.interpolate(scale_factor = s)).  The caller forms them; the
 *                  entry points take the two sizes, so any s > 0 whose sizes are in range is served, upscaling included.
 * COORDINATE RULE  bilinear, align_corners = True, both ways.  Output row i of an `out`-row image made of an `in`-row one reads the source coordinate
 *                  y = i (in - 1) / (out - 1), or 0 when out == 1.  Formed in INTEGERS: y0 = (i (in - 1)) / (out - 1), rem = (i (in - 1)) % (out - 1),
 *                  y1 = min(y0 + 1, in - 1), t = (float)rem / (float)(out - 1): the taps are exact and t carries one rounding (torch forms y in float32:
 *                  its taps can be off by one at a whole-numbered y and its t carries the coordinate's ulp).  Columns alike.
 * VALUE            with taps a = (y0, x0), b = (y0, x1), c = (y1, x0), d = (y1, x1), float32, in this order:
 *                    top = fma(tx, b, (1 - tx) a);  bottom = fma(tx, d, (1 - tx) c);  value = fma(ty, bottom, (1 - ty) top)
 *                  (1 - t is rounded once; a weight of exactly 0 meets a finite tap: a value that is a tap is that tap bit for bit).
 *
 * ibgs_rsz_features_forward: what the CNN reads at Hr x Wr.  Images are float32 planes of H x W, contiguous, as in ibgs_color_agg.h: render (3), warped
 * (S x 3), cam_feat (S x 4), camera_ray (3); the parameters are w1 (32 x 7), b1 (32), w2 (32 x 32), b2 (32) in nn.Linear layout.  For the reduced pixel q:
 *   x(q, k)  = VALUE of x_full(., k) over the four taps, element by element, where x_full(p, k) is the slot definition of ibgs_color_agg.h evaluated at the
 *              FULL-RESOLUTION pixel p with its own mask: v = (((f0 + f1) + f2) + f3) > 0 in float32 in that order,
 *              x_full = [(warped[3k + c] - render[c]) v for c in 0..2, f0, f1, f2, f3].  The features are masked first and interpolated afterwards, as the
 *              reference does; interpolating the images first gives something else wherever the four taps differ in validity.
 *   h1 = relu(w1 x + b1), h2 = relu(w2 h1 + b2): f32 fma chains from the bias, the 32 terms of the second layer in the matrix cores' order
 *              (v_mfma_f32_32x32x2_f32, the instruction and the order of coloragg.hip).
 *   agg      = the mean of h2 over k < levels (IBGS_RSZ_MEAN: ((h2_0 + h2_1) + ..) / levels) or the maximum (IBGS_RSZ_MAX); 0 when levels == 0.
 *   ray      = r / (sqrt((r0 r0 + r1 r1) + r2 r2) + 1e-10f) with r = VALUE of camera_ray;  colour = VALUE of render.
 *   out      (38 planes of Hr x Wr) = [agg (32), ray (3), colour (3)], every element written.
 * `levels` is the device word of ibgs_cagg_levels, counted at FULL resolution as the reference counts it (values outside 0 .. S are clamped into it); the
 * host never reads it.
 *
 * ibgs_rsz_residual_upsample: residual_out (3 x H x W) = VALUE of residual_r (3 x Hr x Wr), and in the same pass
 *   image_pred_out = render_scale * render + residual_out   (a rounded product, then a rounded sum: bit for bit torch's expression on residual_out).
 *
 * The contract is a tolerance against a float64 restatement (tests/resample_ref.py).  Promised bit for bit: the same arguments give the
 * same results on every call and stream (no atomics, no scratch: every output element is one thread's own chain).
 *
 * Conventions are those of ibgs_color_agg.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.  Arguments are validated before any HIP call.
 *
 * Limits: 1 <= S <= IBGS_RSZ_MAX_SRC; 1 <= H, W, Hr, Wr <= IBGS_RSZ_MAX_SIDE.
 */
#ifndef IBGS_RESAMPLE_H
#define IBGS_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_RSZ_MAX_SRC 5
#define IBGS_RSZ_MAX_SIDE 65536
#define IBGS_RSZ_FEATURES 32
#define IBGS_RSZ_MEAN 0
#define IBGS_RSZ_MAX 1

/* out: 38 x Hr x Wr, every element written.  levels: the device word of ibgs_cagg_levels on the FULL-resolution warped planes (or one the caller filled). */
int32_t ibgs_rsz_features_forward(void* stream, int32_t S, int32_t H, int32_t W, int32_t Hr, int32_t Wr, int32_t mode, const float* render, const float* warped,
                                  const float* cam_feat, const float* camera_ray, const float* w1, const float* b1, const float* w2, const float* b2,
                                  const int32_t* levels, float* out);

/* residual_r: 3 x Hr x Wr; render, residual_out, image_pred_out: 3 x H x W.  16-byte stores where W % 4 == 0 and the full-resolution pointers are 16-byte
 * aligned, 4-byte ones otherwise: the same values either way. */
int32_t ibgs_rsz_residual_upsample(void* stream, int32_t H, int32_t W, int32_t Hr, int32_t Wr, const float* residual_r, const float* render, float render_scale,
                                   float* residual_out, float* image_pred_out);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_RESAMPLE_H */
