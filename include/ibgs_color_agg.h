/*
 * ibgs_color_agg.h -- C ABI of the per-view front end of the colour aggregation network in libibgs_rast.so (ibgs_amd/csrc/coloragg.hip): what the
 * reference's fuse_color and ColorFusionResidualNet.forward do between the rasterizer's outputs and the input of the hourglass CNN
 * (color_aggregation_network.py:102-133, 156-198, 229-233), with its gradient.  Python: ibgs_amd/coloragg.py (`per_view_features`, `PerViewFrontEnd`,
 * `fuse_color_inputs`).
 *
 * Images are float32, planes of H x W, contiguous: render (3 planes, or the exposure-corrected image made of it), warped (S x 3 planes), cam_feat
 * (S x 4 planes), camera_ray (3 planes).  The parameters are those of nn.Sequential(Linear(7, 32), ReLU, Linear(32, 32), ReLU) in nn.Linear layout:
 * w1 (32 x 7), b1 (32), w2 (32 x 32), b2 (32).
 *   levels   = min(number of slots k whose 3 warped planes hold any value != 0, nb_visible_src_frames, S): a DEVICE word, read there by the other entry
 *              points (values outside 0 .. S are clamped into it).  The first `levels` slots are used.
 *   slot k of pixel p:  v = (((f0 + f1) + f2) + f3) > 0 on the four feature planes, float32, in that order;
 *                       x = [(warped[3k + c] - render[c]) v for c in 0..2, f0, f1, f2, f3];  h1 = relu(w1 x + b1);  h2 = relu(w2 h1 + b2)
 *              (an invalid slot is not skipped: it contributes the MLP of [0, 0, 0, f0 .. f3]).
 *   agg      = the mean of h2 over k < levels (IBGS_CAGG_MEAN) or the maximum (IBGS_CAGG_MAX); 0 when levels == 0.
 *   out      (38 planes) = [agg (32), camera_ray (3), render (3)].
 * Gradients: render, warped (all S slots written, zero from `levels` on) and the four parameters; none for cam_feat and camera_ray.  ReLU's derivative at 0
 * is 0; in IBGS_CAGG_MAX mode the gradient of a channel goes to the first slot that attains the maximum.
 * The contract is a tolerance against a float64 restatement (tests/coloragg_ref.py).  Promised bit for bit: the same arguments give
 * the same results on every call and stream (the parameter gradients are per-workgroup partial sums in the scratch arena, added in a fixed order, across
 * workgroups in f64; no float atomics).
 *
 * Conventions are those of ibgs_geo_loss.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.  Arguments are validated before any HIP call.
 *
 * Limits: 1 <= S <= IBGS_CAGG_MAX_SRC; 1 <= H, W <= IBGS_CAGG_MAX_SIDE; nb_visible_src_frames >= 1.
 */
#ifndef IBGS_COLOR_AGG_H
#define IBGS_COLOR_AGG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_CAGG_MAX_SRC 5
#define IBGS_CAGG_MAX_SIDE 65536
#define IBGS_CAGG_FEATURES 32
#define IBGS_CAGG_MEAN 0
#define IBGS_CAGG_MAX 1

/* bytes of the scratch arena of ibgs_cagg_levels and ibgs_cagg_backward for S sources of H x W (two counting words and the per-workgroup partial sums of the
 * parameter gradients: the backward's grid is capped, so the size does not grow with the frame beyond that cap; 128-byte aligned); 0 when an argument is
 * out of range */
size_t ibgs_cagg_required_scratch(int64_t S, int64_t H, int64_t W);

/* levels_out (1 int32) = min(slots of warped with any value != 0, nb_visible_src_frames, S).  One kernel behind a memset of the two counting words. */
int32_t ibgs_cagg_levels(void* stream, int32_t S, int32_t H, int32_t W, const float* warped, int32_t nb_visible_src_frames, int32_t* levels_out,
                         void* scratch, size_t scratch_bytes);

/* out: 38 x H x W, every element written.  levels: the device word of ibgs_cagg_levels (or one the caller filled). */
int32_t ibgs_cagg_forward(void* stream, int32_t S, int32_t H, int32_t W, int32_t mode, const float* render, const float* warped, const float* cam_feat,
                          const float* camera_ray, const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* levels, float* out);

/* grad_out: 38 x H x W.  Each of grad_render (3 x H x W), grad_warped (S x 3 x H x W), grad_w1, grad_b1, grad_w2, grad_b2 may be null: what is null is not
 * computed (with both image gradients null the input-gradient arithmetic is not run; with all four parameter gradients null the scratch is not used and
 * may be null).  h1 and h2 are recomputed from the inputs. */
int32_t ibgs_cagg_backward(void* stream, int32_t S, int32_t H, int32_t W, int32_t mode, const float* render, const float* warped, const float* cam_feat,
                           const float* w1, const float* b1, const float* w2, const float* b2, const int32_t* levels, const float* grad_out,
                           float* grad_render, float* grad_warped, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, void* scratch,
                           size_t scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_COLOR_AGG_H */
