/*
 * ibgs_hourglass.h -- C ABI of the hourglass CNN of the colour aggregation network in libibgs_rast.so (ibgs_amd/csrc/hourglass.hip): the forward of the
 * reference's ConvDecoderAE(38) (color_aggregation_network.py:6-68) behind the per-view front end of ibgs_color_agg.h, for test-time rendering.  Python:
 * ibgs_amd/hourglass.py (`hourglass_forward`, `HourglassCNN`, `ColorAggregationNet`, `fuse_color`).
 *
 * x is 38 float32 planes of H x W, contiguous.  Every parameter is in nn.Conv2d layout (Cout, Cin, k, k) with a bias (Cout).  conv3 is a 3 x 3
 * cross-correlation with zero padding 1, conv1 is 1 x 1, pool a 2 x 2 maximum with stride 2 that drops an odd last row or column, and
 * up(t, (h, w))[y, x] = t[min(y hin / h, hin - 1), min(x win / w, win - 1)] in integers (nearest).  With H2 = H / 2 and H4 = H2 / 2 (W alike):
 *   e1 = relu(conv3(x;               enc1     38 -> 38))    H  x W
 *   e2 = relu(conv3(pool(e1);        enc2     38 -> 19))    H2 x W2
 *   b  = relu(conv3(pool(e2);        enc3     19 ->  9))    H4 x W4
 *   u2 = relu(conv3(up(b, (H2, W2)); up2_conv  9 -> 19))    H2 x W2
 *   d2 = relu(conv3([u2, e2];        dec2     38 -> 19))    H2 x W2
 *   u1 = relu(conv3(up(d2, (H, W));  up1_conv 19 -> 38))    H  x W
 *   d1 = relu(conv3([u1, e1];        dec1     76 -> 38))
 *   f  = relu(conv1([d1, x];         fuse_input 76 -> 38))
 *   residual   = conv1(f;            final    38 ->  3)     3 planes of H x W
 *   image_pred = burned_in_gauss * x[35 .. 37] + residual   (the product rounded to float32, then the sum)
 * Forward only, float32: every product runs on the matrix cores in exact f32 (multiply-add chains started from the bias).  The contract is a tolerance
 * against a float64 restatement (tests/hourglass_ref.py).  Promised bit for bit: the same arguments give the same results on every
 * call and stream (no atomics, nothing crosses a workgroup), and image_pred is the float32 expression above on the residual that is returned.
 *
 * THE ARENA holds the six intermediates as planes of their resolution, in this order, each at the next multiple of 128 bytes:
 *   e1 (38 H W floats), e2 (19 H2 W2), b (9 H4 W4), u2 (19 H2 W2), d2 (19 H2 W2), u1 (38 H W)
 * and ibgs_hg_required_scratch is the end of u1 rounded up to 128 bytes.  d1 and f never reach memory.  After the call the caller may read the stages there.
 *
 * Conventions are those of ibgs_color_agg.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state (the weights are laid out for the matrix cores
 * while they are staged, in every call), never waits for the device and never writes an input.  Arguments are validated before any HIP call.
 *
 * Limits: IBGS_HG_MIN_SIDE <= H, W <= IBGS_HG_MAX_SIDE; 38 channels only.
 */
#ifndef IBGS_HOURGLASS_H
#define IBGS_HOURGLASS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_HG_CHANNELS 38
#define IBGS_HG_MIN_SIDE 4
#define IBGS_HG_MAX_SIDE 8192

/* bytes of the arena of ibgs_hg_forward for a frame of H x W (the layout above); 0 when an argument is out of range */
size_t ibgs_hg_required_scratch(int64_t H, int64_t W);

/* residual: 3 x H x W, every element written; image_pred: the same, or null.  Seven kernels on `stream`. */
int32_t ibgs_hg_forward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                        const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                        const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                        const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                        float burned_in_gauss, float* residual, float* image_pred /* may be null */, void* scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_HOURGLASS_H */
