/*
 * ibgs_hg_train.h -- C ABI of the backward of the hourglass CNN in libibgs_rast.so (ibgs_amd/csrc/hgtrain.hip): the gradients of the network of
 * ibgs_hourglass.h (whose notation this header keeps) for training.  Python: ibgs_amd/hourglass.py (`hourglass_backward`, `hourglass_train`,
 * `fuse_color_train`).  The forward of a training step is ibgs_hg_forward itself, on an arena the caller keeps until the backward has run.
 *
 * Inputs: x (38 planes of H x W), the eighteen parameters, the six saved stages e1, e2, b, u2, d2, u1 in the arena layout of ibgs_hg_forward (unchanged),
 * burned_in_gauss, and the upstream gradients grad_residual and / or grad_image_pred (3 planes of H x W each; either may be null, not both).
 *
 *   g  = grad_residual + grad_image_pred
 *   d1 = relu(conv3([u1, e1]; dec1)),  f = relu(conv1([d1, x]; fuse_input))           (recomputed, not saved)
 *   final:       dW = sum_p g (x) f,           db = sum_p g,    g_f   = (final_w^T g) [f > 0]
 *   fuse_input:  dW = sum_p g_f (x) [d1 | x],  db = sum_p g_f,  g_cat = fuse_input_w^T g_f
 *   G_d1 = g_cat[0:38] [d1 > 0];   g_x = g_cat[38:76];   g_x[35 + c] += burned_in_gauss grad_image_pred[c]
 * A 3 x 3 layer with input I (at the layer's resolution, zero outside) and pre-activation gradient G:
 *   dW[o, i, ky, kx] = sum_{y, x} G[o, y, x] I[i, y + ky - 1, x + kx - 1],   db[o] = sum G[o],
 *   g_I[i, y, x] = sum_{o, ky, kx} W[o, i, ky, kx] G[o, y - ky + 1, x - kx + 1]
 * pool^T: g_t[c, y, x] = g_pool[c, y / 2, x / 2] where (y, x) is the FIRST maximum of its 2 x 2 window in row-major order, else 0 (a dropped odd last row
 * or column gets 0).  up^T: g_t[c, y, x] = the sum of g_up[c, Y, X] over the (Y, X) whose nearest source under the integer rule of ibgs_hourglass.h is (y, x).
 *   G_d1 -> dec1:     g_u1, g_e1a             G_u1 = g_u1 [u1 > 0]
 *   G_u1 -> up1_conv: g_d2 = up^T(g_I)        G_d2 = g_d2 [d2 > 0]
 *   G_d2 -> dec2:     g_u2, g_e2a             G_u2 = g_u2 [u2 > 0]
 *   G_u2 -> up2_conv: g_b  = up^T(g_I)        G_b  = g_b [b > 0]
 *   G_b  -> enc3:     g_e2b = pool^T(g_I)     G_e2 = (g_e2a + g_e2b) [e2 > 0]
 *   G_e2 -> enc2:     g_e1b = pool^T(g_I)     G_e1 = (g_e1a + g_e1b) [e1 > 0]
 *   G_e1 -> enc1:     g_x += g_I
 * Outputs: grad_x (38 planes) and the eighteen parameter gradients, each in its parameter's layout.  Each GROUP is optional: grad_x null means no input
 * gradient (enc1's g_I is not computed); the eighteen gradient pointers all null means no parameter gradients (no weight-gradient kernel is launched).
 * Some of the eighteen null and some not is an error, and so is asking for nothing.
 *
 * Float32; every product (the 3 x 3 input gradients, the weight gradients, the recomputed dec1, the 1 x 1 products) runs on the matrix cores in exact f32.
 * The contract is a tolerance against a float64 restatement (tests/hourglass_bwd_ref.py).  Promised bit for bit: the same arguments
 * give the same results on every call and stream (no atomics: a weight gradient is summed from per-workgroup partials in a fixed order), and grad_x does
 * not depend on whether parameter gradients are asked for (nor the other way round).
 *
 * THE ARENA of the backward (scratch), each part at the next multiple of 128 bytes, with P = H W, P2 = H2 W2, P4 = H4 W4 floats per plane:
 *   A (38 P: d1, then G_u1), B (38 P: f, then g_e1a and G_e1 in place), C (38 P: g_f, then up1_conv's g_I), D (38 P: G_d1), g (3 P),
 *   G_d2 (19 P2), G_u2 (19 P2), E2 (19 P2: g_e2a, then G_e2 in place), up2_conv's g_I (9 P2), enc2's g_I (38 P2), G_b (9 P4), enc3's g_I (19 P4),
 *   and the weight-gradient partials: the largest layer's (strips x slices x padded rows x padded columns) floats.
 * ibgs_hgb_required_scratch is the end of the partials rounded up to 128 bytes.
 *
 * Conventions are those of ibgs_hourglass.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input (x, the parameters, the stages, the upstream gradients).  Arguments are validated before any HIP call.
 *
 * Limits: those of ibgs_hourglass.h.
 */
#ifndef IBGS_HG_TRAIN_H
#define IBGS_HG_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the arena of ibgs_hgb_backward for a frame of H x W (the layout above); 0 when an argument is out of range */
size_t ibgs_hgb_required_scratch(int64_t H, int64_t W);

/* stages_arena: the arena ibgs_hg_forward filled for these x and parameters (ibgs_hg_required_scratch(H, W) bytes, read only). */
int32_t ibgs_hgb_backward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                          const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                          const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                          const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                          float burned_in_gauss, const void* stages_arena, const float* grad_residual /* may be null */,
                          const float* grad_image_pred /* may be null */, float* grad_x /* may be null */, float* grad_enc1_w, float* grad_enc1_b,
                          float* grad_enc2_w, float* grad_enc2_b, float* grad_enc3_w, float* grad_enc3_b, float* grad_up2_conv_w, float* grad_up2_conv_b,
                          float* grad_dec2_w, float* grad_dec2_b, float* grad_up1_conv_w, float* grad_up1_conv_b, float* grad_dec1_w, float* grad_dec1_b,
                          float* grad_fuse_input_w, float* grad_fuse_input_b, float* grad_final_w, float* grad_final_b, void* scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_HG_TRAIN_H */
