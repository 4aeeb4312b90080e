/*
 * ibgs_hg_half_train.h -- C ABI of the half-precision backward of the hourglass CNN in libibgs_rast.so (ibgs_amd/csrc/hghtrain.hip): the operation of
 * ibgs_hg_train.h (whose notation this header keeps) with binary16 operands on v_mfma_f32_16x16x32_f16, for mixed-precision training.  Python:
 * ibgs_amd/hourglass.py (`hourglass_backward` and `hourglass_train` with precision="float16"; `fuse_color_train` and
 * ibgs_amd/resample_train.py's `fuse_color_train_scaled` inside `train_precision("float16")`).
 *
 * THE FORWARD of a training step is ibgs_hgh_forward (ibgs_hg_half.h) itself, on an arena the caller keeps until the backward has run: residual and
 * image_pred are the test-time half forward's bit for bit, and the kept activations are its h(x) and its six binary16 stages e1, e2, b, u2, d2, u1.
 *
 * THE BOUNDARY IS FLOAT32 on both sides: x (38 planes of H x W), the eighteen parameters and the upstream gradients come in as float32; grad_x and the
 * eighteen parameter gradients leave as float32.  THE OPERATION, with h(.) = rounding to binary16, to nearest even (a cast; overflow becomes +-inf),
 * S = 2^k the scale (below) and every product an exact binary16 x binary16 product accumulated in float32 on the matrix cores:
 *   1. g = grad_residual + grad_image_pred in float32 (one of them alone when the other is null).   gS = h(S g).
 *      g_x[35 + c] += burned_in_gauss grad_image_pred[c] stays float32 and unscaled.
 *   2. d1 = h(relu(conv3([u1, e1]; h(dec1)))),  f = h(relu(conv1([d1, h(x)]; h(fuse_input))))  are RECOMPUTED, in the k order of ibgs_hgh_forward
 *      (the same bits), and written to the backward's arena; they are not kept by the forward.
 *   3. final:       dW = sum_p gS (x) f,              db = sum_p gS,   G_f  = h((h(final_w)^T gS) [f > 0])
 *      fuse_input:  dW = sum_p G_f (x) [d1 | h(x)],   db = sum_p G_f,  g_cat = h(fuse_input_w)^T G_f
 *      G_d1 = h(g_cat[0:38] [d1 > 0]);   g_x = 2^-k g_cat[38:76]  (float32, not rounded to binary16)
 *   4. a 3 x 3 layer with input I (binary16: a stage, pooled or upsampled as the forward reads it, or h(x)) and pre-activation gradient G (binary16):
 *      dW[o, i, ky, kx] = sum_{y, x} G[o, y, x] I[i, y + ky - 1, x + kx - 1],   db[o] = sum G[o]       (a GEMM over the pixels)
 *      g_I[i, y, x] = sum_{o, ky, kx} h(W)[o, i, ky, kx] G[o, y - ky + 1, x - kx + 1]                  (the forward's implicit GEMM, weight transposed and flipped)
 *      g_I is a float32 accumulation.  Each pre-activation gradient G_* is rounded to binary16 ONCE, after the mask and after any skip sum (which is
 *      added in float32); the masks come from the binary16 stages; pool^T and up^T are the gathers of ibgs_hg_train.h (first maximum in row-major
 *      order; the integer nearest rule), summed in float32:
 *        G_u1 = h(g_u1 [u1 > 0])   G_d2 = h(up^T(g_I) [d2 > 0])   G_u2 = h(g_u2 [u2 > 0])   G_b = h(up^T(g_I) [b > 0])
 *        G_e2 = h((g_e2a + pool^T(g_I)) [e2 > 0])                 G_e1 = h((g_e1a + pool^T(g_I)) [e1 > 0])
 *   5. weight gradients, bias gradients and grad_x are NOT rounded to binary16: they leave as the float32 accumulation times 2^-k.  A weight gradient is
 *      one float32 partial per workgroup, summed in the order of the workgroups (in double) and scaled; no float atomics.  The same arguments give the
 *      same bits on every call and stream; grad_x does not depend on whether parameter gradients are asked for, nor the other way round.
 *
 * THE SCALE  k = grad_scale_log2 when scale_mode is IBGS_HGHT_SCALE_FIXED.  With IBGS_HGHT_SCALE_AUTO one reduction launch finds m = max |g| over the
 * upstream and writes k = IBGS_HGHT_E_TARGET - floor(log2 m) to a device word that every later launch reads (no host synchronisation); m zero or
 * non-finite gives k = 0.  The scale is internal and exact (a power of two): the caller sees true gradients and needs no loss scaling of its own.
 * status (optional, two int32 on the device): status[0] = the k that was used, status[1] = the number of non-finite binary16 gradient values that were
 * stored (gS and the nine G_*).  Overflow is never hidden: non-finite values propagate into the float32 outputs.
 *
 * THE ARENA of the backward (scratch; uninitialised memory is fine), each part at the next multiple of 128 bytes, P = H W, P2, P4 the pixels of the
 * three levels; "h" binary16 and "f" float32 values per pixel, pixel-major with the channels innermost and padded to a multiple of 8:
 *   control (128 bytes: max |g| as bits, k, the non-finite count, the reduction's ticket), d1 (40 h P), f (40 h P), G_f then G_u1 (40 h P),
 *   G_d1 then G_e1 (40 h P), gS (8 h P), g_e1a (40 f P), up1_conv's g_I (24 f P), G_d2 (24 h P2), G_u2 (24 h P2), G_e2 (24 h P2),
 *   g_e2a (24 f P2), up2_conv's g_I (16 f P2), enc2's g_I (40 f P2), G_b (16 h P4), enc3's g_I (24 f P4), the packed weights
 *   (IBGS_HGHT_PACKED_WEIGHT_BYTES: operand fragments, private to hghtrain.hip) and the weight-gradient partials.
 * After the call d1 and f lie at bytes 128 and 128 + (80 P rounded up to 128): the ReLU decisions the backward used.
 *
 * Each GROUP of outputs is optional as in ibgs_hg_train.h.  Conventions, limits and messages are those of ibgs_hgb_backward, with "hgh_train_backward"
 * as the name.  No inline assembly; coordinates are clamped into the frame before an offset is formed, every load is unconditional and zero is selected
 * afterwards; no address outside a stage or the arena is formed.
 */
#ifndef IBGS_HG_HALF_TRAIN_H
#define IBGS_HG_HALF_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the exponent the largest scaled upstream magnitude is brought to: S max |g| lies in [2^E_TARGET, 2^(E_TARGET + 1)) (DESIGN.md section 15 has the table) */
#define IBGS_HGHT_E_TARGET 10
#define IBGS_HGHT_SCALE_AUTO 0
#define IBGS_HGHT_SCALE_FIXED 1
/* bytes of the packed weights in the arena: 25344 fragments of eight binary16 */
#define IBGS_HGHT_PACKED_WEIGHT_BYTES 405504

/* bytes of the arena of ibgs_hgh_train_backward for a frame of H x W (the layout above); 0 when an argument is out of range */
size_t ibgs_hgh_train_required_scratch(int64_t H, int64_t W);

/* forward_arena: the arena ibgs_hgh_forward filled for these x and parameters (ibgs_hgh_required_scratch(H, W) bytes, read only: its h(x) and its six stages). */
int32_t ibgs_hgh_train_backward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                                const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                                const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                                const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                                float burned_in_gauss, const void* forward_arena, const float* grad_residual /* may be null */,
                                const float* grad_image_pred /* may be null */, int32_t scale_mode, int32_t grad_scale_log2, int32_t* status /* may be null */,
                                float* grad_x /* may be null */, float* grad_enc1_w, float* grad_enc1_b, float* grad_enc2_w, float* grad_enc2_b,
                                float* grad_enc3_w, float* grad_enc3_b, float* grad_up2_conv_w, float* grad_up2_conv_b, float* grad_dec2_w,
                                float* grad_dec2_b, float* grad_up1_conv_w, float* grad_up1_conv_b, float* grad_dec1_w, float* grad_dec1_b,
                                float* grad_fuse_input_w, float* grad_fuse_input_b, float* grad_final_w, float* grad_final_b, void* scratch,
                                size_t scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_HG_HALF_TRAIN_H */
