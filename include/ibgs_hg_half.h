/*
 * ibgs_hg_half.h -- C ABI of the half-precision forward of the hourglass CNN in libibgs_rast.so (ibgs_amd/csrc/hghalf.hip): the network of
 * ibgs_hourglass.h with the roundings of the reference's test-time run under torch.autocast(float16) (render.py:137-147, its default).  Python:
 * ibgs_amd/hourglass.py (`hourglass_forward(..., precision="float16")`, and the same keyword on `HourglassCNN`, `ColorAggregationNet`, `fuse_color`).
 *
 * THE BOUNDARY IS FLOAT32: x (38 planes of H x W, contiguous), the eighteen parameters (nn.Conv2d layout) and both outputs are float32, exactly as in
 * ibgs_hourglass.h, whose definitions of conv3, conv1, pool and up hold here.  THE OPERATION, with h(.) = rounding to binary16, to nearest even
 * (overflow becomes +-inf, as in torch):
 *   e1 = h(relu(conv3(h(x);            h(enc1))))         e2 = h(relu(conv3(pool(e1);  h(enc2))))      b  = h(relu(conv3(pool(e2);    h(enc3))))
 *   u2 = h(relu(conv3(up(b);           h(up2_conv))))     d2 = h(relu(conv3([u2, e2];  h(dec2))))      u1 = h(relu(conv3(up(d2);      h(up1_conv))))
 *   d1 = h(relu(conv3([u1, e1];        h(dec1))))         f  = h(relu(conv1([d1, h(x)]; h(fuse_input))))
 *   residual   = conv1(f; h(final))                       NOT rounded: the float32 accumulator (the reference rounds it to binary16)
 *   image_pred = burned_in_gauss * x[35 .. 37] + residual  with the UNROUNDED float32 x, the product rounded to float32 first: bit for bit torch's
 *                                                          expression on the returned residual
 * h(layer) rounds the weight and the bias.  Every convolution is a float32 accumulation on the matrix cores (v_mfma_f32_16x16x32_f16: exact products
 * of binary16 operands) started from the rounded bias; pool, up and the concatenations are exact.  The order of the sum is not part of the contract: the
 * contract is a tolerance against a float64 restatement, with torch's own autocast run of the network as the yardstick ("Half
 * precision"; tests/hghalf_ref.py).  Promised bit for bit: the same arguments give the same results on every call and stream (no atomics, nothing
 * crosses a workgroup), and image_pred is the float32 expression above.
 *
 * THE ARENA (uninitialised memory is fine: every byte that is read has been written by the call) holds, each at the next multiple of 128 bytes,
 *   xh (40), e1 (40), e2 (24), b (16), u2 (24), d2 (24), u1 (40), then the packed weights (IBGS_HGH_PACKED_WEIGHT_BYTES)
 * where a stage of C channels at h x w is PIXEL-MAJOR binary16 with the channels innermost and padded to CP = 8 ceil(C / 8), the number in brackets:
 * element (c, y, x) is at ((y w + x) CP + c); the padding channels are written as zeros.  xh is h(x) in that layout.  Resolutions as in
 * ibgs_hourglass.h: e1, u1, xh at H x W; e2, u2, d2 at H / 2 x W / 2; b at H / 4 x W / 4.  d1 and f never reach memory.  After the call the caller may
 * read the stages there.  The packed weights are the matrix-core operand fragments of the nine layers, rounded to binary16, zero where a row or a k is
 * padding; their order is private to hghalf.hip.
 *
 * The library keeps NO STATE: one small packing launch per call rounds x and the weights into the arena (hgh_pack_kernel), then seven launches of the
 * convolution kernel.  Conventions, limits (IBGS_HG_MIN_SIDE <= H, W <= IBGS_HG_MAX_SIDE, 38 channels), error codes and messages are those of
 * ibgs_hg_forward, with "hgh_forward" as the name; arguments are validated before any HIP call; the library never waits for the device and never
 * writes an input.
 */
#ifndef IBGS_HG_HALF_H
#define IBGS_HG_HALF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the packed weights at the end of the arena: 17600 fragments of eight binary16 */
#define IBGS_HGH_PACKED_WEIGHT_BYTES 281600

/* bytes of the arena of ibgs_hgh_forward for a frame of H x W (the layout above); 0 when an argument is out of range */
size_t ibgs_hgh_required_scratch(int64_t H, int64_t W);

/* residual: 3 x H x W float32, every element written; image_pred: the same, or null.  Eight kernels on `stream`. */
int32_t ibgs_hgh_forward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                         const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                         const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                         const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                         float burned_in_gauss, float* residual, float* image_pred /* may be null */, void* scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_HG_HALF_H */
