/*
 * ibgs_exposure.h -- C ABI of the exposure correction of the colour aggregation network in libibgs_rast.so (ibgs_amd/csrc/exposure.hip): the reference's
 * compute_exposure_affine_matrix (color_aggregation_network.py:136-153, 182-185), i.e. the 3 x 4 affine colour map that takes the rendered image onto the
 * first warped source image in the least-squares sense over the pixels the rasterizer marked, and that map applied to the whole rendered image, with the
 * gradient of the application.  Python: ibgs_amd/exposure.py (`exposure_correct`).
 *
 * Images are float32, planes of H x W, contiguous: render (3 planes), warped (the 3 planes of slot 0 of warped_image: nothing behind them is read), mask
 * (1 plane of int32, the rasterizer's use_first_src_frame_mask).  A pixel takes part in the fit iff its mask word == 1.
 *   fit     A (3 x 4, row-major float32) minimises the sum over those pixels of |A [r; 1] - s|^2  (r: the rendered colour, s: the warped colour).
 *           Moments: one pass accumulates the IBGS_EXPO_SUMS = 22 distinct sums of the normal equations in f64 -- n; sum r (3); sum r r^T (6: 00 01 02 11 12
 *           22); sum s (3); sum s r^T (9: s-major) -- over quads of IBGS_EXPO_PIXELS_PER_THREAD consecutive pixels: thread t of the grid takes quads t,
 *           t + grid threads, ..., the pixels of a quad in order; pixels outside the mask are skipped (their values never enter any arithmetic: a NaN
 *           there does not reach A).  Each workgroup reduces its threads (csrc/block_ops.h: block_reduce) and writes one partial of 22 f64 to the arena.
 *           Solve: one workgroup adds the partials in index order and solves the 4 x 4 system in f64: the Gram matrix of [r0 r1 r2 1] is scaled to a unit
 *           diagonal and eliminated (Gauss-Jordan) with diagonal pivoting (the largest remaining diagonal entry first, the lowest index among equals).
 *   status  1: A is the fit.  0: the fit is UNDETERMINED -- fewer than 4 pixels take part, a column of the design matrix is zero or not finite, a
 *           pivot of the scaled Gram matrix is not above IBGS_EXPO_PIVOT_MIN, or the solution is not finite -- and A is the
 *           identity map [I | 0].
 *   apply   out[i] = fma(A[i][2], x2, fma(A[i][1], x1, fma(A[i][0], x0, A[i][3]))) at every pixel; with status 0, out = in bit for bit.
 *   apply_backward   out[j] = fma(A[2][j], g2, fma(A[1][j], g1, A[0][j] g0)): the gradient of the application with respect to its input image (A is
 *           a constant, as under the reference's torch.no_grad(): the warped image and the mask get no gradient); with status 0, out = grad bit for bit.
 * The contract is a tolerance against a float64 restatement (tests/exposure_ref.py).  Promised bit for bit: the same arguments give
 * the same A, status and images on every call and stream, whatever the alignment of the planes (no float atomics; every order above is fixed by H x W).
 *
 * Conventions are those of ibgs_color_agg.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.  Arguments are validated before any HIP call.
 *
 * Limits: 1 <= H, W <= IBGS_EXPO_MAX_SIDE.
 */
#ifndef IBGS_EXPOSURE_H
#define IBGS_EXPOSURE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_EXPO_MAX_SIDE 65536
#define IBGS_EXPO_SUMS 22
/* the moments' grid: min(ceil(quads / IBGS_EXPO_THREADS), IBGS_EXPO_MAX_GROUPS) workgroups of IBGS_EXPO_THREADS threads, quads = ceil(H W / 4) */
#define IBGS_EXPO_THREADS 256
#define IBGS_EXPO_MAX_GROUPS 256
#define IBGS_EXPO_PIXELS_PER_THREAD 4
/* which kernels ibgs_expo_fit launches */
#define IBGS_EXPO_MOMENTS 1
#define IBGS_EXPO_SOLVE 2
#define IBGS_EXPO_FIT 3
/* a fit is determined iff every pivot of the unit-diagonal Gram matrix is above this */
#define IBGS_EXPO_PIVOT_MIN 1e-11

/* bytes of the scratch arena of ibgs_expo_fit for a frame of H x W (the workgroups' partial sums: IBGS_EXPO_SUMS f64 each, 128 bytes of slack for the
 * alignment); 0 when an argument is out of range */
size_t ibgs_expo_required_scratch(int64_t H, int64_t W);

/* affine_out (12 float32) and status_out (1 int32) as above.  phases: IBGS_EXPO_FIT; IBGS_EXPO_MOMENTS fills the arena only (affine_out and status_out may
 * be null), IBGS_EXPO_SOLVE solves from an arena an earlier call filled for the same H x W (render, warped and mask may be null). */
int32_t ibgs_expo_fit(void* stream, int32_t H, int32_t W, const float* render, const float* warped, const int32_t* mask, float* affine_out,
                      int32_t* status_out, void* scratch, size_t scratch_bytes, int32_t phases);

/* out (3 x H x W, every element written) = A applied to image (3 x H x W); affine and status: the device words of ibgs_expo_fit (or ones the caller filled) */
int32_t ibgs_expo_apply(void* stream, int32_t H, int32_t W, const float* affine, const int32_t* status, const float* image, float* out);

/* grad_image (3 x H x W, every element written) = the transposed 3 x 3 block of A applied to grad_out (3 x H x W) */
int32_t ibgs_expo_apply_backward(void* stream, int32_t H, int32_t W, const float* affine, const int32_t* status, const float* grad_out, float* grad_image);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_EXPOSURE_H */
