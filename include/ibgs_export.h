/*
 * ibgs_export.h -- C ABI of the frame export in libibgs_rast.so (ibgs_amd/csrc/export.hip): what the second loop of the reference's render.py
 * (render_set, lines 221-249) does to a rendered frame on the host -- torchvision's save_image rounding, the cv2 branch's truncation, the normal map,
 * the normalised residual, and colorize (utils/general_utils.py:153-184: two percentiles of the valid depths, a 256-entry colour table) -- as 8-bit
 * HWC images written on the device.  Python: ibgs_amd/frame_export.py.
 *
 * Inputs are float32 planes of H x W, contiguous (CHW); outputs are uint8, H x W x C interleaved (HWC), 4-byte aligned.  Every rule is the reference's
 * arithmetic operation by operation, each operation rounded to float32 and none contracted into an fma (tests/frame_export_ref.py restates them; the
 * contract is equality of every byte):
 *   ROUND     t = x * 255; t = t + 0.5; clamp to [0, 255]; truncate                       (torchvision.utils.save_image)
 *   TRUNCATE  t = clamp(x, 0, 1) * 255; truncate                                          (render.py:246, the cv2 branch)
 *   NORMAL    t = (x + 1) / 2; t = t * 255; clip to [0, 255]; truncate                    (render.py:234-237)
 *   RESIDUAL  m = max |x| over all planes of the image; t = |x| / m; then ROUND            (render.py:221-222, 244).  m == 0: the image is 0 and status bit 0
 *   COLORIZE  one plane v.  A pixel is invalid when v is NaN, v == invalid_val (when use_invalid_val), or its invalid_mask byte is not 0.
 *             vmin, vmax: given, or percentiles 2 and 85 of the valid pixels (below).  x = vmin != vmax ? (v - vmin) / (vmax - vmin) : v * 0;
 *             xa = x * 256; entry = xa == 256 ? 255 : xa < 0 ? 0 : xa >= 256 ? 255 : trunc(xa)  (matplotlib's lookup, bytes=True); pixel = lut[entry];
 *             x NaN (an infinite v): 0, 0, 0 (matplotlib's `bad` colour); invalid pixels: background.
 *   A NaN that reaches a clamp becomes 0 (the reference's cast of a NaN is undefined).  bgr: channels 0 and 2 change places.
 *   percentile  np.percentile's default rule as numpy 2.x evaluates it for a float32 array.  n valid values, q32 = float32(q) / float32(100) (formed by the
 *             caller): vi = float32(n - 1) * q32; lo = floor(vi); g = vi - lo; hi = min(lo + 1, n - 1); A, B = the lo-th and hi-th smallest valid values;
 *             result = g >= 0.5 ? B - (B - A) * (1 - g) : A + (B - A) * g.  The order statistics are exact (-0.0 counts as +0.0 and comes back as +0.0,
 *             denormals are kept; NaN is invalid -- the reference's percentile would be NaN).  n == 0: the result is 0 and status bit 1.  n <= 2^24.
 * The order statistics come from a radix select on an order-preserving 32-bit key, 11 + 11 + 10 bits: per pass one histogram launch (LDS histograms added
 * to a table in the arena with integer atomics: the same bits on every run) and one single-workgroup launch that scans the table and narrows every rank.
 *
 * Conventions are those of ibgs_exposure.h: device pointers, `stream` is a hipStream_t passed as void*, return value >= 0 on success, < 0 = -(IBGS_ERR_*)
 * with ibgs_last_error() holding the message.  The caller owns every array; the library keeps no state, never waits for the device and never writes an
 * input.  Arguments are validated before any HIP call.  The arena may hold anything on entry: the library zeroes what it accumulates into.
 *
 * Limits: 1 <= H, W <= IBGS_FEXP_MAX_SIDE, H W <= IBGS_FEXP_MAX_PIXELS; percentiles (a COLORIZE image without both vmin and vmax): H W <= IBGS_FEXP_MAX_SELECT.
 */
#ifndef IBGS_EXPORT_H
#define IBGS_EXPORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBGS_FEXP_MAX_SIDE 65536
#define IBGS_FEXP_MAX_PIXELS 1073741824
#define IBGS_FEXP_MAX_SELECT 16777216
#define IBGS_FEXP_MAX_IMAGES 8
#define IBGS_FEXP_MAX_Q 4
/* image modes */
#define IBGS_FEXP_ROUND 0
#define IBGS_FEXP_TRUNCATE 1
#define IBGS_FEXP_NORMAL 2
#define IBGS_FEXP_RESIDUAL 3
#define IBGS_FEXP_COLORIZE 4
/* status bits */
#define IBGS_FEXP_ZERO_RESIDUAL 1
#define IBGS_FEXP_NO_VALID 2

typedef struct ibgs_fexp_image {
    const float* src;      /* `channels` planes of H x W (COLORIZE: one) */
    uint8_t* dst;          /* H x W x channels bytes (COLORIZE: H x W x 3), every byte written */
    int32_t mode;
    int32_t channels;      /* 1 or 3 */
    int32_t bgr;           /* 3 channels only */
    int32_t reserved;
} ibgs_fexp_image;

typedef struct ibgs_fexp_frame {
    int32_t H, W;
    int32_t n_images;      /* 1 .. IBGS_FEXP_MAX_IMAGES; at most one RESIDUAL and one COLORIZE among them */
    int32_t reserved;
    ibgs_fexp_image images[IBGS_FEXP_MAX_IMAGES];
    /* COLORIZE */
    const uint8_t* lut;            /* 256 x 3 */
    const uint8_t* invalid_mask;   /* H x W bytes, or null */
    int32_t use_invalid_val;
    float invalid_val;
    int32_t have_vmin, have_vmax;  /* 0: the percentile q32[0] (vmin), q32[1] (vmax) of the valid pixels */
    float vmin, vmax;
    float q32[2];
    uint8_t background[4];         /* r, g, b, - */
    int32_t* status;               /* one device word, written by every call */
    void* scratch;                 /* ibgs_required_export(H, W) bytes; may be null when no image is RESIDUAL and none needs a percentile */
    size_t scratch_bytes;
} ibgs_fexp_frame;

size_t ibgs_fexp_sizeof_frame(void);

/* bytes of the arena of ibgs_fexp_frame and ibgs_fexp_percentile for H x W values (the select's tables and words; 128 bytes of slack); 0 when out of range */
size_t ibgs_required_export(int64_t H, int64_t W);

/* all images of a frame in one writer launch, behind the select chain when an image needs it */
int32_t ibgs_fexp_frame_u8(void* stream, const ibgs_fexp_frame* frame);

/* out[k], k < nq <= IBGS_FEXP_MAX_Q: the percentile q32[k] (a HOST array of float32(q) / float32(100), each in [0, 1]) of the valid ones among n values;
 * invalid_mask: n bytes or null; status: one device word (IBGS_FEXP_NO_VALID or 0) */
int32_t ibgs_fexp_percentile(void* stream, int64_t n, const float* values, const uint8_t* invalid_mask, int32_t use_invalid_val, float invalid_val,
                             int32_t nq, const float* q32, float* out, int32_t* status, void* scratch, size_t scratch_bytes);

/* out[i] = float32(ROUND(in[i])) / 255, n values: what reading back an 8-bit PNG of the image gives (metrics.py:24-34) */
int32_t ibgs_fexp_quantize(void* stream, int64_t n, const float* in, float* out);

#ifdef __cplusplus
}
#endif

#endif /* IBGS_EXPORT_H */
