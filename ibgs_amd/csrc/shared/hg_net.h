// The hourglass CNN of the colour aggregation network, stated once for the four units that run it: hourglass.hip (the float32 forward), hgtrain.hip (the
// backward, which reads the forward's arena), hghalf.hip (the half-precision forward) and hghtrain.hip (the half-precision backward, which reads that one's arena).  The definition is include/ibgs_hourglass.h:
//   e1 = relu(conv3(x; enc1 38 -> 38))            e2 = relu(conv3(pool(e1); enc2 38 -> 19))       b = relu(conv3(pool(e2); enc3 19 -> 9))
//   u2 = relu(conv3(up(b); up2_conv 9 -> 19))     d2 = relu(conv3([u2, e2]; dec2 38 -> 19))       u1 = relu(conv3(up(d2); up1_conv 19 -> 38))
//   d1 = relu(conv3([u1, e1]; dec1 76 -> 38))     f = relu(conv1([d1, x]; fuse_input 76 -> 38))   residual = conv1(f; final 38 -> 3)
// e1, e2, u2, d2, u1 and b are the STAGES: the outputs of the first six layers, at level 0 (H x W), 1 (H / 2 x W / 2) or 2 (H / 2 / 2 x W / 2 / 2).  THE ARENA
// of a forward holds them in the order of their layers -- e1, e2, b, u2, d2, u1 -- each at the next multiple of 128 bytes; d1 and f never reach memory.
// Host code and what lies outside a kernel body only.  The geometry of the float32 kernels (tile, threads, window, staged planes), their lane map and the rule
// by which a layer reads its first input (a kernel's MODE: CT_PLAIN, CT_POOL, CT_UP) are conv_tile.h's, next to this file; the half-precision kernels' staging
// is conv_tile_f16.h's.  ibgs_amd/_build.py lists this header under the four units (UNIT_HEADERS) and no other: it sits in a subdirectory of csrc/ so that no
// other unit's profile stamp holds it.
#pragma once
#include "../common.h"
#include "../../../include/ibgs_hourglass.h"

namespace ibgs {

constexpr int HG_C = IBGS_HG_CHANNELS;

// the nine layers in the order of the C ABI: the rows of the weight, the channels of its two inputs ([a | b] along Cin), the kernel's side, the output's level
struct HgLayer { const char* name; int cout, ca, cb, side, level; };
enum { HG_ENC1, HG_ENC2, HG_ENC3, HG_UP2_CONV, HG_DEC2, HG_UP1_CONV, HG_DEC1, HG_FUSE_INPUT, HG_FINAL, HG_LAYER_COUNT };
constexpr int HG_STAGE_COUNT = 6;
constexpr HgLayer HG_LAYERS[HG_LAYER_COUNT] = {{"enc1", 38, 38, 0, 3, 0}, {"enc2", 19, 38, 0, 3, 1}, {"enc3", 9, 19, 0, 3, 2}, {"up2_conv", 19, 9, 0, 3, 1},
                                               {"dec2", 19, 19, 19, 3, 1}, {"up1_conv", 38, 19, 0, 3, 0}, {"dec1", 38, 38, 38, 3, 0},
                                               {"fuse_input", 38, 38, 38, 1, 0}, {"final", 3, 38, 0, 1, 0}};
static_assert(HG_LAYERS[HG_ENC1].ca == HG_C && HG_LAYERS[HG_DEC1].cout == HG_C && HG_LAYERS[HG_FINAL].ca == HG_C, "the literals above are IBGS_HG_CHANNELS");

// image_pred of one element: the product rounded before the sum (torch's two kernels), bit for bit
__device__ __forceinline__ float hg_blend(float burned, float render, float residual)
{
#pragma clang fp contract(off)
    const float scaled = burned * render;
    return scaled + residual;
}

// who == nullptr: silent (the size query)
inline bool hg_shape_ok(const char* who, int64_t H, int64_t W)
{
    if (H < IBGS_HG_MIN_SIDE || W < IBGS_HG_MIN_SIDE || H > IBGS_HG_MAX_SIDE || W > IBGS_HG_MAX_SIDE) {
        if (who) set_error("%s: a frame of %lld x %lld is out of range (sides %d .. %d)", who, (long long)H, (long long)W, IBGS_HG_MIN_SIDE, IBGS_HG_MAX_SIDE);
        return false;
    }
    return true;
}

// The eighteen parameters (or their gradients) of an entry point, in its order: entry i is HG_LAYERS[i / 2]'s hg_part(i).  -> the first null one, or -1
template <typename T>
inline int hg_first_null(T* const (&p)[2 * HG_LAYER_COUNT])
{
    for (int i = 0; i < 2 * HG_LAYER_COUNT; ++i)
        if (!p[i]) return i;
    return -1;
}
inline const char* hg_part(int i) { return i & 1 ? "bias" : "weight"; }
inline bool hg_params_ok(const char* who, const float* const (&params)[2 * HG_LAYER_COUNT])
{
    const int i = hg_first_null(params);
    if (i >= 0) set_error("%s: null parameters: %s's %s", who, HG_LAYERS[i / 2].name, hg_part(i));
    return i < 0;
}

// The stages of an arena: `pad` is the multiple a stage's channel count is rounded up to (1: float32 planes; 8: pixel-major binary16 octets).
template <typename T> struct HgStages { T *e1, *e2, *b, *u2, *d2, *u1; };
template <typename T>
inline HgStages<T> hg_carve_stages(Carver& c, size_t H, size_t W, size_t pad)
{
    const size_t pixels[3] = {H * W, (H / 2) * (W / 2), (H / 2 / 2) * (W / 2 / 2)};
    T* s[HG_STAGE_COUNT];
    for (int i = 0; i < HG_STAGE_COUNT; ++i) s[i] = c.take<T>((HG_LAYERS[i].cout + pad - 1) / pad * pad * pixels[HG_LAYERS[i].level]);
    return {s[0], s[1], s[2], s[3], s[4], s[5]};
}
// the bytes carved from `base` so far, rounded up to 128: an arena's required size
inline size_t hg_carved_bytes(const Carver& c, const void* base) { return ((c.cur + 127) & ~uintptr_t(127)) - reinterpret_cast<uintptr_t>(base); }

}  // namespace ibgs
