// The resampling rule of the reduced-resolution colour tail, stated once for the two units that run it: resample.hip (the forward: the gather of the features
// and the upsampling of the residual) and rsztrain.hip (their adjoints, which recompute the forward's taps and blends and must find the same bits).  The
// definition is include/ibgs_resample.h: align_corners = True, the tap's index and remainder in integers, the value as three fma.  With it the check of the two
// frames' sides that every entry point of both units makes.  ibgs_amd/_build.py lists this header under the two units (UNIT_HEADERS) and no other: it sits in
// a subdirectory of csrc/ so that no other unit's profile stamp holds it.
#pragma once
#include "../common.h"
#include "../../../include/ibgs_resample.h"

namespace ibgs {

// One axis of the coordinate rule: the two taps of output index i of an `out`-long axis made of an `in`-long one, t and 1 - t.  (i (in - 1) < 2^32: both
// sides are at most 65536.)
struct RszTap { uint32_t i0, i1; float t, u; };
__device__ __forceinline__ RszTap rsz_tap(uint32_t i, uint32_t in, uint32_t out)
{
    const uint32_t den = out > 1u ? out - 1u : 1u, num = out > 1u ? i * (in - 1u) : 0u;
    RszTap r;
    r.i0 = num / den;
    r.i1 = min(r.i0 + 1u, in - 1u);
    r.t = (float)(num - r.i0 * den) / (float)den;
    r.u = 1.0f - r.t;
    return r;
}

// the value rule on the taps a, b (row y0) and c, d (row y1)
__device__ __forceinline__ float rsz_blend(float a, float b, float c, float d, const RszTap& ty, const RszTap& tx)
{
    const float top = fmaf(tx.t, b, tx.u * a), bottom = fmaf(tx.t, d, tx.u * c);
    return fmaf(ty.t, bottom, ty.u * top);
}

// who == nullptr: silent (a size query)
inline bool rsz_sides_ok(const char* who, int64_t H, int64_t W, int64_t Hr, int64_t Wr)
{
    if (H < 1 || W < 1 || H > IBGS_RSZ_MAX_SIDE || W > IBGS_RSZ_MAX_SIDE) {
        if (who) set_error("%s: a frame of %lld x %lld is out of range (sides 1 .. %d)", who, (long long)H, (long long)W, IBGS_RSZ_MAX_SIDE);
        return false;
    }
    if (Hr < 1 || Wr < 1 || Hr > IBGS_RSZ_MAX_SIDE || Wr > IBGS_RSZ_MAX_SIDE) {
        if (who) set_error("%s: a reduced frame of %lld x %lld is out of range (sides 1 .. %d)", who, (long long)Hr, (long long)Wr, IBGS_RSZ_MAX_SIDE);
        return false;
    }
    return true;
}

}  // namespace ibgs
