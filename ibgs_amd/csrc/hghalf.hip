// The half-precision forward of the hourglass CNN (C ABI: include/ibgs_hg_half.h; Python: ibgs_amd/hourglass.py, precision="float16"): the network of
// hourglass.hip with the roundings of the reference's test-time run under torch.autocast(float16) -- x, weights, biases and the eight ReLU stages rounded to
// binary16 (to nearest even), every convolution a float32 accumulation of exact binary16 products on the matrix cores, `final` left in float32.  One packing
// launch (x and the weights into the arena), then seven launches of ONE templated 3 x 3 implicit-GEMM kernel; the last one carries the two 1 x 1
// convolutions and image_pred: d1 and f never reach memory.  The float32 boundary, the limits and the messages are those of ibgs_hg_forward.
//
// THE PRODUCTS are v_mfma_f32_16x16x32_f16: the tile, the lane map, a stage's layout in memory (pixel-major octets), the k order (free: the contract is a
// tolerance), the staged chunk and the chunk loop are csrc/shared/conv_tile_f16.h's, which hghtrain.hip runs too.  Padding costs products, which are cheap
// here: 38 channels run as 64, [38 | 38] as 96, 19 and 9 as 32 (DESIGN.md section 15 has the shares).
//
// KERNEL  hgh_conv3_kernel<CA, CB, COUT, MODE, FUSE>: 256 threads = 4 waves per 16 x 16 output tile on a 2-D uncapped grid; a wave owns four rows of the tile
// and all output channels.  The accumulators start from the rounded bias, cth_conv3 adds the convolution (the first input pooled, upsampled or plain as MODE
// says), and the epilogue clamps, rounds and stores.  No byte that was not written by this call reaches a product: the arena may hold anything before it.  In
// the last launch the accumulator tile, rounded, is the next product's B operand as it stands (cth_fuse_input, then `final` here), and hgh_pack_kernel lays
// the 1 x 1 weights out in that order.
#include "common.h"
#include "shared/hg_net.h"
#include "shared/conv_tile.h"
#include "shared/conv_tile_f16.h"
#include "../../include/ibgs_hourglass.h"
#include "../../include/ibgs_hg_half.h"

namespace ibgs {

constexpr int HGH_TILE = 16;                         // side of a workgroup's output tile: the names the launches below use, and the numbers the tests read here
constexpr int HGH_THREADS = 256;
static_assert(HGH_TILE == CT_TILE && HGH_THREADS == CT_THREADS, "the tile is conv_tile.h's");
constexpr int HGH_FIN_STEPS = 2;          // k-steps of final
// layer i of HG_LAYERS in the packed weights, which hold the nine in the order of the C ABI: its kind (0: 3 x 3; 1: fuse_input; 2: final), its fragments, its first one
constexpr int hgh_kind(int i) { return HG_LAYERS[i].side == 3 ? 0 : (i == HG_FINAL ? 2 : 1); }
constexpr int hgh_layer_frags(int i)
{
    const HgLayer& l = HG_LAYERS[i];
    return hgh_kind(i) == 0 ? cth_frags3(cth_octets(l.ca) + cth_octets(l.cb), l.cout) : (hgh_kind(i) == 1 ? CTH_FUSE_STEPS : HGH_FIN_STEPS) * ((l.cout + 15) / 16) * 64;
}
constexpr int hgh_at(int i) { return i == 0 ? 0 : hgh_at(i - 1) + hgh_layer_frags(i - 1); }
constexpr int HGH_FRAGS = hgh_at(HG_LAYER_COUNT);
static_assert((size_t)HGH_FRAGS * 16 == IBGS_HGH_PACKED_WEIGHT_BYTES, "the header's size of the packed weights");

// ---- the packing launch: h(x) pixel-major, and the nine layers' weights as operand fragments ---------------------------------------------------------------
struct HghPackLayer {
    const float* w;
    int cout, ca, cb;          // rows; channels of the two inputs ([a | b] along Cin)
    int first;                 // its first fragment
    int kind;                  // 0: 3 x 3; 1: fuse_input; 2: final
};
struct HghPackArgs {
    const float* x; cth_h8* xh; size_t pixels; unsigned x_blocks;
    cth_h8* packed;
    HghPackLayer layer[9];
};

__global__ void __launch_bounds__(HGH_THREADS) hgh_pack_kernel(const HghPackArgs a)
{
    if (blockIdx.x < a.x_blocks) {          // (uniform over the workgroup)
        const size_t p = (size_t)blockIdx.x * HGH_THREADS + threadIdx.x;
        if (p >= a.pixels) return;
#pragma unroll
        for (int o = 0; o < CTH_XO; ++o) {
            cth_h8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 8 * o + j < HG_C ? (_Float16)a.x[(size_t)(8 * o + j) * a.pixels + p] : (_Float16)0.0f;
            a.xh[p * CTH_XO + o] = v;
        }
        return;
    }
    const int i = (int)(blockIdx.x - a.x_blocks) * HGH_THREADS + (int)threadIdx.x;
    if (i >= HGH_FRAGS) return;
    HghPackLayer L = a.layer[0];
#pragma unroll
    for (int n = 1; n < 9; ++n)
        if (i >= a.layer[n].first) L = a.layer[n];          // (selects: the table is never indexed by a register)
    const int local = i - L.first, lane = local & 63, rest = local >> 6, kq = lane >> 4;
    cth_h8 v;
    if (L.kind == 0) {
        const int mtn = (L.cout + 15) / 16;
        const int mt = rest % mtn, t = (rest / mtn) % 9, c = rest / (mtn * 9), m = mt * 16 + (lane & 15), o = 4 * c + kq;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = cth_frag3_channel(o, j, L.ca, L.cb);
            v[j] = (m < L.cout && idx >= 0) ? (_Float16)L.w[((size_t)m * (L.ca + L.cb) + idx) * 9 + t] : (_Float16)0.0f;
        }
    } else {
        const int mtn = L.kind == 1 ? 3 : 1, mt = rest % mtn, s = rest / mtn, m = mt * 16 + (lane & 15), cin = L.ca + L.cb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = cth_frag1_channel(s, kq, j, L.ca, L.cb);
            v[j] = (m < L.cout && idx >= 0) ? (_Float16)L.w[(size_t)m * cin + idx] : (_Float16)0.0f;
        }
    }
    a.packed[i] = v;
}

// ---- the convolution ------------------------------------------------------------------------------------------------------------------------------------
struct HghArgs {
    const _Float16* a; const _Float16* b;          // the two inputs ([a | b] along the channels), pixel-major; b may be null when CB == 0
    const cth_h8* wfrag; const float* bias;        // the layer's packed weights; its float32 bias (COUT), rounded here
    _Float16* out;                                 // h x w pixels of CPOUT channels (null in the last launch)
    int h, w, hs, ws;                              // the output's resolution, and a's
    // the last launch: h(x) pixel-major, x (38 float32 planes), the packed fuse_input and final, the two outputs
    const _Float16* xh; const float* x; const cth_h8* fuse_frag; const float* fuse_b; const cth_h8* final_frag; const float* final_b;
    float burned; float* residual; float* image_pred;
};

template <int CA, int CB, int COUT, int MODE, bool FUSE>
__global__ void __launch_bounds__(HGH_THREADS, 2) hgh_conv3_kernel(const HghArgs a)
{
    constexpr int MT = (COUT + 15) / 16, CPOUT = 8 * cth_octets(COUT);
    static_assert(!FUSE || (COUT == HG_C && MT == 3), "the last launch is dec1");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int tx0 = blockIdx.x * HGH_TILE, ty0 = blockIdx.y * HGH_TILE;
    const int h = a.h, w = a.w;

    ct_f32x4 acc[MT][CT_ROWS];
    cth_start<COUT>(acc, a.bias, kq);
    cth_conv3<CA, CB, COUT, MODE>(acc, a.a, a.b, a.wfrag, h, w, a.hs, a.ws);

    const int x = tx0 + col;
    const size_t plane = (size_t)h * (size_t)w;
    if constexpr (!FUSE) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int c0 = mt * 16 + kq * 4;
            if (c0 < CPOUT) {          // (whole groups of four: CPOUT is a multiple of 8)
#pragma unroll
                for (int nt = 0; nt < CT_ROWS; ++nt) {
                    const int y = ty0 + wave * CT_ROWS + nt;
                    cth_h4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = (c0 + r < COUT && acc[mt][nt][r] > 0.0f) ? (_Float16)acc[mt][nt][r] : (_Float16)0.0f;          // padding channels: zeros
                    if (y < h && x < w) *reinterpret_cast<cth_h4*>(a.out + ((size_t)y * w + x) * CPOUT + c0) = v;
                }
            }
        }
    } else {
        // acc is d1 before its ReLU and rounding (padding channels: exact zeros).  fuse_input on [d1, h(x)], then final on f, the weights in the k order the
        // registers give, read from the arena as fragments.
        ct_f32x4 f[3][CT_ROWS];
        cth_fuse_input<true>(f, acc, a.fuse_frag, a.fuse_b, a.xh, h, w);
        ct_f32x4 res[CT_ROWS];
        {
            ct_f32x4 start;
#pragma unroll
            for (int r = 0; r < 4; ++r) start[r] = kq * 4 + r < 3 ? cth_round(a.final_b[min(kq * 4 + r, 2)]) : 0.0f;
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) res[nt] = start;
        }
#pragma unroll
        for (int s = 0; s < HGH_FIN_STEPS; ++s) {
            const cth_h8 av = a.final_frag[s * 64 + lane];
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) res[nt] = cth_mfma(av, cth_as_operand<3, true>(f, nt, s), res[nt]);
        }
        if (kq == 0) {          // rows 0 .. 2 of the result tile: the three colour channels, unrounded
#pragma unroll
            for (int nt = 0; nt < CT_ROWS; ++nt) {
                const int y = ty0 + wave * CT_ROWS + nt;
                if (y < h && x < w) {
                    const size_t p = (size_t)y * w + x;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        a.residual[(size_t)ch * plane + p] = res[nt][ch];
                        if (a.image_pred) a.image_pred[(size_t)ch * plane + p] = hg_blend(a.burned, a.x[(size_t)(HG_C - 3 + ch) * plane + p], res[nt][ch]);
                    }
                }
            }
        }
    }
}

struct HghScratch {          // the arena of the header, in its order: h(x), the six stages (both pixel-major octets), the packed weights
    _Float16* xh;
    HgStages<_Float16> s;
    cth_h8* packed;
    size_t bytes;
    HghScratch(char* base, size_t H, size_t W)
    {
        Carver c(base);
        xh = c.take<_Float16>(8 * CTH_XO * H * W);
        s = hg_carve_stages<_Float16>(c, H, W, 8);
        packed = c.take<cth_h8>(HGH_FRAGS);
        bytes = hg_carved_bytes(c, base);
    }
};

template <int CA, int CB, int COUT, int MODE, bool FUSE>
static void hgh_launch(hipStream_t st, const HghArgs& a)
{
    const dim3 grid((unsigned)((a.w + HGH_TILE - 1) / HGH_TILE), (unsigned)((a.h + HGH_TILE - 1) / HGH_TILE));
    hipLaunchKernelGGL((hgh_conv3_kernel<CA, CB, COUT, MODE, FUSE>), grid, dim3(HGH_THREADS), 0, st, a);
}

static HghArgs hgh_layer(const _Float16* in_a, const _Float16* in_b, const cth_h8* wfrag, const float* bias, _Float16* out, int h, int w, int hs, int ws)
{
    HghArgs a = {};
    a.a = in_a; a.b = in_b; a.wfrag = wfrag; a.bias = bias; a.out = out; a.h = h; a.w = w; a.hs = hs; a.ws = ws;
    return a;
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_hgh_required_scratch(int64_t H, int64_t W)
{
    return hg_shape_ok(nullptr, H, W) ? HghScratch(nullptr, (size_t)H, (size_t)W).bytes : 0;
}

int32_t ibgs_hgh_forward(void* stream, int32_t H, int32_t W, const float* x, const float* enc1_w, const float* enc1_b, const float* enc2_w,
                         const float* enc2_b, const float* enc3_w, const float* enc3_b, const float* up2_conv_w, const float* up2_conv_b,
                         const float* dec2_w, const float* dec2_b, const float* up1_conv_w, const float* up1_conv_b, const float* dec1_w,
                         const float* dec1_b, const float* fuse_input_w, const float* fuse_input_b, const float* final_w, const float* final_b,
                         float burned_in_gauss, float* residual, float* image_pred, void* scratch, size_t scratch_bytes)
{
    if (!hg_shape_ok("hgh_forward", H, W)) return -IBGS_ERR_INVALID;
    if (!x) { set_error("hgh_forward: null input"); return -IBGS_ERR_INVALID; }
    const float* const params[18] = {enc1_w, enc1_b, enc2_w, enc2_b, enc3_w, enc3_b, up2_conv_w, up2_conv_b, dec2_w, dec2_b, up1_conv_w, up1_conv_b, dec1_w, dec1_b,
                                     fuse_input_w, fuse_input_b, final_w, final_b};
    if (!hg_params_ok("hgh_forward", params)) return -IBGS_ERR_INVALID;
    if (!residual) { set_error("hgh_forward: null outputs: residual is required"); return -IBGS_ERR_INVALID; }
    const HghScratch sc(static_cast<char*>(scratch), (size_t)H, (size_t)W);
    if (!arena_ok("hgh_forward", "scratch", scratch, scratch_bytes, sc.bytes)) return -IBGS_ERR_INVALID;
    const HgStages<_Float16>& s = sc.s;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2;

    HghPackArgs pk = {};
    pk.x = x; pk.xh = reinterpret_cast<cth_h8*>(sc.xh); pk.pixels = (size_t)H * (size_t)W; pk.x_blocks = grid_for(pk.pixels, HGH_THREADS); pk.packed = sc.packed;
    for (int i = 0; i < HG_LAYER_COUNT; ++i) pk.layer[i] = {params[2 * i], HG_LAYERS[i].cout, HG_LAYERS[i].ca, HG_LAYERS[i].cb, hgh_at(i), hgh_kind(i)};
    hipLaunchKernelGGL(hgh_pack_kernel, dim3(pk.x_blocks + grid_for(HGH_FRAGS, HGH_THREADS)), dim3(HGH_THREADS), 0, st, pk);

    hgh_launch<38, 0, 38, CT_PLAIN, false>(st, hgh_layer(sc.xh, nullptr, sc.packed + hgh_at(HG_ENC1), enc1_b, s.e1, H, W, H, W));
    hgh_launch<38, 0, 19, CT_POOL, false>(st, hgh_layer(s.e1, nullptr, sc.packed + hgh_at(HG_ENC2), enc2_b, s.e2, H2, W2, H, W));
    hgh_launch<19, 0, 9, CT_POOL, false>(st, hgh_layer(s.e2, nullptr, sc.packed + hgh_at(HG_ENC3), enc3_b, s.b, H4, W4, H2, W2));
    hgh_launch<9, 0, 19, CT_UP, false>(st, hgh_layer(s.b, nullptr, sc.packed + hgh_at(HG_UP2_CONV), up2_conv_b, s.u2, H2, W2, H4, W4));
    hgh_launch<19, 19, 19, CT_PLAIN, false>(st, hgh_layer(s.u2, s.e2, sc.packed + hgh_at(HG_DEC2), dec2_b, s.d2, H2, W2, H2, W2));
    hgh_launch<19, 0, 38, CT_UP, false>(st, hgh_layer(s.d2, nullptr, sc.packed + hgh_at(HG_UP1_CONV), up1_conv_b, s.u1, H, W, H2, W2));
    HghArgs last = hgh_layer(s.u1, s.e1, sc.packed + hgh_at(HG_DEC1), dec1_b, nullptr, H, W, H, W);
    last.xh = sc.xh; last.x = x; last.fuse_frag = sc.packed + hgh_at(HG_FUSE_INPUT); last.fuse_b = fuse_input_b; last.final_frag = sc.packed + hgh_at(HG_FINAL); last.final_b = final_b;
    last.burned = burned_in_gauss; last.residual = residual; last.image_pred = image_pred;
    hgh_launch<38, 38, 38, CT_PLAIN, true>(st, last);
    IBGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
