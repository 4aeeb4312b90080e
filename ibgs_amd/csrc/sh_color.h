// The SH -> RGB evaluation of the forward (forward.cu:58-109, 280-286) as device code, shared by the translation units that launch it:
// preprocess.hip (sh_color_kernel, the standalone pass) and scan_sort.hip (the same waves riding in the depth sort's launches, see ShRide).
// Both are compiled with -ffp-contract=off (ibgs_amd/_build.py): the evaluation is the oracle's, operation by operation, and colours and
// clamp flags must stay bit-identical whichever kernel runs it.
#pragma once
#include "common.h"

namespace ibgs {

static __constant__ float kC0 = 0.28209479177387814f;
static __constant__ float kC1 = 0.4886025119029199f;
static __constant__ float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                    -1.0925484305920792f, 0.5462742152960396f};
static __constant__ float kC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                    0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                    -0.5900435899266435f};

struct PreParams {
    int P, D, M;
    const float* means3D; const float* scales; const float* rotations; const float* opacities;
    const float* shs; const float* shs_rest;          // shs_rest != nullptr: shs holds the DC coefficient (P x 1 x 3), shs_rest the other M - 1 (P x (M - 1) x 3)
    const float* cov3D_precomp; const float* colors_precomp; const float* all_map;
    const float* plane_normal; const float* plane_offset; int plane_mode;
    int inst0;          // batched views: index of this view's first instance in the per-instance outputs (view * P)
    int tile_row0;      // ... and its first row in the stacked tile grid (view * ceil(H/16))
    float scale_modifier;
    int depth_only;
    int32_t* radii;
    float* rec; float* depths; float* cov3D; uint32_t* tiles; uint4* fp; uint64_t* tmask_hi; uint8_t* clamped;
    uint64_t* alive64;      // split mode only (else nullptr): per wave of 64 Gaussians, who reaches a tile list
    uint32_t* sort_key; uint32_t* sort_val;
    int cull;
    uint32_t* zero_a; uint32_t zero_a_n; uint32_t* zero_b; uint32_t zero_b_n;      // words the next stages want zeroed (the depth sort's scratch, its counters)
    RenderedNote note;          // sh_color_kernel: note.host != nullptr -> workgroup 0 adds the tile sums up for the host first (common.h)
    uint32_t* tile_partial; int partial0; int partial_err;      // tiles touched per wave: this launch's first word; the word that follows ALL waves' words (the depth sort's error flag, zeroed here)
};

// ---- SH -> RGB as its own pass (forward.cu:58-109, 280-286) ------------------------------------------------------------------------
// One wave per 64 consecutive Gaussians.  Their coefficient rows are one contiguous 12 KB block (M = 16): the wave fetches it with twelve
// fully coalesced 1 KB loads (float4 per lane, all in flight together) -- skipping the 16-byte pieces of rows whose Gaussian reaches no
// tile list (culled, off screen: 40 % of C3; the preprocess kernel left a lane mask per wave) -- and transposes it through LDS in two
// rounds of 32 rows (rows padded to 52 words: conflict-free 16-byte accesses both ways; 6.5 KB per wave, so the register budget and not
// LDS sets the occupancy): round h parks rows 32h .. 32h + 31, lane 32h + r reads row r back.  Every load instruction covers one
// contiguous kilobyte, every cache line is fetched once.  In the step it runs at ~3 TB/s of useful bytes -- what a 100-200 MB read gets
// right after kernels that left the caches full of dirty lines (tests/csrc/probe_read_bw.hip "cold": 2.9 TB/s; 6.2 TB/s when nothing
// has to drain), whatever its occupancy or load shape (three variants measured, docs/EXPERIMENTS.md section 7).  The evaluation is the oracle's, operation by
// operation and in its order (every file that includes this one is compiled without contraction): colours and clamp flags stay bit-identical.  Writes quad 2 of
// the render record and the clamp bits.
constexpr int SHC_ROW = 52;          // LDS words per row: 48 coefficients + 4 words of padding
constexpr int SHC_WAVE_FLOATS = 32 * SHC_ROW;          // one wave's LDS stage
// One wave: Gaussians [64 wave, 64 wave + 64) cut at P.  s_sh: SHC_WAVE_FLOATS words of LDS private to the wave.
template <bool SPLIT>          // SPLIT: DC and rest coefficients in two arrays (ibgs_forward_args.shs_rest) -- its own instantiation, so that the combined layout's code stays what it was
__device__ __forceinline__ void sh_color_wave(const PreParams& p, const Cam& cam, int wave, float* s_sh)
{
    const int lane = threadIdx.x & 63;
    const int first = wave * 64;          // this wave's Gaussians: [first, first + 64) cut at P
    if (first >= p.P) return;
    const uint64_t alive_m = p.alive64[wave];          // wave-uniform
    if (alive_m == 0ull) return;
    const int i = min(first + lane, p.P - 1);
    const bool alive = (alive_m >> lane) & 1ull;
    const int D = p.D, M = p.M;
    const int nb = (D + 1) * (D + 1);
    const float px3 = p.means3D[3 * i], py3 = p.means3D[3 * i + 1], pz3 = p.means3D[3 * i + 2];
    float shv[48];
    if (SPLIT && M == 16 && first + 64 <= p.P) {
        // DC and the rest in two arrays (the reference model's `_features_dc` (P, 1, 3) and `_features_rest` (P, 15, 3) as they are: no torch.cat, no
        // second copy of 192 B per Gaussian).  Same scheme as below: the wave's 64 rows are one contiguous block per array -- 64 x 180 B = 720 float4 of
        // rest, 64 x 12 B = 48 float4 of DC, 768 = 12 x 64 pieces, all loads coalesced and in flight together -- parked in LDS in two rounds of 32 rows
        // (360 + 24 = 384 = 6 x 64 pieces per round) AS THEY LIE in memory (16-byte LDS stores, conflict-free); lane r then reads its row word by word:
        // the rows are 45 (and 3) words apart, odd strides, so the 64 lanes of every read hit distinct banks.  (Scattering the pieces into padded rows
        // instead -- word stores 4 apart -- ran into 8-way bank conflicts: sh_color 51 -> 83 us.)  Pieces that hold nothing a live Gaussian needs are skipped.
        const float4* rest4 = reinterpret_cast<const float4*>(p.shs_rest + (size_t)first * 45);
        const float4* dc4 = reinterpret_cast<const float4*>(p.shs + (size_t)first * 3);
        float4 v[12];
#pragma unroll
        for (int it = 0; it < 12; it++) {
            const int h = it / 6, qp = (it % 6) * 64 + lane;          // piece of round h
            if (qp < 360) {
                const int ra = (4 * qp) / 45, rb = (4 * qp + 3) / 45;          // the (at most two) rows the piece touches
                const bool need = nb > 1 && (((alive_m >> (32 * h + ra)) & 1ull) || ((alive_m >> (32 * h + rb)) & 1ull));
                v[it] = need ? rest4[360 * h + qp] : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const int ra = (4 * (qp - 360)) / 3, rb = (4 * (qp - 360) + 3) / 3;
                const bool need = (((alive_m >> (32 * h + ra)) & 3ull) != 0ull) || ((alive_m >> (32 * h + rb)) & 1ull);          // (a DC piece touches rows ra, ra + 1 [, rb])
                v[it] = need ? dc4[24 * h + (qp - 360)] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        float4* s_raw = reinterpret_cast<float4*>(s_sh);          // 384 float4 of this round: rest rows 0..31 (1440 words), then their DC (96 words)
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int it = 0; it < 6; it++) s_raw[it * 64 + lane] = v[h * 6 + it];
            if ((lane >> 5) == h) {
                const float* rr = s_sh + 45 * (lane & 31);
                const float* rd = s_sh + 1440 + 3 * (lane & 31);
                shv[0] = rd[0]; shv[1] = rd[1]; shv[2] = rd[2];
#pragma unroll
                for (int k = 0; k < 45; k++) shv[3 + k] = rr[k];
            }
        }
    } else if (SPLIT) {          // other coefficient counts / the last, partial wave: plain per-lane loads from the two arrays
        const float* sr = p.shs_rest + (size_t)i * (M - 1) * 3;
        const float* sd = p.shs + (size_t)i * 3;
#pragma unroll
        for (int k = 0; k < 48; k++) shv[k] = (alive && k < 3 * nb) ? (k < 3 ? sd[k] : sr[k - 3]) : 0.f;
    } else if (M == 16) {
        const float4* src = reinterpret_cast<const float4*>(p.shs) + (size_t)first * 12;
        const int nq = min(64, p.P - first) * 12;          // float4 pieces of this wave's block
        float4 v[12];
#pragma unroll
        for (int it = 0; it < 12; it++) {
            const int q = it * 64 + lane;
            const int row = q / 12, piece = q - row * 12;
            const bool ok = q < nq && ((alive_m >> row) & 1ull) && 4 * piece < 3 * nb;
            v[it] = ok ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int it = 0; it < 6; it++) {
                const int q = it * 64 + lane;          // piece index within this round's 32 rows
                const int row = q / 12, piece = q - row * 12;
                *reinterpret_cast<float4*>(s_sh + row * SHC_ROW + piece * 4) = v[h * 6 + it];
            }
            if ((lane >> 5) == h) {
                const float4* row4 = reinterpret_cast<const float4*>(s_sh + (lane & 31) * SHC_ROW);
#pragma unroll
                for (int k = 0; k < 12; k++) { const float4 q = row4[k]; shv[4 * k] = q.x; shv[4 * k + 1] = q.y; shv[4 * k + 2] = q.z; shv[4 * k + 3] = q.w; }
            }
        }
    } else {          // other coefficient counts: plain per-lane loads of the row's first 3 * nb floats
        const float* sh = p.shs + (size_t)i * M * 3;
#pragma unroll
        for (int k = 0; k < 48; k++) shv[k] = (alive && k < 3 * nb) ? sh[k] : 0.f;
    }
    if (!alive) return;
    float d0 = px3 - cam.campos[0], d1 = py3 - cam.campos[1], d2 = pz3 - cam.campos[2];
    const float len = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    d0 /= len; d1 /= len; d2 /= len;
    float B[16];
    B[0] = kC0;
    if (D > 0) {
        const float x = d0, y = d1, z = d2;
        B[1] = -kC1 * y; B[2] = kC1 * z; B[3] = -kC1 * x;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            B[4] = kC2[0] * xy; B[5] = kC2[1] * yz; B[6] = kC2[2] * (2.0f * zz - xx - yy);
            B[7] = kC2[3] * xz; B[8] = kC2[4] * (xx - yy);
            if (D > 2) {
                B[9] = kC3[0] * y * (3.0f * xx - yy);
                B[10] = kC3[1] * xy * z;
                B[11] = kC3[2] * y * (4.0f * zz - xx - yy);
                B[12] = kC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
                B[13] = kC3[4] * x * (4.0f * zz - xx - yy);
                B[14] = kC3[5] * z * (xx - yy);
                B[15] = kC3[6] * x * (xx - 3.0f * yy);
            }
        }
    }
    float col[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) col[ch] = B[0] * shv[ch];
#pragma unroll
    for (int k = 1; k < 16; k++) {
        if (k < nb) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) col[ch] = col[ch] + B[k] * shv[3 * k + ch];
        }
    }
    const int o = p.inst0 + i;
    uint8_t clampbits = 0;
    float4 out;
    float* oc = &out.x;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float v = col[ch] + 0.5f;
        if (v < 0) clampbits |= (uint8_t)(1u << ch);
        oc[ch] = fmaxf(v, 0.0f);
    }
    out.w = 0.f;
    reinterpret_cast<float4*>(p.rec)[(size_t)o * 4 + 2] = out;
    p.clamped[o] = clampbits;
}


// The SH waves of a hinted forward ride in the depth sort's launches (scan_sort.hip: onesweep_hist_sh_kernel, onesweep_pass_sh_kernel): the
// workgroups behind the sort's chunks evaluate a slice of the waves each.  The sort is latency-bound (five dependent launches that keep
// few CUs busy), the SH pass HBM-bound; side by side the colours cost little more than the sort alone.  p.note: carried by the hist launch.
struct ShRide {
    PreParams p;
    Cam cam;
    int split;          // shs_rest given: sh_color_wave<true>
    int waves;          // ceil(P / 64)
};

}  // namespace ibgs
