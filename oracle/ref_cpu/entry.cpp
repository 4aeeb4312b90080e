/*
 * entry.cpp -- plain-pointer C entry points into the reference rasterizer compiled for the CPU (TEST INFRASTRUCTURE ONLY; own code).
 *
 * Whole passes go through CudaRasterizer::Rasterizer::forward / backward / markVisible with malloc-backed allocators; the internal state is read
 * out of the reference's own chunk layout through its fromChunk functions.  The four stage functions (FORWARD::preprocess, FORWARD::render,
 * BACKWARD::render, BACKWARD::preprocess) are also callable on caller-given inputs, so a test can feed a stage the oracle's state.
 * Output and gradient arrays must come in zeroed, as the reference's torch front end allocates them.
 */
#include <functional>

#include "shim/refcpu.h"
#include <glm/glm.hpp>

#include "backward.h"
#include "forward.h"
#include "rasterizer.h"
#include "rasterizer_impl.h"
#include "auxiliary.h"

using namespace CudaRasterizer;

namespace {
struct Chunk {
    char* p = nullptr;
    std::function<char*(size_t)> alloc() { return [this](size_t n) { free(p); p = static_cast<char*>(calloc(n + 256, 1)); return p; }; }
    ~Chunk() { free(p); }
};
struct State { Chunk geom, binning, img; int P = 0, R = 0, W = 0, H = 0; };

struct Modes {
    bool q, r;
    Modes(int tex_quant, int reverse) : q(refcpu::tex_quant), r(refcpu::reverse_blocks) { refcpu::tex_quant = tex_quant != 0; refcpu::reverse_blocks = reverse != 0; }
    ~Modes() { refcpu::tex_quant = q; refcpu::reverse_blocks = r; }
};

/* layered colour (RGBA, alpha 1) and depth textures for the stage calls, through the same shim API the reference's host code uses */
struct Textures {
    cudaArray_t color = nullptr, depth = nullptr;
    cudaTextureObject_t tc = 0, td = 0;
    Textures(int W, int H, int n, const float* images, const float* depths)
    {
        if (n <= 0) return;
        cudaChannelFormatDesc c4 = cudaCreateChannelDesc<float4>(), c1 = cudaCreateChannelDesc<float>();
        cudaMalloc3DArray(&color, &c4, make_cudaExtent(W, H, n), cudaArrayLayered);
        cudaMalloc3DArray(&depth, &c1, make_cudaExtent(W, H, n), cudaArrayLayered);
        const size_t hw = (size_t)W * H;
        for (int l = 0; l < n; l++)
            for (size_t i = 0; i < hw; i++) {
                for (int c = 0; c < 3; c++) color->data[(l * hw + i) * 4 + c] = images[(l * 3 + c) * hw + i];
                color->data[(l * hw + i) * 4 + 3] = 1.0f;
                depth->data[l * hw + i] = depths[l * hw + i];
            }
        tc = (cudaTextureObject_t)(uintptr_t)color; td = (cudaTextureObject_t)(uintptr_t)depth;
    }
    ~Textures() { delete color; delete depth; }
};

template <typename T> void copy_out(void* dst, const T* src, size_t n) { if (dst && n) memcpy(dst, src, n * sizeof(T)); }
} // namespace

extern "C" {

void ref_mark_visible(int P, const float* means3D, const float* vm, const float* pm, uint8_t* present)
{
    static_assert(sizeof(bool) == 1, "bool is one byte");
    Rasterizer::markVisible(P, const_cast<float*>(means3D), const_cast<float*>(vm), const_cast<float*>(pm), reinterpret_cast<bool*>(present));
}

void* ref_forward(int P, int D, int M, const float* bg, int W, int H, const float* means3D, const float* shs, const float* colors_precomp,
                  const float* opacities, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                  const float* all_map, const float* vm, const float* pm, const float* ref_to_src, const float* src_cam_pos,
                  const float* src_images, const float* src_depths, int n_src, int buffer_length, float depth_thr, const float* campos,
                  float tanfovx, float tanfovy, float* out_color, int* radii, float* out_normal, float* out_depth, float* out_cam_feat,
                  float* out_warped, float* out_min_depth_diff, float* out_camera_ray, int* out_mask, int render_geo, int depth_only,
                  int tex_quant, int reverse_blocks, int* num_rendered)
{
    Modes modes(tex_quant, reverse_blocks);
    State* s = new State;
    s->P = P; s->W = W; s->H = H;
    s->R = Rasterizer::forward(s->geom.alloc(), s->binning.alloc(), s->img.alloc(), P, D, M, bg, W, H, means3D, shs, colors_precomp, opacities, scales,
                               scale_modifier, rotations, cov3D_precomp, all_map, vm, pm, ref_to_src, src_cam_pos, src_images, src_depths, n_src,
                               buffer_length, depth_thr, campos, tanfovx, tanfovy, false, out_color, radii, out_normal, out_depth, out_cam_feat,
                               out_warped, out_min_depth_diff, out_camera_ray, out_mask, render_geo != 0, depth_only != 0, false);
    *num_rendered = s->R;
    return s;
}

/* every internal array, carved from the chunks by the reference's own layout functions; null destinations are skipped */
void ref_state(void* handle, float* means2D, float* depths, float* cov3D, float* rgb, float* conic_opacity, uint32_t* tiles_touched,
               uint8_t* clamped, uint32_t* point_offsets, uint64_t* keys, uint32_t* point_list, uint64_t* keys_unsorted, uint32_t* point_list_unsorted,
               uint32_t* ranges, float* final_T, uint32_t* n_contrib, float* cache_sum_w, uint32_t* cache_low, uint32_t* cache_high,
               int* valid_src_idx, float* valid_src_w)
{
    State* s = static_cast<State*>(handle);
    const size_t P = s->P, R = s->R, HW = (size_t)s->W * s->H;
    char* g = s->geom.p; char* b = s->binning.p; char* i = s->img.p;
    GeometryState geom = GeometryState::fromChunk(g, P);
    BinningState bin = BinningState::fromChunk(b, R);
    ImageState img = ImageState::fromChunk(i, HW);
    copy_out(means2D, geom.means2D, P); copy_out(depths, geom.depths, P); copy_out(cov3D, geom.cov3D, 6 * P); copy_out(rgb, geom.rgb, 3 * P);
    copy_out(conic_opacity, geom.conic_opacity, P); copy_out(tiles_touched, geom.tiles_touched, P); copy_out(clamped, geom.clamped, 3 * P);
    copy_out(point_offsets, geom.point_offsets, P);
    copy_out(keys, bin.point_list_keys, R); copy_out(point_list, bin.point_list, R);
    copy_out(keys_unsorted, bin.point_list_keys_unsorted, R); copy_out(point_list_unsorted, bin.point_list_unsorted, R);
    const size_t tiles = (size_t)((s->W + BLOCK_X - 1) / BLOCK_X) * ((s->H + BLOCK_Y - 1) / BLOCK_Y);
    copy_out(ranges, img.ranges, tiles); copy_out(final_T, img.accum_alpha, HW); copy_out(n_contrib, img.n_contrib, HW);
    copy_out(cache_sum_w, img.buffer_cache_sum_median_weight, HW); copy_out(cache_low, img.buffer_cache_low_median_contributor, HW);
    copy_out(cache_high, img.buffer_cache_high_median_contributor, HW);
    copy_out(valid_src_idx, img.valid_src_indices, HW * M); copy_out(valid_src_w, img.valid_src_sum_median_weight, HW * M);
}

void ref_backward(void* handle, int D, int M, const float* bg, const float* normal_map, const float* depth_map, const float* warped, const float* means3D,
                  const float* shs, const float* colors_precomp, const float* all_map, const float* scales, float scale_modifier,
                  const float* rotations, const float* cov3D_precomp, const float* vm, const float* pm, const float* ref_to_src,
                  const float* src_cam_pos, const float* src_images, const float* src_depths, int n_src, const float* campos, float tanfovx,
                  float tanfovy, const int* radii, const float* g_color, const float* g_normal, const float* g_depth, const float* g_warped,
                  float* dL_dmean2D, float* dL_dmean2D_abs, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                  float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, float* dL_dall_map, int render_geo, int tex_quant,
                  int reverse_blocks)
{
    Modes modes(tex_quant, reverse_blocks);
    State* s = static_cast<State*>(handle);
    Rasterizer::backward(s->P, D, M, s->R, bg, normal_map, depth_map, warped, s->W, s->H, means3D, shs, colors_precomp, all_map, scales, scale_modifier,
                         rotations, cov3D_precomp, vm, pm, ref_to_src, src_cam_pos, src_images, src_depths, n_src, campos, tanfovx, tanfovy, radii,
                         s->geom.p, s->binning.p, s->img.p, g_color, g_normal, g_depth, g_warped, dL_dmean2D, dL_dmean2D_abs, dL_dconic, dL_dopacity,
                         dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, dL_dall_map, render_geo != 0, false);
}

void ref_free(void* handle) { delete static_cast<State*>(handle); }

/* ---- the four stage functions on caller-given inputs ---- */

void ref_stage_preprocess(int P, int D, int M, const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                          const float* opacities, const float* shs, const float* cov3D_precomp, const float* colors_precomp, const float* vm,
                          const float* pm, const float* campos, int W, int H, float tanfovx, float tanfovy, int depth_only, int* radii,
                          float* means2D, float* depths, float* cov3D, float* rgb, float* conic_opacity, uint32_t* tiles_touched, uint8_t* clamped)
{
    const float focal_y = H / (2.0f * tanfovy), focal_x = W / (2.0f * tanfovx);
    const dim3 grid((W + BLOCK_X - 1) / BLOCK_X, (H + BLOCK_Y - 1) / BLOCK_Y, 1);
    FORWARD::preprocess(P, D, M, means3D, (const glm::vec3*)scales, scale_modifier, (const glm::vec4*)rotations, opacities, shs,
                        reinterpret_cast<bool*>(clamped), cov3D_precomp, colors_precomp, vm, pm, (const glm::vec3*)campos, W, H, focal_x, focal_y,
                        tanfovx, tanfovy, radii, (float2*)means2D, depths, cov3D, rgb, (float4*)conic_opacity, grid, tiles_touched, false,
                        depth_only != 0);
}

void ref_stage_render_forward(int W, int H, const uint32_t* ranges, const uint32_t* point_list, const float* means2D, const float* features,
                              const float* all_map, const float* conic_opacity, const float* vm, const float* campos, const float* bg,
                              float tanfovx, float tanfovy, int n_src, const float* ref_to_src, const float* src_cam_pos, const float* src_images,
                              const float* src_depths, int L, float depth_thr, int render_geo, int depth_only, int tex_quant, float* final_T,
                              uint32_t* n_contrib, float* cache_sum_w, uint32_t* cache_low, uint32_t* cache_high, int* valid_src_idx,
                              float* valid_src_w, float* out_color, float* out_normal, float* out_depth, float* out_cam_feat, float* out_warped,
                              float* out_min_depth_diff, float* out_camera_ray, int* out_mask)
{
    Modes modes(tex_quant, 0);
    const float focal_y = H / (2.0f * tanfovy), focal_x = W / (2.0f * tanfovx);
    const dim3 grid((W + BLOCK_X - 1) / BLOCK_X, (H + BLOCK_Y - 1) / BLOCK_Y, 1), block(BLOCK_X, BLOCK_Y, 1);
    Textures tex(W, H, n_src, src_images, src_depths);
    FORWARD::render(grid, block, (const uint2*)ranges, point_list, W, H, focal_x, focal_y, float(W * 0.5f), float(H * 0.5f), vm, ref_to_src,
                    src_cam_pos, src_images, tex.tc, src_depths, tex.td, n_src, L, depth_thr, campos, (const float2*)means2D, features, all_map,
                    (const float4*)conic_opacity, final_T, n_contrib, cache_sum_w, cache_low, cache_high, valid_src_idx, valid_src_w, bg, out_color,
                    out_normal, out_depth, out_cam_feat, out_warped, out_min_depth_diff, out_camera_ray, out_mask, render_geo != 0, depth_only != 0);
}

void ref_stage_render_backward(int W, int H, const uint32_t* ranges, const uint32_t* point_list, const float* means2D, const float* conic_opacity,
                               const float* colors, const float* all_map, const float* bg, float tanfovx, float tanfovy, int n_src,
                               const float* ref_to_src, const float* src_cam_pos, const float* src_images, const float* src_depths,
                               const float* normal_map, const float* depth_map, const float* warped, const float* final_T, const uint32_t* n_contrib,
                               float* cache_sum_w, uint32_t* cache_low, uint32_t* cache_high, int* valid_src_idx, float* valid_src_w,
                               const float* g_color, const float* g_normal, const float* g_depth, const float* g_warped, int render_geo,
                               int tex_quant, int reverse_blocks, float* dL_dmean2D /* P x 3 */, float* dL_dmean2D_abs /* P x 3 */,
                               float* dL_dconic /* P x 4 */, float* dL_dopacity, float* dL_dcolors, float* dL_dall_map)
{
    Modes modes(tex_quant, reverse_blocks);
    const float focal_y = H / (2.0f * tanfovy), focal_x = W / (2.0f * tanfovx);
    const dim3 grid((W + BLOCK_X - 1) / BLOCK_X, (H + BLOCK_Y - 1) / BLOCK_Y, 1), block(BLOCK_X, BLOCK_Y, 1);
    Textures tex(W, H, n_src, src_images, src_depths);
    BACKWARD::render(grid, block, (const uint2*)ranges, point_list, W, H, focal_x, focal_y, bg, (const float2*)means2D, (const float4*)conic_opacity,
                     ref_to_src, src_cam_pos, src_images, tex.tc, src_depths, tex.td, n_src, colors, all_map, normal_map, depth_map, warped, final_T,
                     n_contrib, cache_sum_w, cache_low, cache_high, valid_src_idx, valid_src_w, g_color, g_normal, g_depth, g_warped,
                     (float3*)dL_dmean2D, (float3*)dL_dmean2D_abs, (float4*)dL_dconic, dL_dopacity, dL_dcolors, dL_dall_map, render_geo != 0);
}

void ref_stage_preprocess_backward(int P, int D, int M, const float* means3D, const int* radii, const float* shs, const uint8_t* clamped,
                                   const float* scales, const float* rotations, float scale_modifier, const float* cov3D, const float* vm,
                                   const float* pm, const float* campos, int W, int H, float tanfovx, float tanfovy, const float* dL_dmean2D,
                                   const float* dL_dconic, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                                   float* dL_drot)
{
    const float focal_y = H / (2.0f * tanfovy), focal_x = W / (2.0f * tanfovx);
    BACKWARD::preprocess(P, D, M, (const float3*)means3D, radii, shs, reinterpret_cast<const bool*>(clamped), (const glm::vec3*)scales,
                         (const glm::vec4*)rotations, scale_modifier, cov3D, vm, pm, focal_x, focal_y, tanfovx, tanfovy, (const glm::vec3*)campos,
                         (const float3*)dL_dmean2D, dL_dconic, (glm::vec3*)dL_dmean3D, dL_dcolor, dL_dcov3D, dL_dsh, (glm::vec3*)dL_dscale,
                         (glm::vec4*)dL_drot);
}

} // extern "C"
