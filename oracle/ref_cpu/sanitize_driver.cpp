/*
 * sanitize_driver.cpp -- stand-alone program (own code, own main) for sanitizer runs of the CPU build of the reference: entry.cpp's whole forward and backward on a
 * small random 3-source geo scene, in both texture modes and both block orders.  Built and run by `python oracle/ref_cpu/build.py --sanitize [undefined|address]`
 * into oracle/_ref/; never loaded into Python.  TEST INFRASTRUCTURE ONLY.
 */
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include <cmath>
extern "C" {
void* ref_forward(int P, int D, int M, const float* bg, int W, int H, const float* means3D, const float* shs, const float* colors_precomp,
                  const float* opacities, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                  const float* all_map, const float* vm, const float* pm, const float* ref_to_src, const float* src_cam_pos,
                  const float* src_images, const float* src_depths, int n_src, int buffer_length, float depth_thr, const float* campos,
                  float tanfovx, float tanfovy, float* out_color, int* radii, float* out_normal, float* out_depth, float* out_cam_feat,
                  float* out_warped, float* out_min_depth_diff, float* out_camera_ray, int* out_mask, int render_geo, int depth_only,
                  int tex_quant, int reverse_blocks, int* num_rendered);
void ref_backward(void* handle, int D, int M, const float* bg, const float* normal_map, const float* depth_map, const float* warped, const float* means3D,
                  const float* shs, const float* colors_precomp, const float* all_map, const float* scales, float scale_modifier,
                  const float* rotations, const float* cov3D_precomp, const float* vm, const float* pm, const float* ref_to_src,
                  const float* src_cam_pos, const float* src_images, const float* src_depths, int n_src, const float* campos, float tanfovx,
                  float tanfovy, const int* radii, const float* g_color, const float* g_normal, const float* g_depth, const float* g_warped,
                  float* dL_dmean2D, float* dL_dmean2D_abs, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                  float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, float* dL_dall_map, int render_geo, int tex_quant, int reverse_blocks);
void ref_free(void*);
}
static float rnd() { return (float)rand() / RAND_MAX; }
int main() {
    const int P = 700, W = 72, H = 56, M = 16, D = 3, n = 3, HW = W * H;
    std::vector<float> m(3 * P), sh(3 * M * P), op(P), sc(3 * P), rot(4 * P), am(5 * P), img(n * 3 * HW), dep(n * HW, 4.0f), r2s(n * 16, 0.f), scp(n * 3, 0.1f);
    for (int i = 0; i < P; i++) { m[3*i] = 2*rnd()-1; m[3*i+1] = 1.5f*rnd()-0.75f; m[3*i+2] = 3 + 2*rnd(); op[i] = 0.2f + 0.7f*rnd();
        for (int k = 0; k < 3; k++) sc[3*i+k] = 0.05f + 0.2f*rnd(); rot[4*i] = 1; rot[4*i+1] = rot[4*i+2] = rot[4*i+3] = 0;
        am[5*i] = 0; am[5*i+1] = 0; am[5*i+2] = -1; am[5*i+3] = 0; am[5*i+4] = m[3*i+2]; }
    for (auto& v : sh) v = rnd() - 0.5f;
    for (auto& v : img) v = rnd();
    for (int s = 0; s < n; s++) { float* r = &r2s[16*s]; r[0] = r[5] = r[10] = r[15] = 1; r[3] = 0.05f * (s + 1); }
    const float tanx = 0.36f, tany = 0.28f, zn = 0.01f, zf = 100.f;
    float vm[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1}, pm[16] = {0};
    pm[0] = 1/tanx; pm[5] = 1/tany; pm[10] = zf/(zf-zn); pm[11] = 1; pm[14] = -(zf*zn)/(zf-zn);
    float campos[3] = {0,0,0}, bg[3] = {1, 0.5f, 0.2f};
    std::vector<float> gc(3*HW), gn(3*HW), gd(HW), gw(15*HW);
    for (auto* v : {&gc, &gn, &gd, &gw}) for (auto& x : *v) x = rnd() - 0.5f;
    for (int pass = 0; pass < 4; pass++) {
        std::vector<float> color(3*HW, 0), normal(3*HW, 0), depth(HW, 0), feat(20*HW, 0), warp(15*HW, 0), mdd(HW, 0), ray(3*HW, 0);
        std::vector<int> radii(P, 0), mask(HW, 0); int R = 0;
        void* h = ref_forward(P, D, M, bg, W, H, m.data(), sh.data(), nullptr, op.data(), sc.data(), 1.0f, rot.data(), nullptr, am.data(), vm, pm, r2s.data(), scp.data(),
                              img.data(), dep.data(), n, 4, 0.5f, campos, tanx, tany, color.data(), radii.data(), normal.data(), depth.data(), feat.data(), warp.data(), mdd.data(),
                              ray.data(), mask.data(), 1, 0, pass & 1, pass >> 1, &R);
        std::vector<float> d2(3*P,0), d2a(3*P,0), dc(4*P,0), dop(P,0), dcol(3*P,0), d3(3*P,0), dcov(6*P,0), dsh(3*M*P,0), dsc(3*P,0), drot(4*P,0), dam(5*P,0);
        ref_backward(h, D, M, bg, normal.data(), depth.data(), warp.data(), m.data(), sh.data(), nullptr, am.data(), sc.data(), 1.0f, rot.data(), nullptr, vm, pm, r2s.data(), scp.data(),
                     img.data(), dep.data(), n, campos, tanx, tany, radii.data(), gc.data(), gn.data(), gd.data(), gw.data(), d2.data(), d2a.data(), dc.data(), dop.data(), dcol.data(),
                     d3.data(), dcov.data(), dsh.data(), dsc.data(), drot.data(), dam.data(), 1, pass & 1, pass >> 1);
        ref_free(h);
        double s = 0; int valid = 0; for (float v : d3) s += std::fabs(v); for (float v : warp) valid += v != 0;
        printf("pass %d: R = %d, sum|dL_dmeans3D| = %.6g, warped nonzero = %d\n", pass, R, s, valid);
    }
    return 0;
}
