// gs3d::Selection and the selection overload of Renderer::render (include/gs3d.hpp) through the C ABI: a grid of
// Gaussians in front of the camera, cropped with a box; the frame without the hidden half must equal the frame of a
// buffer that only holds the kept half.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    Device dev(0);
    Stream s(dev);
    using G = GaussianPodWithShNoneCov3dRotScaleConfigs;
    const uint32_t side = 40, n = side * side;
    std::vector<Gaussian> all, kept;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % side) - 19.5f) * 0.125f;      // x in [-2.4375, 2.4375], exact in f32
        g.pos[1] = ((float)(i / side) - 19.5f) * 0.0625f;
        g.pos[2] = -5.0f - (float)(i % 7) * 0.25f;
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = 180;
        g.scale[0] = g.scale[1] = g.scale[2] = 0.03f;
        all.push_back(g);
        if (g.pos[0] >= 0.0f) kept.push_back(g);
    }
    GaussiansBuffer<G> buf(dev, all), kept_buf(dev, kept);
    buf.set_spatial_order(false);           // exact-depth ties blend in mirror order: keep both buffers in index order
    kept_buf.set_spatial_order(false);
    gs_model_transform_pod mt;
    gs_model_transform_pod_default(&mt);
    gs_gaussian_transform_pod gt = *gaussian_transform_pod(1.0f, GS_DISPLAY_SPLAT, 0, false, 3.0f);

    // bit operations and the select ops
    Selection sel(dev, n), other(dev, n);
    REQUIRE(sel.len() == n && sel.words() == (n + 31) / 32 && sel.count(s) == 0);
    sel.fill(s);
    REQUIRE(sel.count(s) == n);
    const float box[12] = {0.25f, 0, 0, 0, 0.25f, 0, 0, 0, 1.0f / 16.0f, 1.0f, 0, 0};   // -8 <= x <= 0, |y| <= 4, |z| <= 16
    sel.select_box(s, buf, mt, box);
    uint64_t left = 0;
    for (const Gaussian &g : all) left += g.pos[0] <= 0.0f ? 1 : 0;
    REQUIRE(sel.count(s) == left && left == n - kept.size());
    auto words = sel.download(s);
    for (uint32_t i = 0; i < n; i++) REQUIRE(((words[i >> 5] >> (i & 31)) & 1u) == (all[i].pos[0] <= 0.0f ? 1u : 0u));
    const float center[3] = {all[77].pos[0], all[77].pos[1], all[77].pos[2]};
    other.select_sphere(s, buf, mt, center, 0.0f);
    REQUIRE(other.count(s) == 1);
    other.combine(s, GS_SEL_OR, sel);
    REQUIRE(other.count(s) == left + (all[77].pos[0] <= 0.0f ? 0 : 1));
    other.invert(s);
    other.combine(s, GS_SEL_AND, sel);
    REQUIRE(other.count(s) == 0);
    try { Selection wrong(dev, n + 1); wrong.combine(s, GS_SEL_OR, sel); REQUIRE(false); } catch (const Error &) {}

    // frames
    const uint32_t W = 320, H = 192;
    gs_camera cam;
    const float eye[3] = {0, 0, 0}, target[3] = {0, 0, -1}, up[3] = {0, 1, 0};
    gs_camera_look_at(eye, target, up, 1.0f, W, H, 0.1f, 100.0f, &cam);
    Buffer img_a(dev, (size_t)W * H * 16), img_b(dev, (size_t)W * H * 16);
    Renderer ra(dev), rb(dev);
    ra.render(s, buf, gt, mt, cam, (float *)img_a.device_ptr(), 0, 0xffffffffu, nullptr, &sel);
    gs_frame_result fa = ra.wait_frame();
    rb.render(s, kept_buf, gt, mt, cam, (float *)img_b.device_ptr());
    gs_frame_result fb = rb.wait_frame();
    REQUIRE(fa.visible == fb.visible && fa.pairs == fb.pairs && fa.visible > 0 && fa.gaussians == n);
    auto a = img_a.download<float>(s), b = img_b.download<float>(s);
    REQUIRE(a.size() == (size_t)W * H * 4 && std::memcmp(a.data(), b.data(), a.size() * 4) == 0);
    // what the frame kept is what lies right of the crop
    Selection vis(dev, n);
    ra.select_visible(s, vis, -1e9f, -1e9f, 1e9f, 1e9f);
    REQUIRE(vis.count(s) == fa.visible);
    vis.combine(s, GS_SEL_AND, sel);
    REQUIRE(vis.count(s) == 0);
    // no selection: the plain frame
    ra.render(s, buf, gt, mt, cam, (float *)img_a.device_ptr(), 0, 0xffffffffu, nullptr, nullptr);
    gs_frame_result fp = ra.wait_frame();
    rb.render(s, buf, gt, mt, cam, (float *)img_b.device_ptr());
    gs_frame_result fq = rb.wait_frame();
    REQUIRE(fp.visible == fq.visible && fp.pairs == fq.pairs && fp.visible > fa.visible);
    a = img_a.download<float>(s); b = img_b.download<float>(s);
    REQUIRE(std::memcmp(a.data(), b.data(), a.size() * 4) == 0);
    // tint with alpha 1: every tinted pixel contribution is the tint colour, so a frame of all-tinted splats over a
    // black background has r : g : b = t
    sel.fill(s);
    const float t[4] = {0.5f, 0.25f, 0.125f, 1.0f};
    ra.render(s, buf, gt, mt, cam, (float *)img_a.device_ptr(), 0, 0xffffffffu, nullptr, nullptr, &sel, t);
    ra.wait_frame();
    a = img_a.download<float>(s);
    size_t lit = 0;
    for (size_t p = 0; p < (size_t)W * H; p++) {
        if (a[4 * p] == 0.0f) continue;
        lit++;
        REQUIRE(a[4 * p + 1] == 0.5f * a[4 * p] && a[4 * p + 2] == 0.25f * a[4 * p]);
    }
    REQUIRE(lit > 0);
    std::printf("cpp selection OK\n");
    return 0;
}
