// Renderer::render_contrib, contributions_clear and Selection::select_contribution (include/gs3d.hpp) through the C ABI: one
// small frame of a grid of 3 001 Gaussians rendered twice into the same records — a frame never clears them, so the second
// frame doubles every `sum` and `hits` and keeps every `wmax` — and the selection of the Gaussians no pixel blended.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    static_assert(sizeof(gs_contribution) == 16, "record size");
    Device dev(0);
    Stream s(dev);
    using G = GaussianPodWithShSingleCov3dRotScaleConfigs;
    const uint32_t n = 3001;        // two full 1024-blocks and a partial one; not a multiple of 32
    std::vector<Gaussian> all;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % 60) - 29.5f) * 0.125f;
        g.pos[1] = ((float)((i / 60) % 50) - 24.5f) * 0.125f;
        g.pos[2] = -6.0f - (float)(i % 5) * 0.5f + (i >= 3000 ? 20.0f : 0.0f);      // the last one lies behind the camera
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = (uint8_t)(128u + i % 128u);
        g.scale[0] = 0.05f; g.scale[1] = 0.04f; g.scale[2] = 0.03f;
        all.push_back(g);
    }
    GaussiansBuffer<G> buf(dev, all);
    gs_camera cam;
    const float eye[3] = {0, 0, 0}, target[3] = {0, 0, -1}, up[3] = {0, 1, 0};
    gs_camera_look_at(eye, target, up, 1.0f, 333, 197, 0.1f, 100.0f, &cam);
    gs_gaussian_transform_pod gt; gs_gaussian_transform_pod_default(&gt);
    gs_model_transform_pod mt; gs_model_transform_pod_default(&mt);
    Buffer img(dev, (size_t)333 * 197 * 16);
    std::vector<uint8_t> poison((size_t)n * 16, 0xA5);
    Buffer contrib(dev, poison.size(), poison.data());
    contributions_clear(contrib, s, n);
    Renderer r(dev);
    r.render_contrib(s, buf, gt, mt, cam, (float *)img.device_ptr(), contrib);
    const gs_frame_result fr = r.wait_frame();
    REQUIRE(fr.flags == 0 && fr.visible > 0 && fr.visible < n);
    const std::vector<gs_contribution> one = contrib.download<gs_contribution>(s);
    REQUIRE(one.size() == n);
    r.render_contrib(s, buf, gt, mt, cam, (float *)img.device_ptr(), contrib);
    REQUIRE(r.wait_frame().flags == 0);
    const std::vector<gs_contribution> two = contrib.download<gs_contribution>(s);
    uint64_t blended = 0;
    for (uint32_t i = 0; i < n; i++) {
        REQUIRE(two[i].sum == 2 * one[i].sum && two[i].hits == 2 * one[i].hits);
        REQUIRE(std::memcmp(&two[i].wmax, &one[i].wmax, 4) == 0);
        REQUIRE((one[i].hits == 0) == (one[i].sum == 0) && (one[i].hits == 0) == (one[i].wmax == 0.0f));
        REQUIRE(one[i].wmax <= 0.99f);
        blended += one[i].hits != 0 ? 1 : 0;
    }
    REQUIRE(blended > 0 && blended <= fr.visible && one[n - 1].hits == 0);
    Selection unseen(dev, n);
    unseen.select_contribution(s, contrib, GS_CONTRIB_HITS, 0.0f, 0.0f);
    REQUIRE(unseen.count(s) == n - blended);
    try { unseen.select_contribution(s, contrib, 3, 0.0f, 0.0f); REQUIRE(false); } catch (const Error &) {}
    std::printf("cpp contrib OK\n");
    return 0;
}
