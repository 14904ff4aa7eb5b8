// GaussiansBuffer::edit / extract and sh_rotation_matrices (include/gs3d.hpp) through the C ABI: a grid of Gaussians is
// split with a box, the left half is moved, recoloured and faded on the device, and the records that come back are
// compared with values computed here (translation, power-of-two scale and an axis-aligned colour matrix are exact in f32).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint8_t quant(float v) {      // t = v 255 + 0.5; 0, 255 or floor(t)
    const float t = v * 255.0f + 0.5f;
    return !(t > 0.0f) ? 0 : t >= 255.0f ? 255 : (uint8_t)std::floor(t);
}

int main() {
    Device dev(0);
    Stream s(dev);
    using G = GaussianPodWithShSingleCov3dRotScaleConfigs;
    const uint32_t side = 40, n = side * side;
    std::vector<Gaussian> all;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % side) - 19.5f) * 0.125f;
        g.pos[1] = ((float)(i / side) - 19.5f) * 0.0625f;
        g.pos[2] = -5.0f - (float)(i % 7) * 0.25f;
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = 180;
        g.scale[0] = 0.03f; g.scale[1] = 0.02f; g.scale[2] = 0.01f;
        for (int k = 0; k < 45; k++) g.sh[k] = (float)((int)((i + k) % 9) - 4) * 0.0625f;
        all.push_back(g);
    }
    GaussiansBuffer<G> buf(dev, all);
    gs_model_transform_pod mt;
    gs_model_transform_pod_default(&mt);
    Selection sel(dev, n);
    const float box[12] = {0.25f, 0, 0, 0, 0.25f, 0, 0, 0, 1.0f / 16.0f, 1.0f, 0, 0};   // -8 <= x <= 0
    sel.select_box(s, buf, mt, box);
    const uint64_t left = sel.count(s);
    REQUIRE(left == n / 2);

    // the identity rotation has identity band matrices
    const float ident[4] = {0, 0, 0, 1};
    ShRotation sr = sh_rotation_matrices(ident);
    for (int k = 0; k < 49; k++) REQUIRE(sr.d3[k] == (k % 8 == 0 ? 1.0f : 0.0f));
    for (int k = 0; k < 9; k++) REQUIRE(sr.d1[k] == (k % 4 == 0 ? 1.0f : 0.0f));

    // one edit: move by (1, -2, 0.5) and double the size; swap red and green, blue := 0.25; halve the opacity
    gs_edit e{};
    e.flags = GS_EDIT_TRANSFORM | GS_EDIT_ROTATE_SH | GS_EDIT_COLOR | GS_EDIT_OPACITY;
    gs_model_transform_pod_default(&e.transform);
    e.transform.pos[0] = 1.0f; e.transform.pos[1] = -2.0f; e.transform.pos[2] = 0.5f;
    e.transform.scale[0] = e.transform.scale[1] = e.transform.scale[2] = 2.0f;
    e.color[1] = 1.0f;      // column 0 (r) -> g
    e.color[3] = 1.0f;      // column 1 (g) -> r
    e.color[11] = 0.25f;    // offset of b
    e.opacity[0] = 0.5f;
    buf.edit(s, &sel, e);
    std::vector<Gaussian> got = buf.download_gaussians(s);
    REQUIRE(got.size() == n);
    for (uint32_t i = 0; i < n; i++) {
        const Gaussian &a = all[i], &b = got[i];
        if (a.pos[0] > 0.0f) {
            REQUIRE(std::memcmp(&a, &b, sizeof(Gaussian)) == 0);
            continue;
        }
        for (int k = 0; k < 3; k++) {
            REQUIRE(b.pos[k] == 2.0f * a.pos[k] + e.transform.pos[k]);
            REQUIRE(b.scale[k] == 2.0f * a.scale[k]);
        }
        for (int k = 0; k < 4; k++) REQUIRE(b.rot[k] == a.rot[k]);
        REQUIRE(b.color[0] == quant((float)a.color[1] / 255.0f) && b.color[1] == quant((float)a.color[0] / 255.0f));
        REQUIRE(b.color[0] == a.color[1] && b.color[1] == a.color[0] && b.color[2] == quant(0.25f));
        REQUIRE(b.color[3] == quant(0.5f * ((float)a.color[3] / 255.0f)));
        for (int k = 0; k < 15; k++) {      // identity rotation; the linear colour part swaps r and g and zeroes b
            REQUIRE(b.sh[3 * k] == a.sh[3 * k + 1] && b.sh[3 * k + 1] == a.sh[3 * k] && b.sh[3 * k + 2] == 0.0f);
        }
    }
    // argument errors
    gs_edit bad = e;
    bad.transform.scale[1] = 3.0f;
    try { buf.edit(s, &sel, bad); REQUIRE(false); } catch (const Error &) {}
    bad = e;
    bad.flags = 16;
    try { buf.edit(s, nullptr, bad); REQUIRE(false); } catch (const Error &) {}

    // extraction: the left half and its complement, in caller order
    GaussiansBuffer<G> lhs = buf.extract(s, &sel), rhs = buf.extract(s, &sel, true), everything = buf.extract(s, nullptr);
    REQUIRE(lhs.len() == left && rhs.len() == n - left && everything.len() == n);
    std::vector<Gaussian> gl = lhs.download_gaussians(s), gr = rhs.download_gaussians(s);
    size_t il = 0, ir = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (all[i].pos[0] <= 0.0f) { REQUIRE(std::memcmp(&gl[il++], &got[i], sizeof(Gaussian)) == 0); }
        else { REQUIRE(std::memcmp(&gr[ir++], &got[i], sizeof(Gaussian)) == 0); }
    }
    REQUIRE(il == gl.size() && ir == gr.size());
    sel.clear(s);
    GaussiansBuffer<G> none = buf.extract(s, &sel);
    REQUIRE(none.len() == 0 && none.is_empty());
    std::printf("cpp edit OK\n");
    return 0;
}
