// GaussiansBuffer::simplify<To> (include/gs3d.hpp) through the C ABI: six clumps of ten equal isotropic Gaussians, an anchor
// at the origin (which shares the first clump's cell), one isolated Gaussian and a NaN row, simplified with a cell of side 1
// into (SH f32, cov f32).  K, the cell plane and the merged first-but-one clump are checked against values computed here in
// double; the isolated Gaussian, simplified into its own layout, keeps its bytes.
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
    using G = GaussianPodWithShSingleCov3dRotScaleConfigs;
    using Wide = GaussianPodWithShSingleCov3dSingleConfigs;
    std::vector<Gaussian> all;
    uint32_t seed = 4321u;
    auto jitter = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 20) * (1.0f / 4096.0f) - 0.5f; };      // [-0.5, 0.5)
    auto add = [&all](float x, float y, float z) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = x; g.pos[1] = y; g.pos[2] = z;
        g.scale[0] = g.scale[1] = g.scale[2] = 0.01f;
        g.color[0] = 10; g.color[1] = 200; g.color[2] = 90; g.color[3] = 255;
        for (int k = 0; k < 45; k++) g.sh[k] = 0.01f * (float)k - 0.2f;
        all.push_back(g);
    };
    add(0.0f, 0.0f, 0.0f);                                           // the anchor: lo = 0 on every axis
    // clump k around x = 10 k + 0.5, y = z = 0.5, +-0.1: with h = 1 + 2^-10 its cell is (10 k, 0, 0), far from a cell border
    for (uint32_t k = 0; k < 6; k++)
        for (uint32_t j = 0; j < 10; j++) add(10.0f * (float)k + 0.5f + 0.2f * jitter(), 0.5f + 0.2f * jitter(), 0.5f + 0.2f * jitter());
    add(100.5f, 0.5f, 0.5f);                                         // alone in its cell
    add(NAN, 0.5f, 0.5f);                                            // no point
    const uint32_t n = (uint32_t)all.size(), alone = n - 2u;
    // interleave: the clumps must not be contiguous in caller order
    std::vector<Gaussian> mixed(n);
    std::vector<uint32_t> where(n);
    for (uint32_t i = 0; i < n; i++) where[i] = (i * 37u) % n;      // 37 and n = 63 are coprime
    REQUIRE(n == 63);
    for (uint32_t i = 0; i < n; i++) mixed[where[i]] = all[i];
    GaussiansBuffer<G> buf(dev, mixed);

    Buffer plane(dev, (size_t)n * 4);
    GaussiansBuffer<Wide> out = buf.simplify<Wide>(s, 1.0f, nullptr, &plane);
    REQUIRE(out.len() == 7);                                         // six clumps (the anchor is in the first) and the isolated one
    const std::vector<uint32_t> cell_of = plane.download<uint32_t>(s);
    REQUIRE(cell_of[where[0]] == 0u && cell_of[where[alone]] == 6u && cell_of[where[n - 1u]] == 0xffffffffu);
    for (uint32_t k = 0; k < 6; k++)
        for (uint32_t j = 0; j < 10; j++) REQUIRE(cell_of[where[1u + 10u * k + j]] == k);

    // clump 1: equal weights, so the position is the mean and the covariance 1e-4 I plus the scatter of the positions
    double mean[3] = {0, 0, 0}, second[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t j = 0; j < 10; j++)
        for (int a = 0; a < 3; a++) mean[a] += (double)all[11u + j].pos[a] / 10.0;
    const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {0, 1, 2, 1, 2, 2};
    for (uint32_t j = 0; j < 10; j++)
        for (int k = 0; k < 6; k++)
            second[k] += ((double)all[11u + j].pos[pa[k]] - mean[pa[k]]) * ((double)all[11u + j].pos[pb[k]] - mean[pb[k]]) / 10.0;
    const std::vector<uint8_t> bytes = out.download(s);
    REQUIRE(bytes.size() == 7 * Wide::size() && Wide::size() == 224);
    float rec[56];
    std::memcpy(rec, bytes.data() + 1 * Wide::size(), sizeof rec);
    const double s2 = (double)0.01f * (double)0.01f;
    for (int a = 0; a < 3; a++) REQUIRE(std::fabs((double)rec[a] - mean[a]) <= 1e-5);
    for (int k = 0; k < 6; k++) REQUIRE(std::fabs((double)rec[49 + k] - (second[k] + (pa[k] == pb[k] ? s2 : 0.0))) <= 1e-6);
    for (int k = 0; k < 45; k++) REQUIRE(std::fabs((double)rec[4 + k] - (double)(0.01f * (float)k - 0.2f)) <= 1e-6);
    const uint8_t *color = bytes.data() + 1 * Wide::size() + 12;
    REQUIRE(std::abs((int)color[0] - 10) <= 1 && std::abs((int)color[1] - 200) <= 1 && std::abs((int)color[2] - 90) <= 1);
    // opacity x size mass: W = 10 x 3e-4 over the larger merged trace
    const double trace = 3.0 * s2 + second[0] + second[3] + second[5];
    REQUIRE(30.0 * s2 / trace < 0.9);
    REQUIRE(std::abs((int)color[3] - (int)std::floor(255.0 * (30.0 * s2 / trace) + 0.5)) <= 1);

    // into its own layout: the isolated Gaussian keeps its bytes, and two calls agree
    GaussiansBuffer<G> same = buf.simplify(s, 1.0f);
    const std::vector<uint8_t> a = same.download(s), src = buf.download(s);
    REQUIRE(same.len() == 7 && std::memcmp(a.data() + 6 * G::size(), src.data() + where[alone] * G::size(), G::size()) == 0);
    REQUIRE(buf.simplify(s, 1.0f).download(s) == a);
    REQUIRE(buf.download(s) == src);
    try { buf.simplify(s, -1.0f); REQUIRE(false); } catch (const Error &) {}
    std::printf("cpp simplify OK\n");
    return 0;
}
