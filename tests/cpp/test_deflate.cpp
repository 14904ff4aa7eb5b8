// gs3d::gzip_fast, Buffer::gzip_fast and GaussiansBuffer::export_spz_fast (include/gs3d.hpp) through the C ABI:
// the device member of a buffer's bytes equals the host member of the same bytes and inflates to them; a grid of Gaussians is
// saved with and without a selection and read back through SpzGaussians::read_from; the argument errors come as exceptions.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static std::vector<uint8_t> inflate_member(const std::vector<uint8_t> &z) {
    size_t n = 0;
    check(gs_spz_decompress(z.data(), z.size(), nullptr, 0, &n));
    std::vector<uint8_t> out(n ? n : 1);
    check(gs_spz_decompress(z.data(), z.size(), out.data(), n, &n));
    out.resize(n);
    return out;
}

int main() {
    Device dev(0);
    Stream s(dev);
    // three chunks and a bit: a skewed part, a constant chunk, noise
    std::vector<uint8_t> bytes(3 * 32768 + 777);
    uint32_t x = 12345u;
    for (size_t i = 0; i < bytes.size(); i++) {
        x = x * 1664525u + 1013904223u;
        const uint32_t r = x >> 24;
        bytes[i] = i < 32768 ? (uint8_t)(r & (r >> 4) & 15u) : i < 65536 ? (uint8_t)9 : (uint8_t)r;
    }
    Buffer buf(dev, bytes.size(), bytes.data());
    const std::vector<uint8_t> host = gzip_fast(bytes.data(), bytes.size());
    REQUIRE(host.size() <= gs_gzip_fast_bound(bytes.size()) && host.size() < bytes.size());
    REQUIRE(host[0] == 0x1f && host[1] == 0x8b && host[9] == 0x03);
    REQUIRE(buf.gzip_fast(s, 0, bytes.size()) == host);
    REQUIRE(inflate_member(host) == bytes);
    // an unaligned range
    const std::vector<uint8_t> part(bytes.begin() + 13, bytes.begin() + 13 + 40001);
    const std::vector<uint8_t> dev_part = buf.gzip_fast(s, 13, 40001);
    REQUIRE(dev_part == gzip_fast(part.data(), part.size()) && inflate_member(dev_part) == part);
    REQUIRE(buf.gzip_fast(s, 5, 0).size() == 20);
    try { buf.gzip_fast(s, bytes.size() - 3, 4); REQUIRE(false); } catch (const Error &e) { REQUIRE(e.status == GS_ERR_INVALID_ARGUMENT); }

    // a scene saved on the device
    using Full = GaussianPodWithShSingleCov3dRotScaleConfigs;
    const uint32_t n = 1025;
    std::vector<Gaussian> all;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[0] = 0.1f * (float)(i % 5); g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % 50) - 24.5f) * 0.125f;
        g.pos[1] = ((float)(i / 50) - 24.5f) * 0.0625f;
        g.pos[2] = -5.0f - (float)(i % 7) * 0.25f;
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = (uint8_t)(i * 7u);
        for (int k = 0; k < 45; k++) g.sh[k] = 0.001f * (float)((i * 13u + (uint32_t)k * 7u) % 2001u) - 1.0f;
        g.scale[0] = 0.03f; g.scale[1] = 0.02f; g.scale[2] = 0.01f + 0.001f * (float)(i % 3);
        all.push_back(g);
    }
    GaussiansBuffer<Full> full(dev, all);
    auto payload_of = [&](const Selection *sel, bool invert) {
        size_t bytes_out = 0;
        check(gs_gaussians_buffer_export_spz_decompressed(full.raw(), s.raw(), sel ? sel->raw() : nullptr, invert ? 1 : 0, nullptr, nullptr, 0, &bytes_out));
        std::vector<uint8_t> p(bytes_out);
        check(gs_gaussians_buffer_export_spz_decompressed(full.raw(), s.raw(), sel ? sel->raw() : nullptr, invert ? 1 : 0, nullptr, p.data(), p.size(), &bytes_out));
        return p;
    };
    const std::vector<uint8_t> file = full.export_spz_fast(s);
    REQUIRE(inflate_member(file) == payload_of(nullptr, false));
    REQUIRE(file == gzip_fast(payload_of(nullptr, false).data(), payload_of(nullptr, false).size()));
    REQUIRE(SpzGaussians::read_from(file.data(), file.size()).gaussians.size() == n);
    Selection sel(dev, n);
    std::vector<uint32_t> words(sel.words(), 0u);
    uint32_t picked = 0;
    for (uint32_t i = 0; i < n; i += 3) { words[i >> 5] |= 1u << (i & 31u); picked++; }
    sel.upload(s, words);
    const std::vector<uint8_t> third = full.export_spz_fast(s, &sel), rest = full.export_spz_fast(s, &sel, true);
    REQUIRE(inflate_member(third) == payload_of(&sel, false) && inflate_member(rest) == payload_of(&sel, true));
    REQUIRE(SpzGaussians::read_from(third.data(), third.size()).gaussians.size() == picked);
    REQUIRE(SpzGaussians::read_from(rest.data(), rest.size()).gaussians.size() == n - picked);
    // a layout that cannot be exported is refused as by the zlib export
    GaussiansBuffer<GaussianPodWithShHalfCov3dHalfConfigs> small(dev, all);
    try { small.export_spz_fast(s); REQUIRE(false); } catch (const Error &e) { REQUIRE(e.status == GS_ERR_LOSSY_CONFIG); }
    std::printf("cpp deflate OK\n");
    return 0;
}
