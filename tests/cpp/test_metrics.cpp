// gs3d::image_compare (include/gs3d.hpp) through the C ABI: a 37 x 21 image against itself (identical, every SSIM value 1)
// and against a copy with one changed pixel (one differing pixel, the maxima at its index), and the argument errors as
// exceptions.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    static_assert(sizeof(gs_image_metrics) == 176 && sizeof(gs_image_compare_desc) == 40, "record sizes");
    Device dev(0);
    Stream s(dev);
    const uint32_t W = 37, H = 21, at = 9 * W + 30;      // more than one tile in both axes, ragged edges
    std::vector<float> a((size_t)W * H * 4);
    for (size_t i = 0; i < a.size(); i++) a[i] = (float)((i * 2654435761u) >> 8 & 0xffff) / 65535.0f;
    std::vector<float> b = a;
    b[(size_t)at * 4 + 1] += 0.25f;      // green
    b[(size_t)at * 4 + 3] -= 0.5f;       // alpha
    Buffer da(dev, a.size() * 4, a.data()), db(dev, b.size() * 4, b.data()), plane(dev, (size_t)W * H * 4);
    const float *pa = (const float *)da.device_ptr(), *pb = (const float *)db.device_ptr();

    gs_image_compare_desc d{};
    d.flags = GS_COMPARE_SSIM;
    d.data_range = 1.0f;
    d.err_plane = (float *)plane.device_ptr();
    const gs_image_metrics same = image_compare(dev, s, pa, pa, W, H, &d);
    REQUIRE(same.pixels == (uint64_t)W * H && same.finite == same.pixels && same.differing == 0 && same.bit_differing == 0);
    for (int c = 0; c < 4; c++) REQUIRE(same.sum_sq[c] == 0.0 && same.sum_abs[c] == 0.0 && same.max_abs[c] == 0.0f && same.max_abs_at[c] == 0);
    for (int c = 0; c < 3; c++) REQUIRE(same.ssim_sum[c] == (double)(W * H) && same.ssim_finite[c] == (uint64_t)W * H);
    REQUIRE(image_ssim(same) == 1.0 && std::isinf(image_psnr(same)));

    const gs_image_metrics one = image_compare(dev, s, pa, pb, W, H, &d);
    REQUIRE(one.finite == one.pixels && one.differing == 1 && one.bit_differing == 1);
    const float dg = a[(size_t)at * 4 + 1] - b[(size_t)at * 4 + 1], dal = a[(size_t)at * 4 + 3] - b[(size_t)at * 4 + 3];
    REQUIRE(one.max_abs[0] == 0.0f && one.max_abs_at[0] == 0 && one.max_abs[2] == 0.0f && one.max_abs_at[2] == 0);
    REQUIRE(one.max_abs[1] == std::fabs(dg) && one.max_abs_at[1] == at && one.max_abs[3] == std::fabs(dal) && one.max_abs_at[3] == at);
    REQUIRE(one.sum_sq[1] == (double)dg * (double)dg && one.sum_abs[3] == (double)std::fabs(dal) && one.sum_sq[0] == 0.0);
    REQUIRE(one.ssim_sum[0] == (double)(W * H) && one.ssim_sum[1] < (double)(W * H) && one.ssim_sum[2] == (double)(W * H));
    REQUIRE(image_ssim(one) < 1.0 && image_psnr(one) > 0.0 && !std::isinf(image_psnr(one)));
    const std::vector<float> err = plane.download<float>(s);
    for (uint32_t p = 0; p < W * H; p++) REQUIRE(err[p] == (p == at ? std::fabs(dal) : 0.0f));

    // no descriptor: no SSIM, the same error fields
    const gs_image_metrics plain = image_compare(dev, s, pa, pb, W, H);
    REQUIRE(plain.differing == 1 && plain.max_abs_at[3] == at && plain.sum_sq[1] == one.sum_sq[1] && plain.ssim_finite[0] == 0);

    try { image_compare(dev, s, pa, pb, 0, H); REQUIRE(false); } catch (const Error &e) { REQUIRE(e.status == GS_ERR_INVALID_ARGUMENT); }
    try { image_compare(dev, s, pa + 1, pb, W - 1, H); REQUIRE(false); } catch (const Error &e) { REQUIRE(e.status == GS_ERR_INVALID_ARGUMENT); }
    gs_image_compare_desc bad{};
    bad.data_range = 1.0f;
    bad.ssim_plane = (float *)plane.device_ptr();      // without the flag
    try { image_compare(dev, s, pa, pb, W, H, &bad); REQUIRE(false); } catch (const Error &e) { REQUIRE(e.status == GS_ERR_INVALID_ARGUMENT); }
    std::printf("cpp metrics OK\n");
    return 0;
}
