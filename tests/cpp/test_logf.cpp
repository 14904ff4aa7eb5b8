// gs::gs_logf (csrc/gs_convert.h) against the C library's logf over EVERY binary32 bit pattern, on up to 16 threads.
//
// gs_logf restates the algorithm glibc's logf uses; the golden file tests/golden/logf_v1.npz was recorded on glibc 2.35.  On
// that C library the two must agree bit for bit, the NaN patterns of negative and NaN arguments included (the count of
// differing inputs is printed and must be 0).  On any other C library a correctly working logf stays within 1 ulp of it and
// agrees about which inputs give a NaN: that is required, and the count of last-bit differences is printed without failing.
//
// Stand-alone: needs only gs_convert.h.  Build: g++ -std=c++17 -O2 -ffp-contract=off -pthread
#include <gnu/libc-version.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../wgpu-3dgs-core_amd/csrc/gs_convert.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// distance in units in the last place between two non-NaN floats (+0 and -0 are 0 apart)
static uint64_t ulp_distance(uint32_t a, uint32_t b) {
    const int64_t x = (a & 0x80000000u) ? -(int64_t)(a & 0x7fffffffu) : (int64_t)a;
    const int64_t y = (b & 0x80000000u) ? -(int64_t)(b & 0x7fffffffu) : (int64_t)b;
    return (uint64_t)(x > y ? x - y : y - x);
}

int main() {
    const char *ver = gnu_get_libc_version();
    const bool golden_libc = std::strcmp(ver, "2.35") == 0;
    unsigned hw = std::thread::hardware_concurrency();
    const unsigned threads = hw == 0 ? 4 : hw > 16 ? 16 : hw;
    std::atomic<uint64_t> differing{0}, beyond{0};
    std::atomic<uint32_t> first_bad{0};
    std::vector<std::thread> pool;
    const uint64_t total = 1ull << 32, per = (total + threads - 1) / threads;
    for (unsigned t = 0; t < threads; t++) {
        pool.emplace_back([&, t] {
            uint64_t diff = 0, bad = 0;
            const uint64_t a = t * per, b = a + per < total ? a + per : total;
            for (uint64_t u = a; u < b; u++) {
                float x;
                const uint32_t ux = (uint32_t)u;
                std::memcpy(&x, &ux, 4);
                volatile float xin = x;      // the C library's function, not a folded constant
                const uint32_t mine = bits(gs::gs_logf(x)), ref = bits(std::log(xin));
                if (mine == ref) continue;
                diff++;
                const bool nan_m = (mine & 0x7fffffffu) > 0x7f800000u, nan_r = (ref & 0x7fffffffu) > 0x7f800000u;
                if (nan_m != nan_r || (!nan_m && ulp_distance(mine, ref) > 1)) {
                    if (bad++ == 0) first_bad = ux;
                }
            }
            differing += diff;
            beyond += bad;
        });
    }
    for (auto &th : pool) th.join();
    std::printf("glibc %s, %u threads: gs_logf differs from logf on %llu of 4294967296 inputs, %llu of them by more than 1 ulp or in NaN-ness\n",
                ver, threads, (unsigned long long)differing.load(), (unsigned long long)beyond.load());
    if (beyond.load()) {
        std::printf("FAIL: first input beyond 1 ulp: 0x%08x\n", first_bad.load());
        return 1;
    }
    if (golden_libc && differing.load()) {
        std::printf("FAIL: this is the C library the golden file was recorded on; the two must be bit-equal\n");
        return 1;
    }
    std::printf("cpp logf OK\n");
    return 0;
}
