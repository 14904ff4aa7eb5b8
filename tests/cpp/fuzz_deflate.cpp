// Stand-alone driver of the host encoder gs_gzip_fast for an AddressSanitizer + UBSan build
// (tests/test_deflate_sanitizers.py): g++ -fsanitize=address,undefined fuzz_deflate.cpp gs_deflate.cpp gs_spz.cpp gs_ply.cpp -lz.
// Every input — the fixed cases of the format's tests and mutations of them — is encoded into a buffer of EXACTLY the size
// the size query returned (an overrun by one byte is a report), inflated by zlib and by gs_spz_decompress, and compared.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gs3d.h"

// the product's gs_fail lives in the HIP translation unit; the encoder only needs it to return the code
extern "C++" gs_status gs_fail(gs_status code, uint64_t, uint64_t, uint64_t, const char *, ...) { return code; }

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

typedef std::vector<uint8_t> Bytes;

static Bytes skewed(size_t n) {      // small values are frequent, as in a quantised column
    Bytes v(n);
    for (auto &b : v) {
        uint32_t k = 0;
        while (k < 255 && rnd() % 100 >= 8) k++;
        b = (uint8_t)k;
    }
    return v;
}
static Bytes uniform(size_t n) {
    Bytes v(n);
    for (auto &b : v) b = (uint8_t)rnd();
    return v;
}
static Bytes fibonacci() {
    Bytes v;
    uint32_t a = 1, b = 1;
    for (int i = 0; i < 20; i++) {
        v.insert(v.end(), a, (uint8_t)(10 + i));
        const uint32_t c = a + b;
        a = b;
        b = c;
    }
    v.resize(32768, 200);
    for (size_t i = v.size() - 1; i > 0; i--) std::swap(v[i], v[rnd() % (i + 1)]);
    v.push_back(1);
    v.push_back(2);
    v.push_back(3);
    return v;
}

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
            failures++;                   \
            return;                       \
        }                                 \
    } while (0)

static void round_trip(const char *name, const Bytes &in) {
    size_t size = 0;
    CHECK(gs_gzip_fast(in.data(), in.size(), nullptr, 0, &size) == GS_OK, "%s: size query", name);
    CHECK(size <= gs_gzip_fast_bound(in.size()), "%s: %zu bytes exceed the bound %zu", name, size, gs_gzip_fast_bound(in.size()));
    Bytes z(size);      // exactly: one byte more written is a heap overflow
    size_t written = 0;
    CHECK(gs_gzip_fast(in.data(), in.size(), z.data(), z.size(), &written) == GS_OK && written == size, "%s: encode", name);
    if (size > 1) {
        Bytes small(size - 1, 0xee);
        size_t need = 0;
        CHECK(gs_gzip_fast(in.data(), in.size(), small.data(), small.size(), &need) == GS_ERR_INVALID_ARGUMENT && need == size, "%s: short capacity", name);
        for (uint8_t b : small) CHECK(b == 0xee, "%s: a refused call wrote", name);
    }
    // zlib, as a gzip stream: the end is reached with every byte consumed
    Bytes back(in.size() + 1);
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    CHECK(inflateInit2(&zs, 16 + MAX_WBITS) == Z_OK, "%s: inflateInit2", name);
    zs.next_in = z.data();
    zs.avail_in = (uInt)z.size();
    zs.next_out = back.data();
    zs.avail_out = (uInt)back.size();
    const int rc = inflate(&zs, Z_FINISH);
    const size_t got = back.size() - zs.avail_out, left = zs.avail_in;
    inflateEnd(&zs);
    CHECK(rc == Z_STREAM_END && left == 0, "%s: inflate returned %d with %zu bytes left", name, rc, left);
    CHECK(got == in.size() && (got == 0 || std::memcmp(back.data(), in.data(), got) == 0), "%s: inflated bytes differ", name);
    // the project's own bounded gunzip
    size_t n2 = 0;
    CHECK(gs_spz_decompress(z.data(), z.size(), nullptr, 0, &n2) == GS_OK && n2 == in.size(), "%s: gs_spz_decompress size", name);
    Bytes back2(n2 + 1);
    CHECK(gs_spz_decompress(z.data(), z.size(), back2.data(), n2, &n2) == GS_OK, "%s: gs_spz_decompress", name);
    CHECK(n2 == 0 || std::memcmp(back2.data(), in.data(), n2) == 0, "%s: gs_spz_decompress bytes differ", name);
}

int main(int argc, char **argv) {
    const int mutations = argc > 1 ? std::atoi(argv[1]) : 40;
    std::vector<std::pair<const char *, Bytes>> cases;
    const size_t lengths[] = {0, 1, 3, 4, 127, 128, 129, 32767, 32768, 32769, 65536, 3 * 32768 + 5};
    for (size_t n : lengths) cases.push_back({"skewed", skewed(n)});
    cases.push_back({"constant", Bytes(32768, 0x5a)});
    Bytes c1(32768, 0x5a);
    c1.push_back(0x11);
    cases.push_back({"constant plus one", c1});
    cases.push_back({"uniform", uniform(2 * 32768 + 100)});
    Bytes three(40000, 0), r = uniform(40000);
    three.insert(three.end(), r.begin(), r.end());
    three.insert(three.end(), 5, 0);
    cases.push_back({"three forms", three});
    cases.push_back({"fibonacci", fibonacci()});
    Bytes two(32768);
    for (auto &b : two) b = rnd() % 10 < 3 ? 7 : 250;
    cases.push_back({"two values", two});
    for (auto &c : cases) round_trip(c.first, c.second);
    // mutations: a case cut somewhere, with a run written over a part of it and a few bytes changed
    for (int k = 0; k < mutations && !failures; k++) {
        Bytes m = cases[rnd() % cases.size()].second;
        if (m.empty()) m = skewed(1 + rnd() % 70000);
        m.resize(1 + rnd() % m.size());
        if (rnd() % 2) {
            const size_t a = rnd() % m.size(), n = rnd() % (m.size() - a + 1);
            std::memset(m.data() + a, (int)(rnd() & 255), n);
        }
        for (int j = 0; j < 8; j++) m[rnd() % m.size()] = (uint8_t)rnd();
        round_trip("mutation", m);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("fuzz OK: %zu cases, %d mutations\n", cases.size(), mutations);
    return 0;
}
