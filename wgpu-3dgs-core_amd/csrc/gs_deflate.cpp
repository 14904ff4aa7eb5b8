// gs_deflate.cpp — the host encoder of the Huffman-only gzip member: gs_gzip_fast, gs_gzip_fast_bound.  Every
// rule is gs_deflate.h's, shared with the device kernels (gs_deflate_kernels.h); the chunks are independent, so they are sized,
// placed and then written by several threads, and the bytes do not depend on how many.  Host side only, no HIP.
#include <zlib.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "gs_deflate.h"
#include "gs_internal.h"

namespace {

// fn(first, end) over [0, n) on GS3D_HOST_THREADS threads (default: the hardware's, at most 32), one range each
template <class F>
void chunk_parallel_for(size_t n, F fn) {
    const unsigned hw = std::thread::hardware_concurrency();
    size_t threads = n < 8 ? 1 : (hw ? (hw > 32 ? 32 : hw) : 4);
    if (const char *e = std::getenv("GS3D_HOST_THREADS")) threads = std::atoi(e) > 0 ? (size_t)std::atoi(e) : threads;
    if (threads > n) threads = n;
    if (threads <= 1) {
        fn((size_t)0, n);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (n + threads - 1) / threads;
    for (size_t t = 0; t < threads; t++) {
        const size_t a = t * per, b = a + per < n ? a + per : n;
        if (a >= b) break;
        pool.emplace_back([=] { fn(a, b); });
    }
    for (auto &th : pool) th.join();
}

struct ChunkPlan {
    uint32_t form, bytes, hdr_bits;
};

// One chunk: its form and size, and with `out` its block (plan.bytes of them).  `image` holds DF_SLOT bytes.
ChunkPlan encode_chunk(const uint8_t *src, uint32_t len, bool final, uint8_t *out, uint8_t *image, gs::DfHuff &h) {
    ChunkPlan p{};
    uint32_t hist[gs::DF_SYMS];
    std::memset(hist, 0, sizeof(hist));
    for (uint32_t i = 0; i < len; i++) hist[src[i]]++;
    hist[gs::DF_EOB] = 1;
    if (len >= 4 && hist[src[0]] == len) {
        p.form = gs::DF_FORM_RUN;
        p.bytes = gs::df_run_block(image, src[0], len, final);
        if (out) std::memcpy(out, image, p.bytes);
        return p;
    }
    uint8_t lens[gs::DF_SYMS];
    uint16_t codes[gs::DF_SYMS];
    p.form = gs::df_plan_chunk(hist, len, final, lens, codes, image, h, &p.hdr_bits, &p.bytes);
    if (!out) return p;
    if (p.form == gs::DF_FORM_STORED) {
        gs::df_stored_header(out, len, final);
        std::memcpy(out + 5, src, len);
        return p;
    }
    // the header again, straight into the block, and the literals behind it
    gs::DfBits w{out, 0, 0, 0};
    gs::df_dyn_header(w, lens, final, h);
    for (uint32_t i = 0; i < len; i++) w.put(codes[src[i]], lens[src[i]]);
    w.put(codes[gs::DF_EOB], lens[gs::DF_EOB]);
    gs::df_close_block(w, final);
    return p;
}

}  // namespace

extern "C" size_t gs_gzip_fast_bound(size_t len) { return (size_t)gs::df_bound(len); }

void gs_gzip_fast_frame(uint8_t *out, size_t body, uint32_t crc, size_t len) {
    static const uint8_t head[10] = {0x1f, 0x8b, 0x08, 0, 0, 0, 0, 0, 0, 0x03};
    std::memcpy(out, head, 10);
    uint8_t *t = out + 10 + body;
    const uint32_t isize = (uint32_t)(len & 0xffffffffu);
    for (int k = 0; k < 4; k++) {
        t[k] = (uint8_t)(crc >> (8 * k));
        t[4 + k] = (uint8_t)(isize >> (8 * k));
    }
}

// crc(A B) = crc(A) x^(8 |B|) mod P xor crc(B).  Every chunk but the last has 32768 bytes, so its multiplier is one constant
// (zlib's crc32_combine would work it out again per chunk: 30 ms for the 20 000 chunks of a 10 M scene); the last chunk, of
// any length, goes through crc32_combine.
uint32_t gs_gzip_fast_fold_crcs(const uint32_t *crcs, size_t chunks, size_t len) {
    static constexpr gs::DfCrcTables tables = gs::df_make_crc_tables();
    static constexpr uint32_t chunk_mul = gs::df_crc_mul(tables.mul[gs::DF_THREADS - 1u], tables.mul[1]);      // x^(8 * 128 * 256)
    uint32_t crc = 0;
    for (size_t c = 0; c + 1 < chunks; c++) crc = gs::df_crc_mul(crc, chunk_mul) ^ crcs[c];
    if (!chunks) return 0;
    const size_t last = len - (chunks - 1) * gs::DF_CHUNK;
    return (uint32_t)crc32_combine(crc, crcs[chunks - 1], (z_off_t)last);
}

extern "C" gs_status gs_gzip_fast(const void *bytes, size_t len, void *out, size_t capacity, size_t *bytes_out) {
    if ((len && !bytes) || !bytes_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    const uint8_t *in = (const uint8_t *)bytes;
    uint8_t *dst = (uint8_t *)out;
    if (len == 0) {      // an empty input is the empty fixed block 03 00
        *bytes_out = 20;
        if (!out) return GS_OK;
        if (capacity < 20) return gs_fail(GS_ERR_INVALID_ARGUMENT, capacity, 20, 0, "output buffer too small: %zu < %zu", capacity, (size_t)20);
        dst[10] = 0x03;
        dst[11] = 0x00;
        gs_gzip_fast_frame(dst, 2, 0, 0);
        return GS_OK;
    }
    const size_t chunks = (size_t)gs::df_chunks(len);
    std::vector<uint64_t> offset;
    std::vector<uint32_t> crcs;
    try {
        offset.resize(chunks + 1);
        crcs.resize(chunks);
    } catch (const std::bad_alloc &) {
        return gs_fail(GS_ERR_OUT_OF_MEMORY, chunks * 12, 0, 0, "out of memory compressing %zu bytes", len);
    }
    auto chunk_len = [=](size_t c) { return (uint32_t)(c + 1 < chunks ? gs::DF_CHUNK : len - c * gs::DF_CHUNK); };
    // sizes first: the capacity is checked before a byte is written, and every chunk then knows its place
    chunk_parallel_for(chunks, [&](size_t a, size_t b) {
        std::vector<uint8_t> image(gs::DF_SLOT);
        gs::DfHuff h;
        for (size_t c = a; c < b; c++) {
            const uint8_t *src = in + c * gs::DF_CHUNK;
            offset[c + 1] = encode_chunk(src, chunk_len(c), c + 1 == chunks, nullptr, image.data(), h).bytes;
            if (out) crcs[c] = (uint32_t)crc32(0L, src, chunk_len(c));
        }
    });
    offset[0] = 0;
    for (size_t c = 0; c < chunks; c++) offset[c + 1] += offset[c];
    const size_t body = (size_t)offset[chunks], total = 18 + body;
    *bytes_out = total;
    if (!out) return GS_OK;
    if (capacity < total) return gs_fail(GS_ERR_INVALID_ARGUMENT, capacity, total, 0, "output buffer too small: %zu < %zu", capacity, total);
    chunk_parallel_for(chunks, [&](size_t a, size_t b) {
        std::vector<uint8_t> image(gs::DF_SLOT);
        gs::DfHuff h;
        for (size_t c = a; c < b; c++)
            encode_chunk(in + c * gs::DF_CHUNK, chunk_len(c), c + 1 == chunks, dst + 10 + offset[c], image.data(), h);
    });
    gs_gzip_fast_frame(dst, body, gs_gzip_fast_fold_crcs(crcs.data(), chunks, len), len);
    return GS_OK;
}
