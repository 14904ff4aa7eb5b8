// gs_deflate.h — the Huffman-only gzip member of DESIGN.md §3.15 as ONE set of host + device functions (the gs_convert.h
// pattern): code lengths, canonical codes, the block headers, the run block and the size rule.  The host encoder
// (gs_deflate.cpp) and the device kernels (gs_deflate_kernels.h) both call the functions below, so the two members are the
// same bytes by construction; tests/deflate_np.py restates the format independently.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define GS_DF_HD __host__ __device__
#else
#define GS_DF_HD
#endif

namespace gs {

constexpr uint32_t DF_CHUNK = 32768;       // input bytes per DEFLATE block
constexpr uint32_t DF_SYMS = 257;          // the 256 literals and end of block
constexpr uint32_t DF_EOB = 256;
constexpr uint32_t DF_LMAX = 15;           // literal / length code
constexpr uint32_t DF_CL_SYMS = 19;
constexpr uint32_t DF_CL_LMAX = 7;         // code-length code
// a block's image: a stored block is 5 + len bytes, a dynamic one is taken only when it is shorter, a run block is far below
// both; rounded up so that whole 16-byte words can be copied
constexpr uint32_t DF_SLOT = DF_CHUNK + 16;
constexpr uint32_t DF_FORM_STORED = 0, DF_FORM_RUN = 1, DF_FORM_DYNAMIC = 2;

// member <= 18 + len + 5 max(1, chunks)
GS_DF_HD inline uint64_t df_chunks(uint64_t len) { return (len + DF_CHUNK - 1u) / DF_CHUNK; }
GS_DF_HD inline uint64_t df_bound(uint64_t len) {
    const uint64_t c = df_chunks(len);
    return 18u + len + 5u * (c ? c : 1u);
}

// bits go out LSB-first into bytes; Huffman codes are handed over already reversed (df_canonical)
struct DfBits {
    uint8_t *p;
    uint64_t acc;
    uint32_t n, pos;
    GS_DF_HD void put(uint32_t v, uint32_t k) {
        acc |= (uint64_t)v << n;
        n += k;
        while (n >= 8u) {
            p[pos++] = (uint8_t)acc;
            acc >>= 8;
            n -= 8u;
        }
    }
    GS_DF_HD uint32_t bits() const { return pos * 8u + n; }
    GS_DF_HD void flush() {      // zero pad to the byte boundary
        if (n) {
            p[pos++] = (uint8_t)acc;
            acc = 0;
            n = 0;
        }
    }
};

// scratch of df_code_lengths and df_dyn_header (on the device: LDS of the chunk's workgroup, used by one lane)
struct DfHuff {
    uint32_t heap[DF_SYMS];          // keys of the live nodes: weight << 9 | smallest symbol of the subtree
    uint16_t node_of[DF_SYMS];       // smallest symbol -> the live node that has it
    uint16_t parent[2 * DF_SYMS];
    uint8_t depth[2 * DF_SYMS];
    uint32_t cl_freq[DF_CL_SYMS];
    uint8_t cl_len[DF_CL_SYMS];
    uint16_t cl_code[DF_CL_SYMS];
};

GS_DF_HD inline void df_sift_down(uint32_t *heap, uint32_t m, uint32_t i) {
    const uint32_t v = heap[i];
    for (;;) {
        uint32_t c = 2u * i + 1u;
        if (c >= m) break;
        if (c + 1u < m && heap[c + 1u] < heap[c]) c++;
        if (heap[c] >= v) break;
        heap[i] = heap[c];
        i = c;
    }
    heap[i] = v;
}
GS_DF_HD inline uint32_t df_heap_pop(uint32_t *heap, uint32_t &m) {
    const uint32_t top = heap[0];
    heap[0] = heap[--m];
    if (m) df_sift_down(heap, m, 0);
    return top;
}
GS_DF_HD inline void df_heap_push(uint32_t *heap, uint32_t &m, uint32_t v) {
    uint32_t i = m++;
    while (i) {
        const uint32_t p = (i - 1u) / 2u;
        if (heap[p] <= v) break;
        heap[i] = heap[p];
        i = p;
    }
    heap[i] = v;
}

// §3.15 "code lengths": len[s] for the n <= 257 counts freq[s] (sum < 2^23), limited to lmax <= 15.  Returns the depth of the
// deepest leaf BEFORE limiting.  The keys (weight, smallest symbol) of the live nodes are distinct, so the tree is unique.
GS_DF_HD inline uint32_t df_code_lengths(const uint32_t *freq, uint32_t n, uint32_t lmax, uint8_t *len, DfHuff &h) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; s++) {
        len[s] = 0;
        if (freq[s]) {
            h.heap[m++] = freq[s] << 9 | s;
            h.node_of[s] = (uint16_t)s;
        }
    }
    if (m == 0) return 0;
    if (m == 1) {
        len[h.heap[0] & 511u] = 1;
        return 1;
    }
    const uint32_t used = m;
    for (uint32_t i = m / 2u; i-- > 0;) df_sift_down(h.heap, m, i);
    uint32_t next = n;      // leaves are nodes 0..n-1, parents follow in the order they are made
    while (m > 1) {
        const uint32_t a = df_heap_pop(h.heap, m), b = df_heap_pop(h.heap, m);
        const uint32_t ia = a & 511u, ib = b & 511u, idx = ia < ib ? ia : ib;
        h.parent[h.node_of[ia]] = (uint16_t)next;
        h.parent[h.node_of[ib]] = (uint16_t)next;
        h.node_of[idx] = (uint16_t)next;
        df_heap_push(h.heap, m, ((a >> 9) + (b >> 9)) << 9 | idx);
        next++;
    }
    // a parent's number is above its children's: one walk down from the root
    h.depth[next - 1u] = 0;
    for (uint32_t v = next - 1u; v-- > n;) h.depth[v] = (uint8_t)(h.depth[h.parent[v]] + 1u);
    uint32_t deepest = 0;
    for (uint32_t s = 0; s < n; s++)
        if (freq[s]) {
            const uint32_t d = h.depth[h.parent[s]] + 1u;
            len[s] = (uint8_t)d;      // at most 22 for sums below 2^16: the Fibonacci bound
            if (d > deepest) deepest = d;
        }
    if (deepest <= lmax) return deepest;
    // the length-limiting procedure
    uint32_t cnt[16];
    for (uint32_t i = 0; i < 16u; i++) cnt[i] = 0;
    for (uint32_t s = 0; s < n; s++)
        if (freq[s]) cnt[len[s] < lmax ? len[s] : lmax]++;
    uint32_t total = 0;
    for (uint32_t i = 1; i <= lmax; i++) total += cnt[i] << (lmax - i);
    while (total != 1u << lmax) {
        cnt[lmax]--;
        uint32_t i = lmax - 1u;
        while (i > 0 && cnt[i] == 0) i--;
        if (i == 0) break;      // cannot happen: the folded counts over-fill the code space by less than cnt[lmax]
        cnt[i]--;
        cnt[i + 1u] += 2u;
        total--;
    }
    // ascending lengths to the symbols by (count descending, symbol ascending): the heap sorts them
    m = 0;
    for (uint32_t s = 0; s < n; s++)
        if (freq[s]) h.heap[m++] = (0x7fffffu - freq[s]) << 9 | s;
    for (uint32_t i = m / 2u; i-- > 0;) df_sift_down(h.heap, m, i);
    uint32_t l = 1;
    for (uint32_t k = 0; k < used; k++) {
        const uint32_t s = df_heap_pop(h.heap, m) & 511u;
        while (l < lmax && cnt[l] == 0) l++;
        len[s] = (uint8_t)l;
        cnt[l]--;
    }
    return deepest;
}

GS_DF_HD inline uint32_t df_reverse(uint32_t v, uint32_t k) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < k; i++) r |= ((v >> i) & 1u) << (k - 1u - i);
    return r;
}

// RFC 1951 §3.2.2, each code reversed so that DfBits::put sends its first bit first
GS_DF_HD inline void df_canonical(const uint8_t *len, uint32_t n, uint16_t *code) {
    uint32_t count[16], next[16];
    for (uint32_t i = 0; i < 16u; i++) count[i] = 0;
    for (uint32_t s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (uint32_t i = 1; i < 16u; i++) {
        c = (c + count[i - 1u]) << 1;
        next[i] = c;
    }
    for (uint32_t s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)df_reverse(next[len[s]]++, len[s]) : (uint16_t)0;
}

// The header of a dynamic block for the 257 lengths `len`: BFINAL, BTYPE = 10, HLIT = 0, HDIST = 0, HCLEN, the code-length
// code, then the 258 lengths (the single distance code has length 1), one symbol each.  Bits are left in `w` unflushed.
GS_DF_HD inline void df_dyn_header(DfBits &w, const uint8_t *len, bool final, DfHuff &h) {
    const uint8_t order[DF_CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (uint32_t i = 0; i < DF_CL_SYMS; i++) h.cl_freq[i] = 0;
    for (uint32_t s = 0; s < DF_SYMS; s++) h.cl_freq[len[s]]++;
    h.cl_freq[1]++;
    df_code_lengths(h.cl_freq, DF_CL_SYMS, DF_CL_LMAX, h.cl_len, h);
    df_canonical(h.cl_len, DF_CL_SYMS, h.cl_code);
    uint32_t hclen = DF_CL_SYMS;
    while (hclen > 4u && h.cl_len[order[hclen - 1u]] == 0) hclen--;
    w.put(final ? 1u : 0u, 1);
    w.put(2u, 2);
    w.put(0u, 5);
    w.put(0u, 5);
    w.put(hclen - 4u, 4);
    for (uint32_t i = 0; i < hclen; i++) w.put(h.cl_len[order[i]], 3);
    for (uint32_t s = 0; s < DF_SYMS; s++) w.put(h.cl_code[len[s]], h.cl_len[len[s]]);
    w.put(h.cl_code[1], h.cl_len[1]);
}

// the size rule: the bytes a dynamic block of B bits takes, with the empty stored block behind a block that is not the last
GS_DF_HD inline uint32_t df_dyn_bytes(uint32_t B, bool final) { return final ? (B + 7u) / 8u : (B + 3u + 7u) / 8u + 4u; }

// what follows a run or dynamic block: the last one is padded, any other gets an empty stored block (000, pad, 00 00 ff ff)
GS_DF_HD inline void df_close_block(DfBits &w, bool final) {
    if (!final) w.put(0u, 3);
    w.flush();
    if (!final) {
        w.put(0xffff0000u, 32);
    }
}

// a literal / a match length in the fixed code (RFC 1951 §3.2.6)
GS_DF_HD inline void df_fixed_literal(DfBits &w, uint32_t b) {
    if (b < 144u) w.put(df_reverse(0x30u + b, 8), 8);
    else w.put(df_reverse(0x190u + (b - 144u), 9), 9);
}
GS_DF_HD inline void df_fixed_match(DfBits &w, uint32_t length) {      // 3..258 at distance 1
    uint32_t sym, extra = 0, ebits = 0;
    if (length == 258u) sym = 285u;
    else if (length < 11u) sym = 254u + length;
    else {
        // groups of four codes share a number of extra bits: 11..18 one bit, 19..34 two, ...
        uint32_t e = 1, base = 11u, code = 265u;
        while (length >= base + (4u << e)) {
            base += 4u << e;
            code += 4u;
            e++;
        }
        sym = code + ((length - base) >> e);
        extra = (length - base) & ((1u << e) - 1u);
        ebits = e;
    }
    if (sym < 280u) w.put(df_reverse(sym - 256u, 7), 7);
    else w.put(df_reverse(0xc0u + (sym - 280u), 8), 8);
    if (ebits) w.put(extra, ebits);
    w.put(0u, 5);      // distance code 0: distance 1
}

// The run form: len >= 4 equal bytes `b` as a fixed-Huffman block, closed; returns its size in bytes.
GS_DF_HD inline uint32_t df_run_block(uint8_t *out, uint32_t b, uint32_t len, bool final) {
    DfBits w{out, 0, 0, 0};
    w.put(final ? 1u : 0u, 1);
    w.put(1u, 2);
    df_fixed_literal(w, b);
    const uint32_t full = (len - 1u) / 258u, r = (len - 1u) % 258u;
    for (uint32_t i = 0; i < full; i++) df_fixed_match(w, 258u);
    if (r >= 3u) df_fixed_match(w, r);
    else
        for (uint32_t i = 0; i < r; i++) df_fixed_literal(w, b);
    w.put(0u, 7);      // end of block
    df_close_block(w, final);
    return w.pos;
}

// the 5 bytes in front of a stored block of len <= 32768 bytes
GS_DF_HD inline void df_stored_header(uint8_t *out, uint32_t len, bool final) {
    out[0] = final ? 1 : 0;
    out[1] = (uint8_t)len;
    out[2] = (uint8_t)(len >> 8);
    out[3] = (uint8_t)~len;
    out[4] = (uint8_t)(~len >> 8);
}

// What one lane decides about a chunk that is not a run, from its byte counts (hist[256] = 1): the code lengths, and the
// form by the size rule.  A dynamic chunk gets its codes and has its header in `image` (flushed: *hdr_bits of them count).
GS_DF_HD inline uint32_t df_plan_chunk(const uint32_t *hist, uint32_t len, bool final, uint8_t *lens, uint16_t *codes, uint8_t *image,
                                       DfHuff &h, uint32_t *hdr_bits, uint32_t *bytes) {
    df_code_lengths(hist, DF_SYMS, DF_LMAX, lens, h);
    DfBits w{image, 0, 0, 0};
    df_dyn_header(w, lens, final, h);
    uint32_t B = w.bits();
    *hdr_bits = B;
    w.flush();
    for (uint32_t s = 0; s < DF_SYMS; s++) B += hist[s] * lens[s];
    const uint32_t dyn = df_dyn_bytes(B, final);
    if (dyn < 5u + len) {
        df_canonical(lens, DF_SYMS, codes);
        *bytes = dyn;
        return DF_FORM_DYNAMIC;
    }
    *bytes = 5u + len;
    return DF_FORM_STORED;
}

// ---- CRC-32 (the gzip trailer) -----------------------------------------------------------------------------------------
// reflected polynomial; a polynomial's coefficient of x^k is bit 31 - k, as in zlib's crc32_combine
constexpr uint32_t DF_CRC_POLY = 0xedb88320u;
constexpr uint32_t DF_PIECE = 128;         // bytes of a chunk one device thread takes
constexpr uint32_t DF_THREADS = DF_CHUNK / DF_PIECE;

GS_DF_HD constexpr uint32_t df_crc_mul(uint32_t a, uint32_t b) {      // a b mod P
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ DF_CRC_POLY : b >> 1;
    }
    return p;
}

// byte[v]: the CRC register after the byte v; mul[k] = x^(8 DF_PIECE k) mod P: crc(A B) = crc(A) mul[|B| / DF_PIECE] ^ crc(B)
struct DfCrcTables {
    uint32_t byte[256];
    uint32_t mul[DF_THREADS];
};
constexpr DfCrcTables df_make_crc_tables() {
    DfCrcTables t{};
    for (uint32_t v = 0; v < 256u; v++) {
        uint32_t c = v;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ DF_CRC_POLY : c >> 1;
        t.byte[v] = c;
    }
    uint32_t step = 0x80000000u;      // x^0
    for (uint32_t k = 0; k < 8u * DF_PIECE; k++) step = (step & 1u) ? (step >> 1) ^ DF_CRC_POLY : step >> 1;
    t.mul[0] = 0x80000000u;
    for (uint32_t k = 1; k < DF_THREADS; k++) t.mul[k] = df_crc_mul(t.mul[k - 1u], step);
    return t;
}

}  // namespace gs
