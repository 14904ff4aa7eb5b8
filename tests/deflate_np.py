"""The Huffman-only gzip member of DESIGN.md §3.15, restated in Python from the text alone: nothing here is shared with
csrc/gs_deflate.h.  member(data) is what gs_gzip_fast and Buffer.gzip_fast must return, byte for byte.  inputs() is the
list of cases the CPU and the GPU tests share."""
import heapq
import struct
import zlib

import numpy as np

CHUNK = 32768
HEADER = bytes([0x1f, 0x8b, 0x08, 0, 0, 0, 0, 0, 0, 0x03])
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def tree_depths(freq):
    """{symbol: depth} of the Huffman tree over the used symbols: merge the two smallest (weight, smallest symbol)"""
    heap = [(f, s, s) for s, f in enumerate(freq) if f > 0]      # (weight, smallest symbol, tree); a tree is a symbol or a pair
    heapq.heapify(heap)
    while len(heap) > 1:
        wa, ia, ta = heapq.heappop(heap)
        wb, ib, tb = heapq.heappop(heap)
        heapq.heappush(heap, (wa + wb, min(ia, ib), (ta, tb)))
    depths, stack = {}, [(heap[0][2], 0)]
    while stack:
        t, d = stack.pop()
        if isinstance(t, tuple):
            stack += [(t[0], d + 1), (t[1], d + 1)]
        else:
            depths[t] = d
    return depths


def code_lengths(freq, lmax):
    """(lengths, depth of the deepest leaf before limiting)"""
    freq = [int(f) for f in freq]
    lengths = [0] * len(freq)
    used = [s for s, f in enumerate(freq) if f > 0]
    if not used:
        return lengths, 0
    if len(used) == 1:
        lengths[used[0]] = 1
        return lengths, 1
    depths = tree_depths(freq)
    deepest = max(depths.values())
    if deepest <= lmax:
        for s, d in depths.items():
            lengths[s] = d
        return lengths, deepest
    cnt = [0] * (lmax + 1)
    for d in depths.values():
        cnt[min(d, lmax)] += 1
    total = sum(cnt[i] << (lmax - i) for i in range(1, lmax + 1))
    while total != 1 << lmax:
        cnt[lmax] -= 1
        i = max(j for j in range(1, lmax) if cnt[j] > 0)
        cnt[i] -= 1
        cnt[i + 1] += 2
        total -= 1
    ordered = sorted(used, key=lambda s: (-freq[s], s))
    handed = [l for l in range(1, lmax + 1) for _ in range(cnt[l])]
    assert len(handed) == len(ordered)
    for s, l in zip(ordered, handed):
        lengths[s] = l
    return lengths, deepest


def canonical(lengths):
    """RFC 1951 §3.2.2: {symbol: code}, the code's first bit being its most significant"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = {}
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


class Bits:
    """a list of bits in stream order"""

    def __init__(self):
        self.parts = []
        self.n = 0

    def value(self, v, k):          # a number: least significant bit first
        self.parts.append(((int(v) >> np.arange(k)) & 1).astype(np.uint8))
        self.n += k

    def code(self, c, k):           # a Huffman code: most significant bit first
        self.parts.append(((int(c) >> np.arange(k - 1, -1, -1)) & 1).astype(np.uint8))
        self.n += k

    def array(self, bits):
        self.parts.append(bits)
        self.n += len(bits)

    def pad(self):
        if self.n % 8:
            self.value(0, 8 - self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return np.packbits(np.concatenate(self.parts), bitorder="little").tobytes() if self.parts else b""


def close(b, final):
    if not final:
        b.value(0, 3)
    b.pad()
    return b.bytes() + (b"" if final else b"\x00\x00\xff\xff")


def fixed_literal(b, v):
    if v < 144:
        b.code(0x30 + v, 8)
    else:
        b.code(0x190 + v - 144, 9)


LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def fixed_match(b, length):
    k = max(i for i in range(29) if LENGTH_BASE[i] <= length) if length < 258 else 28
    sym = 257 + k
    if sym < 280:
        b.code(sym - 256, 7)
    else:
        b.code(0xc0 + sym - 280, 8)
    if LENGTH_EXTRA[k]:
        b.value(length - LENGTH_BASE[k], LENGTH_EXTRA[k])
    b.code(0, 5)


def run_block(chunk, final):
    n, v = len(chunk), chunk[0]
    b = Bits()
    b.value(1 if final else 0, 1)
    b.value(1, 2)
    fixed_literal(b, v)
    for _ in range((n - 1) // 258):
        fixed_match(b, 258)
    r = (n - 1) % 258
    if r >= 3:
        fixed_match(b, r)
    else:
        for _ in range(r):
            fixed_literal(b, v)
    b.code(0, 7)
    return close(b, final)


def dynamic_block(chunk, final):
    """(bytes, B, unlimited depth)"""
    a = np.frombuffer(chunk, np.uint8)
    freq = np.bincount(a, minlength=257)
    freq[256] = 1
    lengths, deepest = code_lengths(freq, 15)
    codes = canonical(lengths)
    sent = lengths + [1]                        # HLIT = 0: 257 lengths, HDIST = 0: the one distance code, length 1
    assert len(sent) == 258
    cl_lengths, _ = code_lengths(np.bincount(sent, minlength=19), 7)
    cl_codes = canonical(cl_lengths)
    hclen = 19
    while hclen > 4 and cl_lengths[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    b = Bits()
    b.value(1 if final else 0, 1)
    b.value(2, 2)
    b.value(0, 5)
    b.value(0, 5)
    b.value(hclen - 4, 4)
    for i in range(hclen):
        b.value(cl_lengths[CL_ORDER[i]], 3)
    for l in sent:
        b.code(cl_codes[l], cl_lengths[l])
    # the literals, vectorised: symbol i gives lengths[a[i]] bits, the code's most significant bit first
    ln = np.array(lengths[:256], np.int64)[a]
    cd = np.array([codes.get(s, 0) for s in range(256)], np.int64)[a]
    j = np.arange(15)
    bits = ((cd[:, None] >> np.maximum(ln[:, None] - 1 - j[None, :], 0)) & 1).astype(np.uint8)
    b.array(bits[j[None, :] < ln[:, None]])
    b.code(codes[256], lengths[256])
    B = b.n
    return close(b, final), B, deepest


def stored_block(chunk, final):
    n = len(chunk)
    return bytes([1 if final else 0]) + struct.pack("<HH", n & 0xffff, ~n & 0xffff) + bytes(chunk)


def block(chunk, final):
    """(bytes, form, unlimited depth) of one chunk"""
    n = len(chunk)
    if n >= 4 and chunk.count(chunk[0]) == n:
        return run_block(chunk, final), "run", 0
    data, B, deepest = dynamic_block(chunk, final)
    dyn = (B + 7) // 8 if final else (B + 3 + 7) // 8 + 4
    assert dyn == len(data)
    if dyn < 5 + n:
        return data, "dynamic", deepest
    return stored_block(chunk, final), "stored", deepest


def member(data, info=None):
    """the gzip member; info (a list) receives (form, unlimited depth) per chunk"""
    data = bytes(data)
    if not data:
        body = b"\x03\x00"
    else:
        parts = []
        for at in range(0, len(data), CHUNK):
            blk, form, deepest = block(data[at:at + CHUNK], at + CHUNK >= len(data))
            parts.append(blk)
            if info is not None:
                info.append((form, deepest))
        body = b"".join(parts)
    return HEADER + body + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)


def bound(n):
    return 18 + n + 5 * max(1, (n + CHUNK - 1) // CHUNK)


# ---- the shared inputs -------------------------------------------------------------------------------------------------

def skewed(n, seed):
    """seeded bytes with a geometric-like distribution: what a quantised column looks like"""
    rng = np.random.default_rng(seed)
    return np.minimum(rng.geometric(0.08, n) - 1, 255).astype(np.uint8).tobytes()


def fibonacci_chunk():
    """twenty values with counts 1, 1, 2, 3, ... 6765, one more value up to 32768 bytes, and 3 bytes of a second chunk"""
    counts = [1, 1]
    while len(counts) < 20:
        counts.append(counts[-1] + counts[-2])
    assert counts[-1] == 6765
    a = np.concatenate([np.full(c, 10 + i, np.uint8) for i, c in enumerate(counts)])
    a = np.concatenate([a, np.full(CHUNK - len(a), 200, np.uint8)])
    np.random.default_rng(5).shuffle(a)
    return a.tobytes() + bytes([1, 2, 3])


LENGTHS = (0, 1, 3, 4, 127, 128, 129, 32767, 32768, 32769, 65536, 3 * 32768 + 5)

_inputs = None


def inputs():
    """[(name, bytes)], built once"""
    global _inputs
    if _inputs is None:
        rng = np.random.default_rng(11)
        two = np.where(rng.random(CHUNK) < 0.3, 7, 250).astype(np.uint8).tobytes()
        _inputs = [("skewed_%d" % n, skewed(n, 100 + i)) for i, n in enumerate(LENGTHS)] + [
            ("constant", bytes([0x5a]) * CHUNK),
            ("constant_plus_one", bytes([0x5a]) * CHUNK + b"\x11"),
            ("uniform", rng.integers(0, 256, 2 * CHUNK + 100, dtype=np.uint8).tobytes()),
            ("three_forms", bytes(40000) + rng.integers(0, 256, 40000, dtype=np.uint8).tobytes() + bytes(5)),
            ("fibonacci", fibonacci_chunk()),
            ("two_values", two),
        ]
    return _inputs
