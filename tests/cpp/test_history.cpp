// GaussiansBuffer::snapshot / restore / concat, Snapshot and Selection::select_range (include/gs3d.hpp) through the C ABI:
// a grid of Gaussians is snapshotted, edited, exchanged back and forth (undo, redo, undo), concatenated with a copy of its
// own selected half, and the pasted part is range-selected.  Everything is compared on bytes.
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
    const uint32_t n = 2500;        // two full 1024-blocks and a partial one; not a multiple of 32
    const size_t nb = G::size();
    std::vector<Gaussian> all;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % 50) - 24.5f) * 0.125f;
        g.pos[1] = ((float)(i / 50) - 24.5f) * 0.0625f;
        g.pos[2] = -5.0f - (float)(i % 7) * 0.25f;
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = 180;
        g.scale[0] = 0.03f; g.scale[1] = 0.02f; g.scale[2] = 0.01f;
        for (int k = 0; k < 45; k++) g.sh[k] = (float)((int)((i + k) % 9) - 4) * 0.0625f;
        all.push_back(g);
    }
    GaussiansBuffer<G> buf(dev, all);
    const std::vector<uint8_t> original = buf.download(s);
    REQUIRE(original.size() == n * nb);

    // every third Gaussian
    Selection sel(dev, n);
    std::vector<uint32_t> words(sel.words(), 0u);
    uint64_t picked = 0;
    for (uint32_t i = 0; i < n; i += 3, picked++) words[i >> 5] |= 1u << (i & 31u);
    sel.upload(s, words);

    Snapshot snap = buf.snapshot(s, &sel);
    REQUIRE(snap.len() == n && snap.count() == picked);
    REQUIRE(snap.bytes() >= picked * nb && snap.bytes() <= picked * nb + 8 * sel.words() + 4096);
    // the snapshot keeps its own mask
    sel.clear(s);
    snap.selection(s, sel);
    REQUIRE(sel.download(s) == words && sel.count(s) == picked);

    gs_edit e{};
    e.flags = GS_EDIT_TRANSFORM | GS_EDIT_COLOR | GS_EDIT_OPACITY;
    gs_model_transform_pod_default(&e.transform);
    e.transform.pos[0] = 1.0f;
    e.transform.scale[0] = e.transform.scale[1] = e.transform.scale[2] = 2.0f;
    e.color[0] = 0.3f; e.color[4] = 0.3f; e.color[8] = 0.3f;
    e.opacity[0] = 0.37f;
    buf.edit(s, &sel, e);
    const std::vector<uint8_t> edited = buf.download(s);
    REQUIRE(edited != original);
    for (uint32_t i = 0; i < n; i++) {
        const bool same = std::memcmp(&edited[i * nb], &original[i * nb], nb) == 0;
        REQUIRE(same == (i % 3 != 0));
    }

    buf.restore(s, snap, true);      // undo
    REQUIRE(buf.download(s) == original);
    buf.restore(s, snap, true);      // redo
    REQUIRE(buf.download(s) == edited);
    buf.restore(s, snap, true);      // undo again
    REQUIRE(buf.download(s) == original);
    buf.restore(s, snap);            // the snapshot holds the edited records now: a plain restore pastes them
    REQUIRE(buf.download(s) == edited);
    {
        GaussiansBuffer<G> other = GaussiansBuffer<G>::new_empty(dev, n + 1);
        try { other.restore(s, snap); REQUIRE(false); } catch (const Error &) {}
    }

    // the buffer followed by a copy of its selected records
    std::vector<uint64_t> counts;
    GaussiansBuffer<G> both = GaussiansBuffer<G>::concat(s, {&buf, &buf}, {nullptr, &sel}, &counts);
    REQUIRE(counts.size() == 2 && counts[0] == n && counts[1] == picked && both.len() == n + picked);
    const std::vector<uint8_t> cat = both.download(s);
    REQUIRE(std::memcmp(cat.data(), edited.data(), n * nb) == 0);
    size_t at = n;
    for (uint32_t i = 0; i < n; i += 3, at++) REQUIRE(std::memcmp(&cat[at * nb], &edited[i * nb], nb) == 0);
    REQUIRE(at == both.len());
    GaussiansBuffer<G> whole = GaussiansBuffer<G>::concat(s, {&buf});
    REQUIRE(whole.download(s) == edited);
    try { GaussiansBuffer<G>::concat(s, {}); REQUIRE(false); } catch (const Error &) {}

    // the pasted part becomes the selection
    Selection pasted(dev, both.len());
    pasted.select_range(s, n, picked);
    REQUIRE(pasted.count(s) == picked);
    const std::vector<uint32_t> pw = pasted.download(s);
    for (size_t i = 0; i < both.len(); i++) REQUIRE(((pw[i >> 5] >> (i & 31u)) & 1u) == (i >= n ? 1u : 0u));
    pasted.select_range(s, 0, both.len(), GS_SEL_XOR);
    REQUIRE(pasted.count(s) == n);
    try { pasted.select_range(s, 1, both.len()); REQUIRE(false); } catch (const Error &) {}
    REQUIRE(pasted.count(s) == n);
    std::printf("cpp history OK\n");
    return 0;
}
