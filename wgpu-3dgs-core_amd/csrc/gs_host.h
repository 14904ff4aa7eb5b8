// gs_host.h — what the HIP translation units of libgs3d_hip.so share: the error macros, the objects behind
// the handles of include/gs3d.h that more than one unit touches, and the few host functions that cross a unit boundary
// (namespace gsh; each says which unit defines it).  gs_internal.h stays free of HIP: gs_ply.cpp and gs_spz.cpp are also
// built by a plain C++ compiler.
#pragma once

#include "gs_internal.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "gs_kernel_lib.h"
#include "gs_policy.h"

// GS_HIP_AS: the call goes through an owner and keeps the wording it had as a plain HIP call
#define GS_HIP_AS(text, expr)                                                                     \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return gs_fail(e_ == hipErrorOutOfMemory ? GS_ERR_OUT_OF_MEMORY : GS_ERR_HIP,         \
                           (uint64_t)e_, 0, 0, "%s failed: %s", text, hipGetErrorString(e_));     \
    } while (0)
#define GS_HIP(expr) GS_HIP_AS(#expr, expr)

#define GS_TRY(expr)                  \
    do {                              \
        gs_status s_ = (expr);        \
        if (s_ != GS_OK) return s_;   \
    } while (0)

// one kernel instance per POD layout: table[sh][cov]
#define GS_CFG_TABLE(kernel)                                                                     \
    {                                                                                            \
        {kernel<0, 0>, kernel<0, 1>, kernel<0, 2>}, {kernel<1, 0>, kernel<1, 1>, kernel<1, 2>},  \
        {kernel<2, 0>, kernel<2, 1>, kernel<2, 2>}, {kernel<3, 0>, kernel<3, 1>, kernel<3, 2>},  \
    }

// ------------------------------------------------------------------------------------------------
// device / stream / buffer
// ------------------------------------------------------------------------------------------------

// ---- owners: each holds ONE resource and lets go of it in its destructor, with the device of its holder current ----
// They serve the temporaries of a call and the members of the handle objects alike: a function that holds one can return
// early with GS_TRY / GS_HIP, and the destroy function of a handle is a `delete`.  hipFree waits for the device, but the
// functions do not lean on that: whoever has enqueued work on an owner's memory synchronises the stream(s) before it
// returns, on every path (the few returns and destroy functions that rely on the wait instead say so).  An enqueue-only
// call hands its memory on: release().
namespace gsh {
// (gs_core.hip) *out = `bytes` of device memory, or null and GS_ERR_OUT_OF_MEMORY / GS_ERR_HIP with the message
// "<what> failed: ..." (gs_error_info: a = the HIP error, b as given: the size, or 0 at the sites that never reported one)
gs_status dev_alloc(void **out, size_t bytes, uint64_t b, const char *what);

struct NoCopy {
    NoCopy() noexcept = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};
struct DevMem : NoCopy {
    ~DevMem() noexcept { if (ptr) (void)hipFree(ptr); }
    // through dev_alloc, with its error (once per owner) ... and for the sites that word the failure themselves
    gs_status alloc(size_t bytes, uint64_t b, const char *what) noexcept { return dev_alloc(&ptr, bytes, b, what); }
    hipError_t alloc_raw(size_t bytes) noexcept { return hipMalloc(&ptr, bytes); }
    // a member that is allocated anew: null when this succeeds (or held nothing), untouched when hipFree fails
    hipError_t free() noexcept {
        const hipError_t e = ptr ? hipFree(ptr) : hipSuccess;
        if (e == hipSuccess) ptr = nullptr;
        return e;
    }
    void *release() noexcept { void *p = ptr; ptr = nullptr; return p; }
    void *ptr = nullptr;
};
// (converts to its handle, so that a GS_HIP around a call on a member event words its failure as it always did)
struct Event : NoCopy {
    ~Event() noexcept { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDisableTiming) noexcept { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const noexcept { return e; }
    hipEvent_t e = nullptr;
};
struct Stream : NoCopy {     // hipStreamNonBlocking, or adopted by whoever made it another way
    ~Stream() noexcept { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() noexcept { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipStream_t s = nullptr;
};
template <typename T>
struct Pinned : NoCopy {     // host memory of hipHostMalloc, flags as the site needs them
    ~Pinned() noexcept { if (ptr) (void)hipHostFree(ptr); }
    hipError_t alloc(size_t bytes, unsigned flags) noexcept { return hipHostMalloc((void **)&ptr, bytes, flags); }
    T *ptr = nullptr;
};
}  // namespace gsh

// a device array that grows and never shrinks (gsh::dev_reserve; hipFree synchronises the device)
struct DevArray : gsh::NoCopy {
    ~DevArray() noexcept { if (ptr) (void)hipFree(ptr); }
    void *release() noexcept { void *p = ptr; ptr = nullptr; bytes = 0; return p; }
    void *ptr = nullptr;
    size_t bytes = 0;
};

// ---- the objects behind the handles: every member has an initialiser, every resource an owner (or, for the references
// to ref-counted buffers, the destructor), so gs_*_destroy is: null check, hipSetDevice, what it waits for, delete ----

struct gs_device {
    int ordinal = 0;
    gs_limits limits{};
    gsh::Stream internal;  // for blocking helper work
    // probe result: returning LDS atomics hand out lane-ordered values.  Written by any renderer of the device whose rank
    // watchdog fired (gs_render_frame / gs_renderer_wait_frame, possibly from different host threads) and read once per
    // frame (SortCtx::fast_rank) and by the stand-alone sorts: atomic, relaxed — it only ever goes from true to false.
    std::atomic<bool> lds_atomic_ordered{false};
    // renderers of this device: gs_stream_destroy records the end-of-frame event of those whose last frame sits on the
    // stream that is going away (the event is otherwise recorded lazily, when the renderer moves to another stream)
    std::mutex renderers_mu;
    std::vector<struct gs_renderer *> renderers;
    // gs_image_compare: the partial rows and the device result of the last call; the call holds the mutex
    std::mutex metrics_mu;
    DevArray metrics_scratch;
};

struct gs_stream {
    gs_stream(gs_device *d, hipStream_t st, bool owned) : dev(d), s(st) { if (owned) own.s = st; }
    gs_device *dev = nullptr;
    hipStream_t s = nullptr;
    gsh::Stream own;       // `s` again when the handle made it (gs_stream_create*), empty around a wrapped stream
};

// (ref-counted: gs_buffer_release frees the memory of an owned one with the last reference)
struct gs_buffer {
    gs_device *dev = nullptr;
    void *ptr = nullptr;
    size_t bytes = 0;
    bool owned = false;
    std::atomic<int> refs{1};
};

namespace gsh {

// ---- gs_core.hip ----
// every GS3D_* switch that is read once per process
const gsp::Switches &switches();
gs_status use_device(const gs_device *dev);
gs_status dev_reserve(DevArray &a, size_t bytes);
// ids of buffers and generations of selections: unique in the process, never 0
uint64_t next_object_id();
// a gs_buffer of one reference over `ptr`: owned (released with hipFree) or borrowed
gs_buffer *make_buffer(gs_device *dev, void *ptr, size_t bytes, bool owned);
// `bytes` of device memory into host memory on `st`, awaited; the caller words the failure
hipError_t fetch(hipStream_t st, void *dst, const void *src, size_t bytes);

}  // namespace gsh

// ------------------------------------------------------------------------------------------------
// GaussiansBuffer<G>
// ------------------------------------------------------------------------------------------------

struct gs_gaussians_buffer : gsh::NoCopy {
    ~gs_gaussians_buffer() {
        if (order) gs_buffer_release(order);
        if (buf) gs_buffer_release(buf);
    }
    gs_buffer *buf = nullptr;             // a reference
    int sh = 0, cov = 0;
    // block-planar mirror read by the preprocess kernel; rebuilt lazily
    gsh::DevMem planar;
    size_t planar_stride = 0;  // capacity in Gaussians = len rounded up to whole 1024-blocks
    // Gaussians [dirty_lo, dirty_hi) of the AoS buffer are newer than the mirror (empty when lo >= hi).
    // update_range dirties only its own range, so an editor's per-edit update re-mirrors a few
    // Gaussians instead of the whole scene.
    size_t dirty_lo = 0, dirty_hi = (size_t)-1;      // a new buffer is dirty all over
    // spatial mirror order: order[slot] = Gaussian index, inv[index] = slot; both
    // null while the mirror is in index order.  `order` is a ref-counted gs_buffer so that the
    // renderer's parity taps can keep the order of the frame they describe.
    bool spatial = true;
    gs_buffer *order = nullptr;           // a reference
    gsh::DevMem inv;
    gsh::DevMem block_bounds;     // 8 floats per 1024-slot block (k_block_bounds); null = not available
    size_t partial_since_order = 0;   // Gaussians rewritten by partial updates since the order was built
    // The mirror is (re)built on the stream of whichever frame first needs it; frames on OTHER streams
    // (several renderers keeping frames in flight on one buffer) wait for this event before reading it.
    gsh::Event mirror_ready;
    hipStream_t mirror_stream = nullptr;
    // gs_gaussians_buffer_edit only ENQUEUES its kernel: a mirror rebuild on another stream waits for
    // this event before it reads the AoS records (gsh::wait_for_edits / record_edit).  keep_order: the whole buffer is
    // dirty but no position changed (a colour / opacity edit), so the rebuild repacks through the order it has instead
    // of sorting again.
    gsh::Event edit_done;
    hipStream_t edit_stream = nullptr;
    bool keep_order = false;
    // what a renderer's slot-ordered selection masks were gathered through: this buffer (ids are never
    // reused, addresses are) and this build of its mirror order
    uint64_t uid = gsh::next_object_id();
    uint64_t order_epoch = 0;
    // gs_gaussians_buffer_create_concat: the per-block offsets its copies read; they are only enqueued
    // when the call returns, so the new buffer owns the array
    gsh::DevMem concat_offsets;
    // gs_gaussians_buffer_stats / _histogram: the partial rows and the device result of the last call
    DevArray stats_scratch;
    // gs_gaussians_buffer_neighbor_counts / gs_select_neighbors and the component calls (§3.16): keys,
    // order, sorted positions, the union-find words and the sort's histograms of the last call; a call on another stream
    // waits for nb_done before it reuses them
    DevArray nb_scratch, nb_ghist, nb_digit_totals;
    gsh::Event nb_done;
    hipStream_t nb_stream = nullptr;
    void mark(size_t lo, size_t hi) {
        if (lo >= hi) return;
        partial_since_order += hi - lo;
        if (dirty_lo >= dirty_hi) { dirty_lo = lo; dirty_hi = hi; return; }
        if (lo < dirty_lo) dirty_lo = lo;
        if (hi > dirty_hi) dirty_hi = hi;
    }
    void mark_all() { dirty_lo = 0; dirty_hi = (size_t)-1; keep_order = false; }
};

// Gaussian selection: n bits in caller index order.  `generation` changes with every call that may
// modify the bits (next_object_id: unique across selections), which is how a renderer knows its slot-ordered copy is stale.
struct gs_selection {
    gs_device *dev = nullptr;
    size_t n = 0, nwords = 0;
    gsh::DevMem words;          // nwords of 32 bits (at least one word is allocated)
    DevArray scratch;           // a plane of the same size for the select ops that scatter their bits (select_visible)
    DevArray counter;           // gs_selection_count's device total
    uint64_t generation = 0;
    uint32_t *bits() const { return (uint32_t *)words.ptr; }
    uint32_t tail_mask() const { return (n & 31u) ? (1u << (n & 31u)) - 1u : 0xffffffffu; }
    uint32_t grid() const { return nwords < 256u * 1024u ? (uint32_t)((nwords + 255u) / 256u) + 1u : 1024u; }
};

namespace gsh {

inline bool valid_cfg(int sh, int cov) { return sh >= 0 && sh <= 3 && cov >= 0 && cov <= 2; }
inline hipStream_t stream_of(gs_device *dev, gs_stream *s) { return s ? s->s : dev->internal.s; }
inline size_t pod_stride(const gs_gaussians_buffer *g) { return (size_t)gs::pod_bytes(g->sh, g->cov); }
inline bool all_finite(const float *v, int n) {
    for (int k = 0; k < n; k++)
        if (!std::isfinite(v[k])) return false;
    return true;
}
// the kernels index Gaussians with 32 bits
inline gs_status check_len32(size_t len) {
    if (len > 0xfffffff0ull) return gs_fail(GS_ERR_INVALID_ARGUMENT, len, 0, 0, "too many Gaussians");
    return GS_OK;
}

// ---- gs_core.hip ----
// `st` waits for the edit, restore or concatenation that another stream still has in flight on the records of `g`
gs_status wait_for_edits(const gs_gaussians_buffer *g, hipStream_t st);
// ... and `st` has just been given such work: whoever reads or writes the records on another stream waits for it
gs_status record_edit(gs_gaussians_buffer *g, hipStream_t st);
// What a call that reads the records of `g` under a selection (NULL: all; invert: the unselected) starts with.
// records_check: the selection fits the buffer and the kernels can index it -> len, n, nblocks, words, inv, dev; touches
// no device.  records_access: ... then dev is current, st is the stream of the call and waits for edits in flight.
// An entry point with checks of its own between the two halves calls records_check and goes on by hand.
struct RecordsAccess {
    gs_device *dev = nullptr;
    hipStream_t st = nullptr;
    size_t len = 0;
    uint32_t n = 0, nblocks = 0;      // nblocks: whole and partial 1024-blocks
    const uint32_t *words = nullptr;
    uint32_t inv = 0;
};
gs_status records_check(const gs_gaussians_buffer *g, const gs_stream *s, const gs_selection *sel, int32_t invert, RecordsAccess &a);
gs_status records_access(const gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert, RecordsAccess &a);

// ---- gs3d.hip ----
// gs_device_create: do returning LDS atomics hand out lane-ordered values (the fast radix rank)?  Blocks on `st`.
bool probe_lds_atomic_order(hipStream_t st);
// gs_stream_destroy: the end-of-frame event of every renderer whose last frame is on `st` is recorded now
void renderers_leave_stream(gs_device *dev, hipStream_t st);
// stable radix sort of (key, u32 value) pairs with a host-known count; instantiated for uint32_t and uint64_t keys
template <typename K>
gs_status sort_pairs_device(const gs_device *dev, void *const keys[2], void *const vals[2], DevArray &ghist, DevArray &digit_totals,
                            uint32_t count, uint32_t end_bit, hipStream_t st, int &result_side, uint32_t &passes_out);
// k_scan_chunks, one workgroup of 1024: out = exclusive scan of in[0, n) (in place allowed), *total = the sum
void scan_chunks_enqueue(hipStream_t st, const uint32_t *in, uint32_t *out, uint32_t *total, uint32_t n);
// k_bbox_final, one workgroup of 256: `count` partial boxes of 6 floats -> bbox
void bbox_final_enqueue(hipStream_t st, const float *partial, uint32_t count, float *bbox);

// ---- gs_select.hip ----
gs_status check_selection(const gs_selection *sel, const gs_stream *s);
gs_status check_select_op(gs_select_op op);
// the contribution records of gs_render_frame_contrib / gs_select_contribution: n x 16 bytes, aligned, on `dev`
gs_status check_contrib_buffer(const gs_buffer *contrib, const gs_device *dev, size_t n);
// the selection argument of an edit / extraction / statistic: NULL (all), or n bits on the buffer's device
gs_status check_buffer_selection(const gs_gaussians_buffer *g, const gs_stream *s, const gs_selection *sel);
// dst = dst op src over whole words on `st` (src: another selection's words, or dst's scratch plane)
gs_status selection_combine_words(gs_selection *dst, hipStream_t st, gs_select_op op, const uint32_t *src);
// k_sel_range: sel = sel op {i : start <= i < end} on `st`; sel->nwords > 0
void sel_range_enqueue(gs_selection *sel, hipStream_t st, uint32_t start, uint32_t end, gs_select_op op);

// ---- gs_edit.hip ----
// a buffer of `len` > 0 records for a copy that writes every byte of it: allocated without the zero fill of gs_buffer_create
gs_status gaussians_buffer_create_unfilled(gs_device *dev, int sh, int cov, size_t len, gs_gaussians_buffer **out);
// the prelude of every extraction, on `st`: per-1024-block counts of the mask, scanned in place, summed into *total_dev
void extract_scan_enqueue(hipStream_t st, const uint32_t *words, uint32_t n, uint32_t invert, uint32_t *offsets, uint32_t *total_dev);
// ... and its total on the host: blocks on `st`
gs_status extract_scan(hipStream_t st, const uint32_t *words, uint32_t n, uint32_t invert, uint32_t *offsets, uint32_t *total_dev,
                       uint32_t *total);
// k_extract_copy: the `total` records the scan counted, src (n records of nc 16-byte chunks) -> dst, packed in index order
void extract_copy_enqueue(hipStream_t st, const void *src, void *dst, const uint32_t *words, uint32_t n, uint32_t invert,
                          const uint32_t *offsets, uint32_t nc, uint32_t total);
// what extraction, conversion and the exports start with: records_access, the scan into an array of the call, its total on
// the host (n == 0: no array, total 0).  Blocks on x.st.
struct ExtractScan : RecordsAccess {
    DevArray scan;            // the per-1024-block offsets, then the total
    uint32_t total = 0;
    const uint32_t *offsets() const { return (const uint32_t *)scan.ptr; }
};
gs_status extract_begin(const gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert, ExtractScan &x);

// ---- gs_relayout.hip ----
// The body of gs_gaussians_buffer_create_from_selection ((dsh, dcov) = the layout of src) and _create_converted: the
// selected records as a new buffer of layout (dsh, dcov).  Blocks.  A copy that fails leaves the HIP error in *copy_error
// and returns GS_ERR_HIP without a message: the entry point words it.
gs_status extract_records(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel, int32_t invert, int dsh, int dcov,
                          gs_gaussians_buffer **out, uint64_t *count_out, hipError_t *copy_error);
// gs_gaussians_buffer_create_concat (as_layout false: the sources share one layout, which the result takes) and
// gs_gaussians_buffer_create_concat_as (as_layout true: every source is converted to (dsh, dcov))
gs_status concat_records(gs_stream *s, gs_gaussians_buffer *const *srcs, const gs_selection *const *sels, uint32_t count, bool as_layout,
                         int dsh, int dcov, gs_gaussians_buffer **out, uint64_t *counts_out);

// ---- gs_neighbors.hip ----
gs_status check_neighbor_radius(float radius);
// What the calls on the neighbour graph share: the cell keys of the points sorted (keys[s], NB_KEY_NONE
// behind the points), vals[s] = the caller index in sorted slot s, the transformed positions gathered into that order, the
// caller-order plane of the buffer's scratch and `extra_bytes` more behind it (256-byte aligned), all in g->nb_scratch.
struct NeighborGrid {
    const uint64_t *keys = nullptr;
    const uint32_t *vals = nullptr;
    const float *sx = nullptr, *sy = nullptr, *sz = nullptr;
    const float *bbox = nullptr;      // lo xyz, hi xyz of the points (k_bbox_final): what nb_grid makes the cells from
    uint32_t *plane = nullptr;
    void *extra = nullptr;
    uint32_t n = 0, nblocks = 0;      // nblocks: of 256 slots
};
gs_status neighbor_grid_enqueue(gs_gaussians_buffer *g, hipStream_t st, const gs_selection *among, const gs_model_transform_pod *mt,
                                float radius, size_t extra_bytes, NeighborGrid &grid);
// ... and behind the last kernel of the call, on every path: the next call on another stream waits until this one has left
// the scratch
gs_status neighbor_scratch_release(gs_gaussians_buffer *g, hipStream_t st);

// ---- gs_deflate.hip ----
// gs_buffer_gzip_fast without its checks: the gzip member of the `len` device bytes at `bytes` (any
// alignment, on the current device) into the host memory `out`; out == NULL: only *bytes_out.  Blocks on `st`.
gs_status gzip_fast_device(hipStream_t st, const uint8_t *bytes, size_t len, void *out, size_t capacity, size_t *bytes_out);

}  // namespace gsh
