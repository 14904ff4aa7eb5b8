// gs3d.hip — the render side of libgs3d_hip.so: camera, renderer, sorts, the spatial order of a buffer's mirror, the
// stages of a frame, the parity taps, and the stand-alone sort / scan.  Kernels: gs_render_kernels.h.  The rest of the C
// ABI of include/gs3d.h is in gs_core / gs_bundle / gs_select / gs_edit / gs_stats / gs_neighbors.hip.
// Built by hipcc --offload-arch=gfx950 -ffp-contract=off (see build.py).  No CPU fallback: every
// compute entry point needs a HIP device.
#include "gs_host.h"

#include <dlfcn.h>

#include <string>

#include "gs_render_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// renderer
// ------------------------------------------------------------------------------------------------

extern "C" void gs_camera_look_at(const float eye[3], const float target[3], const float up[3],
                                  float vfov, uint32_t width, uint32_t height, float near_plane,
                                  float far_plane, gs_camera *out) {
    // glam Mat4::look_at_rh; evaluated in double and rounded once
    double f[3], s[3], u[3], fl = 0, sl = 0;
    for (int i = 0; i < 3; i++) {
        f[i] = (double)target[i] - (double)eye[i];
        fl += f[i] * f[i];
    }
    fl = std::sqrt(fl);
    for (int i = 0; i < 3; i++) f[i] /= fl;
    s[0] = f[1] * up[2] - f[2] * up[1];
    s[1] = f[2] * up[0] - f[0] * up[2];
    s[2] = f[0] * up[1] - f[1] * up[0];
    for (int i = 0; i < 3; i++) sl += s[i] * s[i];
    sl = std::sqrt(sl);
    for (int i = 0; i < 3; i++) s[i] /= sl;
    u[0] = s[1] * f[2] - s[2] * f[1];
    u[1] = s[2] * f[0] - s[0] * f[2];
    u[2] = s[0] * f[1] - s[1] * f[0];
    double e[3] = {eye[0], eye[1], eye[2]};
    double ds = s[0] * e[0] + s[1] * e[1] + s[2] * e[2];
    double du = u[0] * e[0] + u[1] * e[1] + u[2] * e[2];
    double df = f[0] * e[0] + f[1] * e[1] + f[2] * e[2];
    float *v = out->view;
    v[0] = (float)s[0]; v[1] = (float)u[0]; v[2] = (float)-f[0]; v[3] = 0.0f;
    v[4] = (float)s[1]; v[5] = (float)u[1]; v[6] = (float)-f[1]; v[7] = 0.0f;
    v[8] = (float)s[2]; v[9] = (float)u[2]; v[10] = (float)-f[2]; v[11] = 0.0f;
    v[12] = (float)-ds; v[13] = (float)-du; v[14] = (float)df; v[15] = 1.0f;
    std::memcpy(out->pos, eye, 12);
    double focal = 0.5 * (double)height / std::tan(0.5 * (double)vfov);
    out->fx = (float)focal;
    out->fy = (float)focal;
    out->cx = 0.5f * (float)width;
    out->cy = 0.5f * (float)height;
    out->near_plane = near_plane;
    out->far_plane = far_plane;
    out->width = width;
    out->height = height;
    out->background[0] = out->background[1] = out->background[2] = 0.0f;
}

// stage indices of gs_frame_stats.stage_ms
enum { ST_REPACK = 0, ST_PRE, ST_SCAN, ST_DSORT, ST_EXPAND, ST_TSORT, ST_RANGES, ST_BLEND, ST_FRAME, ST_COUNT };

// what sized the scratch of the last frame: a change means the pair count may jump, so the next
// frame measures it first (one blocking "sizing" frame) instead of trusting the history
struct FrameShape {
    uint64_t n = 0;
    uint32_t width = 0, height = 0, band0 = 0, band1 = 0;
    bool operator==(const FrameShape &o) const {
        return n == o.n && width == o.width && height == o.height && band0 == o.band0 && band1 == o.band1;
    }
};

struct gs_renderer : NoCopy {
    ~gs_renderer() { if (last_order) gs_buffer_release(last_order); }
    gs_device *dev = nullptr;
    DevArray order_r2, keep_bits, r2_scan, box_table;         // two-round frames: mirror slots of the Gaussians round 2 keeps, in depth order; one bit per slot
    DevArray recs, depth, rect, sorted_rect, exp_sums, cursors, chunk_tiles, chunk_vis, state, zero_region, scan_tmp, block_list;
    DevArray cull_status;                 // k_block_cull: one (tag << 10 | count) word per group of 256 blocks
    DevArray chunk_hist;                  // [chunks][256] first-digit histogram of every chunk's depth keys (PreOut::chunk_hist)
    bool list_mode = false;               // the last frame's per-slot arrays are in LIST space (k_block_cull ran)
    bool rank_inject_set = false;         // GS3D_TEST_RANK_FAULT: the watchdog's test hook has been armed
    gsp::SortFeedback sort_fb;            // which depth / tile sort, and what the choice rests on (gs_policy.h)
    gsp::RoundsFeedback rounds_fb;        // one round or two, the length of round 1, partitioned or not (gs_policy.h)
    bool tile_msd = false;                // the tile sort of the last frame was MSD-first
    int depth_msd_req = -1, tile_msd_req = -1;   // gs_renderer_set_sort_mode: -1 = the renderer chooses
    int tile_masks_req = -1;              // gs_renderer_set_tile_masks
    bool tile_masks = false;              // the last frame ran tile rect version 4
    bool two_round = false;               // the last frame took two rounds (its taps hold round 2 only)
    bool partitioned = false;             // ... and sorted each round on its own (gs_sort_info)
    int rounds_req = -1;                  // gs_renderer_set_rounds: -1 the renderer decides, 0 one round, 1 two
    uint32_t round1_req = 0;              // ... Gaussians of round 1 (0: a quarter of the visible ones)
    uint32_t round1 = 0;                  // Gaussians the last two-round frame's first round covered
    uint32_t frame_capacity = 0;          // the pair bound the last frame's rounds were planned with (FramePlan::capacity)
    uint8_t done_rounds[2] = {1, 1};      // the rounds of the frames behind the two result blocks, and their round-1 lengths
    uint32_t done_round_k[2] = {0, 0};
    bool wt_pairs = true;                 // k_pairs_emit stores write-through (gs::store16)
    bool state_tile_bmax_dirty = false;   // FrameState::tile_bucket_max holds a value of an MSD-first frame
    uint32_t cull_last_gen = 0, cull_last_groups = 0;   // frame / group count of the last k_block_cull (status tags)
    DevArray dkeys[2], dvals[2];          // (depth bits - bias, mirror slot), capacity N
    DevArray tkeys[2], tvals[2];          // (tile id, mirror slot), capacity pair_capacity
    DevArray ghist, digit_totals, bucket_starts;
    Pinned<gs::FrameResult> results;      // [2]: one per frame parity
    Pinned<uint32_t> host_counters;       // sizing pass total
    uint64_t pair_capacity = 0;
    FrameShape shape;
    uint32_t gen = 0;                     // frame generation (tags the pinned results)
    Event done[2];                        // end of the frame of each parity
    bool done_valid[2] = {false, false};
    uint32_t done_gen[2] = {0, 0};
    uint32_t done_shape[2] = {0, 0};      // shape_epoch of the frame behind each done event
    uint32_t shape_epoch = 0;             // counts the changes of `shape` (a new epoch starts with a sizing frame)
    // last frame (host-side knowledge; V and D live in results[gen & 1])
    uint64_t n = 0;
    uint32_t tiles_x = 0, tiles_y = 0, sort_passes = 0;
    uint32_t key_bias = 0;
    int dsorted_side = 0, tsorted_side = 0;
    bool wide_tiles = false;  // tile keys are u32 (more than 65536 tiles) instead of u16
    bool rect32 = false;      // the last frame's tile rects are packed (gs::rect_pack32)
    uint32_t launches = 0;                // kernel launches of the last frame (diagnostic)
    uint32_t *flags_target = nullptr;     // device word that receives every frame's flags (gs_renderer_set_frame_flags_target)
    // selection frames: the hide / tint masks in mirror-slot order, the per-block "fully hidden" flags,
    // and what each copy was gathered from (SlotMaskKey; generation 0 = nothing cached)
    struct SlotMaskKey {
        uint64_t generation = 0, buffer = 0, order_epoch = 0, n = 0;
        bool operator==(const SlotMaskKey &o) const {
            return generation == o.generation && buffer == o.buffer && order_epoch == o.order_epoch && n == o.n;
        }
    };
    DevArray sel_slots[2], sel_block_hidden;      // [0] hide, [1] tint
    SlotMaskKey sel_key[2];
    uint32_t width = 0, height = 0;       // image size of the last frame (gs_renderer_select_visible)
    hipStream_t last_stream = nullptr;
    bool have_frame = false;              // last_stream is meaningful (the null stream is a valid stream)
    bool last_stream_gone = false;        // ... but has been destroyed since (gs_stream_destroy recorded done[gen & 1] on it)
    gs_buffer *last_order = nullptr;      // a reference: mirror order of the last frame's buffer (null = index order), for the taps
    // timing
    bool timing = false;
    Event ev[ST_COUNT + 2];               // flags 0; made by the first gs_renderer_set_timing(1)
    bool ev_valid = false;                // ... all of them
    bool ev_pending = false;
    double stage_ms[ST_COUNT] = {};
    uint32_t timed_frames = 0;
};

// gs_stream_destroy: the end-of-frame event of every renderer whose last frame is on `st` is recorded now, and the
// renderer remembers that the stream is gone (it must not be touched again: waits go through the event).
void gsh::renderers_leave_stream(gs_device *dev, hipStream_t st) {
    std::lock_guard<std::mutex> lock(dev->renderers_mu);
    for (gs_renderer *r : dev->renderers) {
        if (!r->have_frame || r->last_stream_gone || r->last_stream != st) continue;
        r->done_valid[r->gen & 1u] = hipEventRecord(r->done[r->gen & 1u], st) == hipSuccess;
        r->last_stream_gone = true;
    }
    (void)hipGetLastError();
}

// gs_device_create: both digit widths of the sorts (256 and 512 counters per wave), the scatter's own access pattern
bool gsh::probe_lds_atomic_order(hipStream_t st) {
    bool ordered = false;
    {
        DevMem mem;
        uint32_t h = 1;
        if (mem.alloc_raw(4) == hipSuccess && hipMemset(mem.ptr, 0, 4) == hipSuccess) {
            uint32_t *bad = (uint32_t *)mem.ptr;
            hipLaunchKernelGGL(gs::k_probe_lds_atomic_order<8>, dim3(512), dim3(gs::SORT_THREADS), 0, st, 8u, 0x3D650001u, bad);
            hipLaunchKernelGGL(gs::k_probe_lds_atomic_order<9>, dim3(512), dim3(gs::SORT_THREADS), 0, st, 8u, 0x3D650002u, bad);
            if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(&h, bad, 4, hipMemcpyDeviceToHost) == hipSuccess) ordered = (h == 0);
        }
    }      // (the word is freed before the sticky error of a failed step is dropped, as before)
    (void)hipGetLastError();
    return ordered;
}

// host wait for the renderer's last frame: its stream, or — the stream was destroyed — its end-of-frame event
static hipError_t sync_last_frame(gs_renderer *r) {
    if (!r->have_frame) return hipSuccess;
    if (!r->last_stream_gone) return hipStreamSynchronize(r->last_stream);
    return r->done_valid[r->gen & 1u] ? hipEventSynchronize(r->done[r->gen & 1u]) : hipSuccess;
}

extern "C" gs_status gs_renderer_create(gs_device *dev, gs_renderer **out) {
    if (!out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null out");
    GS_TRY(use_device(dev));
    std::unique_ptr<gs_renderer> r(new gs_renderer());
    r->dev = dev;
    hipError_t e = r->host_counters.alloc(64, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = r->results.alloc(2 * sizeof(gs::FrameResult), hipHostMallocMapped | hipHostMallocCoherent);
    // no system-scope fence at the event: what the host reads after it (the frame result) lives in
    // coherent pinned memory, and images are fetched with copies that synchronise by themselves
    // (GS3D_EVENT_FENCE=1 asks for the fence)
    for (int i = 0; i < 2 && e == hipSuccess; i++)
        e = r->done[i].create(hipEventDisableTiming | (switches().event_fence ? 0u : hipEventDisableSystemFence));
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "renderer allocation failed: %s", hipGetErrorString(e));
    std::memset(r->results.ptr, 0, 2 * sizeof(gs::FrameResult));
    {
        std::lock_guard<std::mutex> lock(dev->renderers_mu);
        dev->renderers.push_back(r.get());
    }
    *out = r.release();
    return GS_OK;
}

extern "C" void gs_renderer_destroy(gs_renderer *r) {
    if (!r) return;
    (void)hipSetDevice(r->dev->ordinal);
    {
        std::lock_guard<std::mutex> lock(r->dev->renderers_mu);
        auto &v = r->dev->renderers;
        for (size_t i = 0; i < v.size(); i++)
            if (v[i] == r) {
                v[i] = v.back();
                v.pop_back();
                break;
            }
    }
    (void)sync_last_frame(r);   // kernels of the last frame write pinned memory
    delete r;
}

extern "C" gs_status gs_renderer_set_timing(gs_renderer *r, int32_t enabled) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    GS_TRY(use_device(r->dev));
    if (enabled && !r->ev_valid) {
        // (a call that failed half way left its events with their owners: this one makes the rest)
        for (auto &e : r->ev)
            if (!e) GS_HIP_AS("hipEventCreate(&e)", e.create(0));
        r->ev_valid = true;
    }
    r->timing = enabled != 0;
    return GS_OK;
}

extern "C" gs_status gs_renderer_set_frame_flags_target(gs_renderer *r, uint32_t *device_word) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    if ((uintptr_t)device_word & 3u) return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(uintptr_t)device_word, 4, 0, "unaligned flags word");
    r->flags_target = device_word;
    return GS_OK;
}

// fold the events of the previous timed frame into the accumulators
static gs_status collect_timing(gs_renderer *r) {
    if (!r->ev_pending) return GS_OK;
    GS_HIP(hipEventSynchronize(r->ev[ST_COUNT]));
    for (int i = 0; i < ST_FRAME; i++) {
        float ms = 0;
        GS_HIP(hipEventElapsedTime(&ms, r->ev[i], r->ev[i + 1]));
        r->stage_ms[i] += ms;
    }
    float ms = 0;
    GS_HIP(hipEventElapsedTime(&ms, r->ev[0], r->ev[ST_FRAME]));
    r->stage_ms[ST_FRAME] += ms;
    r->timed_frames++;
    r->ev_pending = false;
    return GS_OK;
}

extern "C" gs_status gs_renderer_reset_stats(gs_renderer *r) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    GS_TRY(use_device(r->dev));
    GS_TRY(collect_timing(r));
    for (int i = 0; i < ST_COUNT; i++) r->stage_ms[i] = 0.0;
    r->timed_frames = 0;
    return GS_OK;
}

// result block of the most recent frame (valid once its stream work has completed)
static const gs::FrameResult &last_result(const gs_renderer *r) { return r->results.ptr[r->gen & 1u]; }

extern "C" gs_status gs_renderer_wait_frame(gs_renderer *r, gs_frame_result *out) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    GS_TRY(use_device(r->dev));
    if (out) std::memset(out, 0, sizeof(*out));
    if (!r->have_frame) return GS_OK;       // no frame yet
    GS_HIP(sync_last_frame(r));
    const gs::FrameResult &fr = last_result(r);
    if (out) {
        out->gaussians = r->n;
        out->visible = fr.visible;
        out->pairs = fr.pairs_total;
        out->pair_capacity = r->pair_capacity;
        out->flags = fr.flags;
        out->launches = r->launches;
    }
    if (fr.gen != r->gen)
        return gs_fail(GS_ERR_HIP, fr.gen, r->gen, 0, "the frame did not complete (result generation %u, expected %u)",
                    fr.gen, r->gen);
    if (fr.pairs_total > 0xfffffff0ull)
        return gs_fail(GS_ERR_PAIR_OVERFLOW, r->n, 0, 0,
                    "the frame needs more than 2^32 (tile, Gaussian) pairs; pair indices are 32-bit");
    if (fr.flags & gs::FRAME_FLAG_RANK_FAULT) {
        // The device drops to the ballot-based rank, and THIS renderer's watchdog word is cleared whether or not it was
        // this renderer that flipped the switch: with several renderers on one device (FrameRing, parallel.lanes) the
        // second one to report used to find the switch already off, keep its word set, and flag every later frame.
        r->dev->lds_atomic_ordered.store(false);
        (void)hipMemset(&((gs::FrameState *)r->state.ptr)->rank_fault, 0, sizeof(uint32_t));   // the stream is idle here
        return gs_fail(GS_ERR_RANK_ORDER, 0, 0, 0,
                    "the LDS-atomic rank of the radix sort returned an out-of-order value in this frame: its blend order "
                    "may be wrong; the device has been switched to the ballot-based rank: render again");
    }
    if (fr.flags & gs::FRAME_FLAG_PAIR_OVERFLOW) {
        if (r->two_round) {
            // each round of a two-round frame is bounded on its own (gsp::plan_round_capacity): the round that outgrew the
            // bound, its true count and the bound — not the frame's total against the buffers, which may well hold it
            const uint64_t bound = r->frame_capacity, d1 = fr.pairs_round1;
            const uint64_t d2 = fr.pairs_total > d1 ? fr.pairs_total - d1 : 0;
            if (d1 > bound)
                return gs_fail(GS_ERR_PAIR_CAPACITY, d1, bound, 0,
                            "round 1 of the two-round frame produced %llu (tile, Gaussian) pairs, a round's bound was %llu: the "
                            "frame was skipped (the image was not written); render again (the next frame has a larger bound)",
                            (unsigned long long)d1, (unsigned long long)bound);
            return gs_fail(GS_ERR_PAIR_CAPACITY, d2, bound, 0,
                        "round 2 of the two-round frame produced %llu (tile, Gaussian) pairs, a round's bound was %llu: the "
                        "frame was skipped (its band holds round 1's pixel state, not a frame); render again (the next frame "
                        "has a larger bound)",
                        (unsigned long long)d2, (unsigned long long)bound);
        }
        return gs_fail(GS_ERR_PAIR_CAPACITY, fr.pairs_total, r->pair_capacity, 0,
                    "the frame produced %llu (tile, Gaussian) pairs but the pair buffers hold %llu: the frame was "
                    "skipped (the image was not written); render again (the next frame grows the buffers)",
                    (unsigned long long)fr.pairs_total, (unsigned long long)r->pair_capacity);
    }
    return GS_OK;
}

extern "C" gs_status gs_renderer_stats(gs_renderer *r, gs_frame_stats *out) {
    if (!r || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(use_device(r->dev));
    GS_HIP(sync_last_frame(r));
    GS_TRY(collect_timing(r));
    std::memset(out, 0, sizeof(*out));
    const gs::FrameResult &fr = last_result(r);
    out->gaussians = r->n;
    out->visible = r->have_frame ? fr.visible : 0;
    out->pairs = r->have_frame ? fr.pairs_total : 0;
    out->tiles_x = r->tiles_x;
    out->tiles_y = r->tiles_y;
    out->sort_passes = r->sort_passes;
    out->timed_frames = r->timed_frames;
    static_assert(ST_COUNT <= 12, "gs_frame_stats.stage_ms too small");
    for (int i = 0; i < ST_COUNT; i++) out->stage_ms[i] = r->stage_ms[i];
    return GS_OK;
}

extern "C" gs_status gs_renderer_sort_info(gs_renderer *r, gs_sort_info *out) {
    if (!r || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(use_device(r->dev));
    std::memset(out, 0, sizeof(*out));
    out->bucket_capacity = gs::BKT_CAP;
    if (!r->have_frame) return GS_OK;
    GS_HIP(sync_last_frame(r));
    const gs::FrameResult &fr = last_result(r);
    out->depth_msd = r->sort_fb.depth_msd ? 1u : 0u;
    out->depth_bucket_max = fr.gen == r->gen ? fr.depth_bucket_max : 0u;
    out->tile_msd = r->tile_msd ? 1u : 0u;
    out->tile_masks = r->tile_masks ? 1u : 0u;
    out->rounds = r->two_round ? 2u : 1u;
    out->round1 = r->two_round ? r->round1 : 0u;
    out->tiles_done = r->two_round && fr.gen == r->gen ? fr.tiles_done : 0u;
    out->partitioned = r->two_round && r->partitioned ? 1u : 0u;
    if (r->tile_msd && r->state.ptr)      // (the result block carries the PREVIOUS frame's: read this frame's from the device)
        GS_HIP(hipMemcpy(&out->tile_bucket_max, &((gs::FrameState *)r->state.ptr)->tile_bucket_max, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return GS_OK;
}

extern "C" gs_status gs_renderer_set_tile_masks(gs_renderer *r, int32_t mode) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    if (mode < -1 || mode > 1) return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(int64_t)mode, 0, 0, "tile mask modes are -1, 0 or 1");
    r->tile_masks_req = mode;
    return GS_OK;
}

extern "C" gs_status gs_renderer_set_rounds(gs_renderer *r, int32_t mode, uint32_t first_round) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    if (mode < -1 || mode > 1) return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(int64_t)mode, 0, 0, "round modes are -1, 0 or 1");
    r->rounds_req = mode;
    r->round1_req = first_round;
    return GS_OK;
}

extern "C" gs_status gs_renderer_set_sort_mode(gs_renderer *r, int32_t depth_msd, int32_t tile_msd) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    if (depth_msd < -1 || depth_msd > 1 || tile_msd < -1 || tile_msd > 1)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(int64_t)depth_msd, (uint64_t)(int64_t)tile_msd, 0, "sort modes are -1, 0 or 1");
    r->depth_msd_req = depth_msd;
    r->tile_msd_req = tile_msd;
    return GS_OK;
}

typedef void (*preprocess_fn)(const uint4 *, uint32_t, gs::FrameConsts, gs::PreOut);
typedef void (*block_bounds_fn)(const uint4 *, uint32_t, float *);
#define GS_CFG_TABLE_X(kernel, ...)                                                                              \
    {                                                                                                             \
        {kernel<0, 0, __VA_ARGS__>, kernel<0, 1, __VA_ARGS__>, kernel<0, 2, __VA_ARGS__>},                        \
        {kernel<1, 0, __VA_ARGS__>, kernel<1, 1, __VA_ARGS__>, kernel<1, 2, __VA_ARGS__>},                        \
        {kernel<2, 0, __VA_ARGS__>, kernel<2, 1, __VA_ARGS__>, kernel<2, 2, __VA_ARGS__>},                        \
        {kernel<3, 0, __VA_ARGS__>, kernel<3, 1, __VA_ARGS__>, kernel<3, 2, __VA_ARGS__>},                        \
    }
// [non-temporal mirror loads][...]: the cache policy is a template parameter (a run-time flag put a
// branch and a wait behind every load)
static preprocess_fn k_tbl_preprocess[2][4][3] = {GS_CFG_TABLE_X(gs::k_preprocess, false), GS_CFG_TABLE_X(gs::k_preprocess, true)};
// [nt][pipelined]
static preprocess_fn k_tbl_preprocess_banded[2][2][4][3] = {
    {GS_CFG_TABLE_X(gs::k_preprocess_banded, false, false), GS_CFG_TABLE_X(gs::k_preprocess_banded, true, false)},
    {GS_CFG_TABLE_X(gs::k_preprocess_banded, false, true), GS_CFG_TABLE_X(gs::k_preprocess_banded, true, true)}};
static block_bounds_fn k_tbl_block_bounds[4][3] = GS_CFG_TABLE(gs::k_block_bounds);
// the instantiations of selection frames: the same tables with a SelIO behind the PreOut
typedef void (*preprocess_sel_fn)(const uint4 *, uint32_t, gs::FrameConsts, gs::PreOut, gs::SelIO);
static preprocess_sel_fn k_tbl_preprocess_sel[2][4][3] = {GS_CFG_TABLE_X(gs::k_preprocess, false, gs::SelIO),
                                                          GS_CFG_TABLE_X(gs::k_preprocess, true, gs::SelIO)};
static preprocess_sel_fn k_tbl_preprocess_banded_sel[2][2][4][3] = {
    {GS_CFG_TABLE_X(gs::k_preprocess_banded, false, false, gs::SelIO), GS_CFG_TABLE_X(gs::k_preprocess_banded, true, false, gs::SelIO)},
    {GS_CFG_TABLE_X(gs::k_preprocess_banded, false, true, gs::SelIO), GS_CFG_TABLE_X(gs::k_preprocess_banded, true, true, gs::SelIO)}};

// frame constants from the uniforms
static void make_frame_consts(const gs_gaussian_transform_pod *gt, const gs_model_transform_pod *mt,
                              const gs_camera *cam, uint32_t band_ty0, uint32_t band_ty1,
                              gs::FrameConsts &fc) {
    gs::ModelTransform m;
    std::memcpy(&m, mt, sizeof(m));
    gs::model_transform_mat(m, fc.M);
    gs::model_transform_inv_sr_mat(m, fc.ISR);
    float sr[9];
    gs::model_scale_rot_mat(m, sr);
    std::memcpy(fc.V, cam->view, 64);
    for (int r = 0; r < 3; r++) {
        float sg = r == 0 ? 1.0f : -1.0f;
        float w0 = sg * cam->view[0 + r], w1 = sg * cam->view[4 + r], w2 = sg * cam->view[8 + r];
        for (int c = 0; c < 3; c++)
            fc.WS[3 * r + c] = (w0 * sr[3 * c + 0] + w1 * sr[3 * c + 1]) + w2 * sr[3 * c + 2];
    }
    std::memcpy(fc.cam_pos, cam->pos, 12);
    fc.fx = cam->fx;
    fc.fy = cam->fy;
    fc.cx = cam->cx;
    fc.cy = cam->cy;
    fc.near_plane = cam->near_plane;
    fc.far_plane = cam->far_plane;
    uint32_t flags;
    std::memcpy(&flags, gt->flags, 4);
    fc.size2 = gt->size * gt->size;
    fc.limx = 1.3f * ((0.5f * (float)cam->width) / cam->fx);
    fc.limy = 1.3f * ((0.5f * (float)cam->height) / cam->fy);
    fc.max_std_dev = gs::gaussian_transform_max_std_dev(flags);
    std::memcpy(fc.bg, cam->background, 12);
    fc.sh_deg = gs::gaussian_transform_sh_deg(flags);
    fc.no_sh0 = gs::gaussian_transform_no_sh0(flags) ? 1u : 0u;
    fc.width = cam->width;
    fc.height = cam->height;
    fc.tiles_x = (cam->width + 15u) / 16u;
    fc.tiles_y = (cam->height + 15u) / 16u;
    fc.band_ty0 = band_ty0 < fc.tiles_y ? band_ty0 : fc.tiles_y;
    fc.band_ty1 = band_ty1 < fc.tiles_y ? band_ty1 : fc.tiles_y;
    if (fc.band_ty1 < fc.band_ty0) fc.band_ty1 = fc.band_ty0;
    fc.mask_culled_records = 0;
    fc.nt_loads = 0;
    // in display mode Splat the tile rect is clipped to the splat's visible box.
    // GS3D_RECT_V1=1 keeps the unclipped rect of spec version 1 (same images, more pairs) for A/B runs
    // and for the parity tests against the version-1 goldens.
    {
        fc.clip_rect = gt->flags[0] == GS_DISPLAY_SPLAT && !switches().rect_v1 ? 1u : 0u;
        // rect version 4: small rects lose the tiles their splat cannot reach.  GS3D_TILE_MASKS=0: version 3
        // (make_frame_consts only records that the display mode allows it; gs_render_frame decides: gs_renderer_set_tile_masks)
        fc.tile_masks = fc.clip_rect;
    }
    fc.ellipse_pmin = -0.5f * (fc.max_std_dev * fc.max_std_dev);
    {   // packed 4-byte tile rects while both tile counts fit 8 bits (images up to 4096 px); GS3D_RECT32=0: always uint2
        fc.rect32 = !switches().rect32_off && fc.tiles_x <= 256u && fc.tiles_y <= 256u && fc.tiles_x * fc.tiles_y <= 32768u ? 1u : 0u;
        // write-through stores of the 16-byte-per-lane outputs (gs::store16).  GS3D_WT_STORES=0/1
        // GS3D_WT_STORES: bit 0 = the pairs of k_pairs_emit, bit 1 = the image
        const int wt_env = switches().wt_stores;
        fc.wt_stores = (wt_env & 2) ? 1u : 0u;
        fc.wt_pairs = (wt_env & 1) ? 1u : 0u;
        fc.wt_records = (uint32_t)switches().wt_records & 3u;
    }
    // block culling gain (see block_is_culled): size^2 |W R_m S_m|_2^2, the squared SPECTRAL norm of the linear part
    // whatever the caller's view and model matrices are: the largest eigenvalue of A = (WS)^T (WS), in double by the
    // closed form for symmetric 3x3 matrices, never above the trace (= the squared Frobenius norm, the bound of rounds
    // 2-3); 0.1 % head room for the f32 arithmetic.  The Jacobian's norm is taken per block on the device.
    {
        double a[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                for (int k = 0; k < 3; k++) a[i][j] += (double)fc.WS[3 * k + i] * (double)fc.WS[3 * k + j];
        const double tr = a[0][0] + a[1][1] + a[2][2];
        double lmax = tr;
        const double p1 = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double q = tr / 3.0;
        const double p2 = (a[0][0] - q) * (a[0][0] - q) + (a[1][1] - q) * (a[1][1] - q) + (a[2][2] - q) * (a[2][2] - q) + 2.0 * p1;
        const double pp = std::sqrt(p2 / 6.0);
        if (pp == 0.0) {
            lmax = q * (1.0 + 1e-6);          // A = q I (a rotation times a uniform scale: the identity model transform)
        } else if (pp > 0.0 && std::isfinite(pp)) {
            double b[3][3];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) b[i][j] = (a[i][j] - (i == j ? q : 0.0)) / pp;
            double rdet = (b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1]) - b[0][1] * (b[1][0] * b[2][2] - b[1][2] * b[2][0]) +
                           b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0])) / 2.0;
            rdet = rdet < -1.0 ? -1.0 : (rdet > 1.0 ? 1.0 : rdet);
            const double l = q + 2.0 * pp * std::cos(std::acos(rdet) / 3.0);
            if (std::isfinite(l) && l > 0.0 && l <= tr) lmax = l * (1.0 + 1e-6) + 1e-30;
        }
        fc.cull_gain = (float)(1.001 * (double)fc.size2 * lmax);
    }
    if (!(fc.cull_gain > 0.0f) || !(fc.cull_gain < 1e30f)) fc.cull_gain = 0.0f;   // degenerate uniforms: no block culling
}

static uint32_t bit_length(uint32_t v) {
    uint32_t b = 0;
    while (v) {
        b++;
        v >>= 1;
    }
    return b;
}

// depth keys: 9-bit digits when that saves a pass (e.g. 27 significant bits: 3 passes instead of 4);
// otherwise 8-bit digits, whose 256-bin tiles write longer runs and fit more workgroups per CU
static uint32_t depth_radix_bits(uint32_t key_bits) {
    return (key_bits + 8) / 9 < (key_bits + 7) / 8 ? (uint32_t)gs::RADIX_BITS_MAX : (uint32_t)gs::RADIX_BITS;
}

// mask of the FIRST digit of a sort of `key_bits` bits in passes of at most `rb` bits (the balanced widths of
// run_sort_items: 27 bits -> 9 + 9 + 9, 13 -> 7 + 6); the preprocess kernel counts that digit per chunk
static uint32_t first_digit_mask(uint32_t key_bits, uint32_t rb) {
    const uint32_t passes = (key_bits + rb - 1) / rb;
    const uint32_t bits = passes ? (key_bits + passes - 1) / passes : 0u;
    return (1u << bits) - 1u;
}

// What every sort launch of one frame (or of one stand-alone sort) needs.  The rank watchdog's words travel here:
// `rank_fault` = FrameState::rank_fault while the frame sorts with the LDS-atomic rank (null in the stand-alone sorts,
// which are not watched, and once the device has dropped to the ballot-based rank); `watch` = the watchdog's sample of
// this frame (gs::k_sort_scatter: tile = watch mod live tiles, round = (watch / live tiles) mod ITEMS; the frame
// generation, so that every position is visited over a few hundred frames).  `fast_rank` (FAST_RANK of the kernels) is
// read ONCE per frame: every scatter of the frame ranks the same way, whatever another renderer's thread does.
struct SortCtx {
    const gs_device *dev = nullptr;
    hipStream_t st = nullptr;
    DevArray *ghist = nullptr, *digit_totals = nullptr;
    uint32_t *rank_fault = nullptr;
    uint32_t watch = 0;
    bool fast_rank = false;
    uint32_t *launches = nullptr;      // the frame's launch counter (null: not counted)
    void count(uint32_t k) const {
        if (launches) *launches += k;
    }
};

// a sort outside a frame: not watched
static SortCtx standalone_sort_ctx(const gs_device *dev, hipStream_t st, DevArray &ghist, DevArray &digit_totals) {
    SortCtx c;
    c.dev = dev;
    c.st = st;
    c.ghist = &ghist;
    c.digit_totals = &digit_totals;
    c.fast_rank = dev->lds_atomic_ordered.load(std::memory_order_relaxed);
    return c;
}

// The frame's compacting first pass (see gs_render_kernels.h, COMPACT): dense keys in, the index is
// the value, chunks without visible Gaussians are skipped, V comes out in *visible_out.
struct SortCompact {
    const uint32_t *dense_keys = nullptr;   // [N] keys by slot, 0xffffffff = culled (read by pass 0 instead of keys[0])
    const uint32_t *chunk_vis = nullptr;
    uint32_t *visible_out = nullptr;
    uint32_t dense_count = 0;        // N: the first pass runs over all slots (host bound: sizes the grid)
    const uint32_t *dense_count_dev = nullptr;   // optional device word: the slots that really hold data (list frames)
    const uint32_t *chunk_hist = nullptr;        // per-chunk histogram of the first digit, counted by the preprocess kernel
    gs::CompactPred pred;            // which side of a partitioned two-round frame's depth threshold the pass keeps (default: all)
    uint32_t *bucket_max = nullptr;  // receives the largest top-digit bucket (only the LSD sort's LAST pass reports it)
};

// one radix pass (histogram -> row scan -> scatter): what varies from pass to pass.  Keys are typed by the launcher's
// template arguments (KI in, KO out).
struct RadixPass {
    const void *kin = nullptr;
    const uint32_t *vin = nullptr;
    void *kout = nullptr;
    uint32_t ko_shift = 0;
    uint32_t *vout = nullptr;
    gs::SortCount sc{0, nullptr};
    uint32_t shift = 0, digit_mask = 0;
    uint32_t nb = 0, sgrid = 0, xr = 0;          // tiles, padded grid and span of the XCD-aware order (xcd_span_for)
    const uint32_t *chunk_vis = nullptr;         // COMPACT passes
    uint32_t *visible_out = nullptr;
    gs::CompactPred pred;
    const uint32_t *chunk_hist = nullptr;        // ... whose histogram the preprocess kernel counted per chunk
    uint32_t chunk_hist_words = (uint32_t)gs::PP_THREADS;
    uint32_t *bucket_max = nullptr;              // the depth sort's pass on its top digit
    uint32_t *bucket_starts = nullptr;           // the MSD-first sorts' scatter pass writes every bucket's start here
};

template <int TILE>
static void launch_scan_rows(uint32_t rows, hipStream_t st, uint32_t *ghist, uint32_t stride, gs::SortCount sc,
                             uint32_t *totals) {
    // rows of up to SCAN_ROWS_SMALL_MAX blocks (stride = the host's bound of the block count): one wave per row
    if (stride <= gs::SCAN_ROWS_SMALL_MAX && !switches().scan_rows_small_off)
        hipLaunchKernelGGL((gs::k_sort_scan_rows_small<TILE>), dim3((rows + 3u) / 4u), dim3(256), 0, st, ghist, stride, sc,
                           totals, rows);
    else
        hipLaunchKernelGGL((gs::k_sort_scan_rows<TILE>), dim3(rows), dim3(gs::SCAN_ROWS_THREADS), 0, st, ghist, stride, sc,
                           totals);
}

// FAST_RANK of a kernel: chosen by the device probe and the frame's watchdog (SortCtx::fast_rank); fn(tag, rank_fault, watch)
template <class F>
static void with_rank(const SortCtx &c, F fn) {
    if (c.fast_rank) fn(std::true_type(), c.rank_fault, c.rank_fault ? c.watch : 0u);
    else fn(std::false_type(), (uint32_t *)nullptr, 0u);
}

// one scatter launch; KO = type of the keys the pass writes
template <typename KI, typename KO, int RB, bool COMPACT, int ITEMS>
static void launch_scatter(const SortCtx &c, const RadixPass &p) {
    // inputs that cannot stay in the L2s anyway are read non-temporally (top bit of the last argument; see
    // k_sort_scatter).  GS3D_NT_SCATTER=0/1 forces.
    const int nt_env = switches().nt_scatter;
    const bool nt = !COMPACT && (nt_env >= 0 ? nt_env != 0 : (uint64_t)p.sc.count * (sizeof(KI) + 4u) > (32ull << 20));
    const uint32_t xr_nt = p.xr | (nt ? 0x80000000u : 0u);
    const uint32_t *ghist = (const uint32_t *)c.ghist->ptr, *totals = (const uint32_t *)c.digit_totals->ptr;
    // PRED: a partitioned two-round frame's compacting pass (RadixPass::pred)
    auto go = [&](auto pred_tag) {
        with_rank(c, [&](auto fast_tag, uint32_t *rf, uint32_t watch) {
            constexpr bool FAST = decltype(fast_tag)::value, PRED = decltype(pred_tag)::value;
            hipLaunchKernelGGL((gs::k_sort_scatter<KI, FAST, RB, COMPACT, ITEMS, KO, PRED>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st,
                               (const KI *)p.kin, p.vin, (KO *)p.kout, p.ko_shift, p.vout, p.sc, p.shift, p.digit_mask, ghist, totals, p.chunk_vis,
                               p.visible_out, p.nb, xr_nt, rf, watch, p.bucket_max, p.bucket_starts, PRED ? p.pred : gs::CompactPred());
        });
    };
    if constexpr (COMPACT) {
        if (p.pred.tau_dev) {
            go(std::true_type());
            return;
        }
    }
    go(std::false_type());
}

// one radix pass: histogram -> row scan -> scatter
template <typename KI, typename KO, int RB, bool COMPACT, int ITEMS>
static void launch_pass(const SortCtx &c, const RadixPass &p) {
    constexpr int TILE = gs::SORT_THREADS * ITEMS;
    uint32_t *ghist = (uint32_t *)c.ghist->ptr;
    bool summed = false;
    if constexpr (COMPACT && TILE % gs::PP_CHUNK == 0) {
        // GS3D_CHUNK_HIST=0: the compacting pass counts its histogram from the keys again (A/B, tests)
        if (p.chunk_hist && !switches().chunk_hist_off) {
            // the preprocess kernel counted this digit per chunk: sum the chunks' rows instead of re-reading the keys
            hipLaunchKernelGGL((gs::k_sort_hist_chunks<RB, ITEMS>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st, p.chunk_hist, p.sc,
                               p.digit_mask, ghist, p.chunk_vis, p.nb, p.xr, p.chunk_hist_words);
            summed = true;
        }
    }
    if (!summed) {
        bool done = false;
        if constexpr (COMPACT) {
            if (p.pred.tau_dev) {
                hipLaunchKernelGGL((gs::k_sort_hist<KI, RB, COMPACT, ITEMS, true>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st,
                                   (const KI *)p.kin, p.sc, p.shift, p.digit_mask, ghist, p.chunk_vis, p.nb, p.xr, p.pred);
                done = true;
            }
        }
        if (!done)
            hipLaunchKernelGGL((gs::k_sort_hist<KI, RB, COMPACT, ITEMS>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st, (const KI *)p.kin,
                               p.sc, p.shift, p.digit_mask, ghist, p.chunk_vis, p.nb, p.xr, gs::CompactPred());
    }
    launch_scan_rows<TILE>(p.digit_mask + 1u, c.st, ghist, p.nb, p.sc, (uint32_t *)c.digit_totals->ptr);   // live rows only
    launch_scatter<KI, KO, RB, COMPACT, ITEMS>(c, p);
}

// XCD-aware tile order of a radix pass over `pnb` tiles (see run_sort_items): the span factor and the padded grid
static uint32_t xcd_span_for(uint32_t pnb, uint32_t &sgrid) {
    const int remap_c = switches().xcd_remap_c;
    uint32_t xr = 0;
    if (!switches().xcd_remap_off && pnb >= 256u) {
        xr = 4u;
        while (xr < 64u && xr * 2u * 256u <= pnb) xr *= 2u;
        if (remap_c > 1) xr = (uint32_t)remap_c;
    }
    sgrid = xr ? 8u * xr * ((pnb + 8u * xr - 1u) / (8u * xr)) : pnb;
    return xr;
}

// Stable LSD radix sort of (key, u32 value) pairs on key bits [0, end_bit), RB bits per pass at
// most (digit widths balanced over the passes), ping-ponging between side 0 and side 1; the side
// holding the result is returned.  `sc` = host bound of the count (sizes the grid) and, optionally,
// the device word holding the real count.  With `compact`, pass 0 reads keys[0] as the dense key
// array of preprocess and ignores vals[0].
template <typename K, int RB, int ITEMS>
static gs_status run_sort_items(const SortCtx &c, void *const keys[2], void *const vals[2], gs::SortCount sc, uint32_t end_bit,
                                const SortCompact *compact, int &result_side, uint32_t &passes_out,
                                const gs::ExpandIO *source = nullptr) {
    constexpr uint32_t R = 1u << RB;
    constexpr uint32_t TILE = (uint32_t)(gs::SORT_THREADS * ITEMS);
    uint32_t passes = (end_bit + RB - 1) / RB;
    if ((compact || source) && passes == 0) passes = 1;   // the compaction (and V) / the generation (and D) must happen even for a 0-bit key range
    passes_out = passes;
    result_side = 0;
    if (sc.count == 0 || passes == 0) return GS_OK;
    const uint32_t nb = (uint32_t)(((uint64_t)sc.count + TILE - 1) / TILE);
    GS_TRY(dev_reserve(*c.ghist, (size_t)nb * R * 4));
    GS_TRY(dev_reserve(*c.digit_totals, R * 4));
    int side = 0;
    uint32_t shift = 0;
    for (uint32_t i = 0; i < passes; i++) {
        // balanced digit widths: e.g. 13 bits -> 7 + 6, 15 -> 8 + 7, 27 -> 9 + 9 + 9, 32 -> 8 + 8 + 8 + 8
        const uint32_t bits = end_bit > shift ? (end_bit - shift + (passes - i) - 1) / (passes - i) : 0u;
        const bool first = compact && i == 0, last = i == passes - 1;
        RadixPass p;
        p.shift = shift;
        p.digit_mask = (1u << bits) - 1u;
        p.kin = first ? (const void *)compact->dense_keys : keys[side];
        p.vin = (const uint32_t *)vals[side];
        // the sorted depth keys themselves are never read (compact = the frame's depth sort): its last pass
        // writes the order only
        p.kout = compact && last ? nullptr : keys[side ^ 1];
        p.vout = (uint32_t *)vals[side ^ 1];
        p.sc = first ? gs::SortCount{compact->dense_count, compact->dense_count_dev} : sc;
        p.nb = first ? (uint32_t)(((uint64_t)compact->dense_count + TILE - 1) / TILE) : nb;
        if (first) GS_TRY(dev_reserve(*c.ghist, (size_t)p.nb * R * 4));
        if (first) {
            p.chunk_vis = compact->chunk_vis;
            p.visible_out = compact->visible_out;
            p.chunk_hist = compact->chunk_hist;
        }
        if (compact) p.pred = compact->pred;
        // XCD-aware tile order in the scatter (see scatter_tile_of): XCD x takes `xr` consecutive tiles
        // of every group of 8 * xr.  xr grows with the number of tiles (a group must stay a small part
        // of the pass) between 4 and 64.  GS3D_XCD_REMAP=0 disables, GS3D_XCD_REMAP_C=<n> forces a size.
        p.xr = xcd_span_for(p.nb, p.sgrid);
        if (compact && last) p.bucket_max = compact->bucket_max;   // the depth sort's pass on its top digit reports the largest bucket
        if (source && i == 0) {
            // the pairs come from the depth-ordered rects: k_pairs_emit writes this pass's input
            // (keys[side] / vals[side]) and its histogram at once
            if constexpr (sizeof(K) <= 4) {
                gs::ExpandIO src = *source;
                src.tvals = (uint32_t *)vals[side];
                if (sizeof(K) == 2 && src.rect32)
                    hipLaunchKernelGGL((gs::k_pairs_emit<K, RB, ITEMS, sizeof(K) == 2>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st,
                                       src, p.digit_mask, (uint32_t *)c.ghist->ptr, (K *)keys[side], p.nb, p.xr, 0u);
                else
                    hipLaunchKernelGGL((gs::k_pairs_emit<K, RB, ITEMS, false>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st, src,
                                       p.digit_mask, (uint32_t *)c.ghist->ptr, (K *)keys[side], p.nb, p.xr, 0u);
                launch_scan_rows<(int)TILE>(p.digit_mask + 1u, c.st, (uint32_t *)c.ghist->ptr, p.nb, p.sc, (uint32_t *)c.digit_totals->ptr);
                launch_scatter<K, K, RB, false, ITEMS>(c, p);
            }
        } else if constexpr (sizeof(K) == 4) {
            // Narrow keys (the frame's depth sort only): the pass BEFORE the last stores key >> (shift of
            // the last pass) as u16 — all the last pass still needs — and the last pass runs on 16-bit keys:
            // 2 bytes less per element written, 2 x 2 bytes less read.  GS3D_NARROW_KEYS=0 switches it off.
            const bool narrow = !switches().narrow_keys_off && compact && passes >= 2;
            const bool writes_narrow = narrow && i == passes - 2, reads_narrow = narrow && last;
            if (reads_narrow) {
                p.kout = nullptr;
                p.shift = 0u;
                launch_pass<uint16_t, uint16_t, RB, false, ITEMS>(c, p);
            } else if (writes_narrow) {
                p.kout = keys[side ^ 1];
                p.ko_shift = shift + bits;
                if (first) launch_pass<uint32_t, uint16_t, RB, true, ITEMS>(c, p);
                else launch_pass<uint32_t, uint16_t, RB, false, ITEMS>(c, p);
            } else if (first) {
                launch_pass<K, K, RB, true, ITEMS>(c, p);
            } else {
                launch_pass<K, K, RB, false, ITEMS>(c, p);
            }
        } else {
            launch_pass<K, K, RB, false, ITEMS>(c, p);
        }
        c.count(3);
        shift += bits;
        side ^= 1;
    }
    GS_HIP(hipGetLastError());
    result_side = side;
    return GS_OK;
}

// the depth sorts' tile size from the host's bound of the count (see SortCfg): fn(integral_constant ITEMS)
static int depth_sort_items(uint32_t n) { return n >= (4u << 20) ? gs::SortCfg<uint32_t>::ITEMS_LARGE : gs::SortCfg<uint32_t>::ITEMS; }
template <class F>
static gs_status with_depth_items(uint32_t n, F fn) {
    if (n >= (4u << 20)) return fn(std::integral_constant<int, gs::SortCfg<uint32_t>::ITEMS_LARGE>());
    return fn(std::integral_constant<int, gs::SortCfg<uint32_t>::ITEMS>());
}

// The histogram half of that pass on its own (partitioned two-round frames: gs::k_round_threshold needs the totals of the top
// digit before any sort runs): the chunk rows of the preprocess kernel summed per tile, the rows scanned; digit_totals
// holds the 1024 totals afterwards.
template <int ITEMS>
static gs_status run_top_digit_totals(gs_renderer *r, hipStream_t st, uint32_t dense_count, const uint32_t *dense_count_dev) {
    constexpr int RB = gs::MSD_TOP_BITS;
    constexpr uint32_t R = 1u << RB, TILE = (uint32_t)(gs::SORT_THREADS * ITEMS);
    const uint32_t pnb = (uint32_t)(((uint64_t)dense_count + TILE - 1) / TILE);
    GS_TRY(dev_reserve(r->ghist, (size_t)pnb * R * 4));
    GS_TRY(dev_reserve(r->digit_totals, R * 4));
    uint32_t sgrid = 0;
    const uint32_t xr = xcd_span_for(pnb, sgrid);
    const gs::SortCount psc{dense_count, dense_count_dev};
    hipLaunchKernelGGL((gs::k_sort_hist_chunks<RB, ITEMS>), dim3(sgrid), dim3(gs::SORT_THREADS), 0, st, (const uint32_t *)r->chunk_hist.ptr, psc,
                       R - 1u, (uint32_t *)r->ghist.ptr, (const uint32_t *)r->chunk_vis.ptr, pnb, xr, R / 2u);
    launch_scan_rows<(int)TILE>(R, st, (uint32_t *)r->ghist.ptr, pnb, psc, (uint32_t *)r->digit_totals.ptr);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// k_bucket_sort behind an MSD-first scatter pass: the fields both sorts fill the same way (the caller sets nb, the
// key / value arrays, bucket_max and the ranges), and the launch
static gs::BucketSortIO bucket_sort_io(const SortCtx &c, gs_renderer *r, uint32_t low_bits) {
    gs::BucketSortIO io;
    io.totals = (const uint32_t *)r->digit_totals.ptr;
    io.starts = (const uint32_t *)r->bucket_starts.ptr;
    io.low_bits = low_bits;
    io.keys_tmp = nullptr;
    io.vals_tmp = nullptr;
    io.ranges = nullptr;
    io.num_tiles = 0;
    io.rank_fault = c.rank_fault;
    io.watch = c.watch;
    return io;
}
template <typename K, int RBL, int THREADS>
static void launch_bucket_sort(const SortCtx &c, const gs::BucketSortIO &io) {
    with_rank(c, [&](auto fast_tag, uint32_t *, uint32_t) {
        hipLaunchKernelGGL((gs::k_bucket_sort<K, RBL, THREADS, decltype(fast_tag)::value>), dim3(io.nb), dim3(THREADS), 0, c.st, io);
    });
}

// The frame's depth sort, MSD-first (round 5; gs_render_kernels.h, "Bucket sort"): ONE compacting scatter pass on the TOP
// 10 bits of the depth key — its histogram summed from the rows the preprocess kernel counted — then one workgroup per
// bucket sorts the remaining low bits on its CU and writes the final order to vals[0].  4 launches instead of 9; right
// when the buckets fit a workgroup (up to ~1-2 M visible Gaussians spread in depth), which the caller decides from the
// bucket sizes the last frames reported.  `scratch_*`: two passes of the chunked fallback (oversized buckets).
template <int ITEMS>
static gs_status run_depth_msd_items(const SortCtx &c, gs_renderer *r, const SortCompact &cp, uint32_t dbits, uint32_t top_range,
                                     void *scratch_keys, void *scratch_vals, uint32_t &passes_out) {
    constexpr int RB = gs::MSD_TOP_BITS, RBL = gs::RADIX_BITS_MAX;     // top digit 10 bits; two bucket passes of up to 9 below it
    constexpr uint32_t R = 1u << RB, TILE = (uint32_t)(gs::SORT_THREADS * ITEMS);
    const uint32_t low_bits = dbits - (uint32_t)RB;
    RadixPass p;
    p.nb = (uint32_t)(((uint64_t)cp.dense_count + TILE - 1) / TILE);
    GS_TRY(dev_reserve(r->ghist, (size_t)p.nb * R * 4));
    GS_TRY(dev_reserve(r->digit_totals, R * 4));
    GS_TRY(dev_reserve(r->bucket_starts, R * 4));
    p.xr = xcd_span_for(p.nb, p.sgrid);
    p.sc = gs::SortCount{cp.dense_count, cp.dense_count_dev};
    p.kin = cp.dense_keys;
    p.kout = r->dkeys[1].ptr;
    p.vout = (uint32_t *)r->dvals[1].ptr;
    p.shift = low_bits;
    p.digit_mask = R - 1u;
    p.chunk_vis = cp.chunk_vis;
    p.visible_out = cp.visible_out;
    p.pred = cp.pred;
    p.chunk_hist = cp.chunk_hist;
    p.chunk_hist_words = R / 2u;
    p.bucket_starts = (uint32_t *)r->bucket_starts.ptr;
    launch_pass<uint32_t, uint32_t, RB, true, ITEMS>(c, p);
    gs::BucketSortIO io = bucket_sort_io(c, r, low_bits);
    io.nb = top_range < R ? top_range : R;          // digits past the far plane's cannot occur (their totals are zero)
    io.keys_in = r->dkeys[1].ptr;
    io.vals_in = (const uint32_t *)r->dvals[1].ptr;
    io.keys_tmp = scratch_keys;
    io.vals_tmp = (uint32_t *)scratch_vals;
    io.keys_out = nullptr;                          // nobody reads the sorted depth keys
    io.vals_out = (uint32_t *)r->dvals[0].ptr;
    io.bucket_max = cp.bucket_max;
    launch_bucket_sort<uint32_t, RBL, gs::BKT_THREADS>(c, io);
    GS_HIP(hipGetLastError());
    c.count(4);
    passes_out = 1u + (low_bits + RBL - 1u) / RBL;
    return GS_OK;
}

// The frame's tile sort, MSD-first (u16 tile ids, more than 1024 tiles): k_pairs_emit counts the TOP 10 bits of the tile id
// while it writes the pairs, one scatter pass partitions them into buckets of 2^low_bits consecutive tiles (each in depth
// order), and k_bucket_sort finishes every bucket with one counting pass on the low bits — which also yields the tiles'
// [start, end) ranges: no second histogram / row scan / scatter and no range kernel, 4 launches instead of 7.  Result on
// side 0 (keys too: the parity tap rebuilds the 64-bit keys from them).
template <int ITEMS>
static gs_status run_tile_msd_items(const SortCtx &c, gs_renderer *r, const gs::ExpandIO &eo, gs::SortCount tc, uint32_t tile_bits,
                                    uint32_t num_tiles, uint32_t *ranges, uint32_t *bucket_max, uint32_t &passes_out) {
    constexpr int RB = gs::MSD_TOP_BITS, RBL = 6;        // top digit 10 bits; up to 6 bits (65536 tiles) left for the buckets
    constexpr uint32_t R = 1u << RB, TILE = (uint32_t)(gs::SORT_THREADS * ITEMS);
    const uint32_t low_bits = tile_bits - (uint32_t)RB;
    RadixPass p;
    p.nb = (uint32_t)(((uint64_t)tc.count + TILE - 1) / TILE);
    GS_TRY(dev_reserve(r->ghist, (size_t)p.nb * R * 4));
    GS_TRY(dev_reserve(r->digit_totals, R * 4));
    p.xr = xcd_span_for(p.nb, p.sgrid);
    gs::ExpandIO src = eo;
    src.tvals = (uint32_t *)r->tvals[0].ptr;
    if (src.rect32)
        hipLaunchKernelGGL((gs::k_pairs_emit<uint16_t, RB, ITEMS, true>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st, src, R - 1u,
                           (uint32_t *)r->ghist.ptr, (uint16_t *)r->tkeys[0].ptr, p.nb, p.xr, low_bits);
    else
        hipLaunchKernelGGL((gs::k_pairs_emit<uint16_t, RB, ITEMS, false>), dim3(p.sgrid), dim3(gs::SORT_THREADS), 0, c.st, src, R - 1u,
                           (uint32_t *)r->ghist.ptr, (uint16_t *)r->tkeys[0].ptr, p.nb, p.xr, low_bits);
    launch_scan_rows<(int)TILE>(R, c.st, (uint32_t *)r->ghist.ptr, p.nb, tc, (uint32_t *)r->digit_totals.ptr);
    GS_TRY(dev_reserve(r->bucket_starts, R * 4));
    p.kin = r->tkeys[0].ptr;
    p.vin = (const uint32_t *)r->tvals[0].ptr;
    p.kout = r->tkeys[1].ptr;
    p.vout = (uint32_t *)r->tvals[1].ptr;
    p.sc = tc;
    p.shift = low_bits;
    p.digit_mask = R - 1u;
    p.bucket_starts = (uint32_t *)r->bucket_starts.ptr;
    launch_scatter<uint16_t, uint16_t, RB, false, ITEMS>(c, p);
    gs::BucketSortIO io = bucket_sort_io(c, r, low_bits);
    io.nb = ((num_tiles - 1u) >> low_bits) + 1u;
    io.keys_in = r->tkeys[1].ptr;
    io.vals_in = (const uint32_t *)r->tvals[1].ptr;
    io.keys_out = r->tkeys[0].ptr;                  // (one pass: the chunked path needs no scratch)
    io.vals_out = (uint32_t *)r->tvals[0].ptr;
    io.bucket_max = bucket_max;
    io.ranges = ranges;
    io.num_tiles = num_tiles;
    launch_bucket_sort<uint16_t, RBL, gs::BKT_THREADS_SMALL>(c, io);
    GS_HIP(hipGetLastError());
    c.count(4);
    passes_out = low_bits ? 2u : 1u;
    return GS_OK;
}

// tile size from the host-side bound of the element count (see SortCfg)
template <typename K, int RB>
static gs_status run_sort_rb(const SortCtx &c, void *const keys[2], void *const vals[2], gs::SortCount sc, uint32_t end_bit,
                             const SortCompact *compact, int &result_side, uint32_t &passes_out, const gs::ExpandIO *source = nullptr) {
    const uint64_t bound = compact ? compact->dense_count : sc.count;
    if constexpr (gs::SortCfg<K>::ITEMS_LARGE != gs::SortCfg<K>::ITEMS) {
        // u32 keys: larger tiles for larger sorts.  u16 tile keys: a tile's digit runs should hold >= 32
        // elements — 4096-key tiles do for digits of up to 7 bits (1080p: 13 tile bits = 7 + 6) and fit
        // twice as many workgroups per CU (10 M: emit + tile sort 376 -> 358 us); 8-bit digits (4K: 15
        // bits = 8 + 7) keep 8192-key tiles (848 vs 875 us with the small ones).
        bool large = bound >= (4u << 20);
        // GS3D_DEPTH_SORT_LARGE=0/1 forces 4096- / 8192-key tiles for 32-bit keys (A/B runs)
        if (sizeof(K) == 4 && switches().depth_sort_large >= 0) large = switches().depth_sort_large != 0;
        if (sizeof(K) == 2) {
            const uint32_t passes = (end_bit + RB - 1) / RB;
            large = passes ? (end_bit + passes - 1) / passes > 7u : false;
            // GS3D_TILE_SORT_LARGE=0/1 forces 4096- / 8192-key tiles for the 16-bit tile keys (A/B runs)
            if (switches().tile_sort_large >= 0) large = switches().tile_sort_large != 0;
        }
        if (large) return run_sort_items<K, RB, gs::SortCfg<K>::ITEMS_LARGE>(c, keys, vals, sc, end_bit, compact, result_side, passes_out, source);
    }
    return run_sort_items<K, RB, gs::SortCfg<K>::ITEMS>(c, keys, vals, sc, end_bit, compact, result_side, passes_out, source);
}

// host-known count (spatial order build, stand-alone sort)
template <typename K>
gs_status gsh::sort_pairs_device(const gs_device *dev, void *const keys[2], void *const vals[2],
                                 DevArray &ghist, DevArray &digit_totals, uint32_t count,
                                 uint32_t end_bit, hipStream_t st, int &result_side,
                                 uint32_t &passes_out) {
    return run_sort_rb<K, gs::RADIX_BITS>(standalone_sort_ctx(dev, st, ghist, digit_totals), keys, vals, gs::SortCount{count, nullptr}, end_bit,
                                          nullptr, result_side, passes_out);
}
// (the neighbour counts sort 64-bit keys from their own unit)
template gs_status gsh::sort_pairs_device<uint64_t>(const gs_device *, void *const[2], void *const[2], DevArray &, DevArray &, uint32_t, uint32_t,
                                                    hipStream_t, int &, uint32_t &);

// the two kernels of this unit that other units launch too (gs_host.h)
void gsh::scan_chunks_enqueue(hipStream_t st, const uint32_t *in, uint32_t *out, uint32_t *total, uint32_t n) {
    gs::ScanJob job{in, out, total, n};
    hipLaunchKernelGGL(gs::k_scan_chunks, dim3(1), dim3(1024), 0, st, job, job);
}
void gsh::bbox_final_enqueue(hipStream_t st, const float *partial, uint32_t count, float *bbox) {
    hipLaunchKernelGGL(gs::k_bbox_final, dim3(1), dim3(256), 0, st, partial, count, bbox);
}

// (Re)build the block-planar mirror on `st`.  A whole-buffer rebuild in spatial mode first computes
// the order: bounding box of the positions -> 30-bit Morton keys -> stable radix sort -> order / inv.
static gs_status build_spatial_order(gs_gaussians_buffer *g, hipStream_t st, size_t len) {
    gs_device *dev = g->buf->dev;
    const uint32_t n = (uint32_t)len, pod_words = (uint32_t)(pod_stride(g) / 4);
    DevArray keys[2], vals[2], gh, dt, partial, bbox;
    for (int i = 0; i < 2; i++) {
        GS_TRY(dev_reserve(keys[i], (size_t)n * 4));
        GS_TRY(dev_reserve(vals[i], (size_t)n * 4));
    }
    const uint32_t pgrid = n / 256u + 1u < 1024u ? n / 256u + 1u : 1024u;
    GS_TRY(dev_reserve(partial, (size_t)pgrid * 24));
    GS_TRY(dev_reserve(bbox, 24));
    // From here on every return, the last one too, frees scratch that the queued kernels may still use, and none waits
    // for the stream first: it relies on hipFree synchronising the device, as this function always has.
    hipLaunchKernelGGL(gs::k_bbox_partial, dim3(pgrid), dim3(256), 0, st, (const uint32_t *)g->buf->ptr,
                       pod_words, n, (float *)partial.ptr);
    bbox_final_enqueue(st, (const float *)partial.ptr, pgrid, (float *)bbox.ptr);
    hipLaunchKernelGGL(gs::k_morton_keys, dim3((n + 255u) / 256u), dim3(256), 0, st,
                       (const uint32_t *)g->buf->ptr, pod_words, n, (const float *)bbox.ptr,
                       (uint32_t *)keys[0].ptr, (uint32_t *)vals[0].ptr);
    void *k2[2] = {keys[0].ptr, keys[1].ptr};
    void *v2[2] = {vals[0].ptr, vals[1].ptr};
    int side = 0;
    uint32_t passes = 0;
    GS_TRY(sort_pairs_device<uint32_t>(dev, k2, v2, gh, dt, n, 30, st, side, passes));
    // the sorted values ARE the order: keep that array as a ref-counted buffer, free the rest
    if (g->order) gs_buffer_release(g->order);
    g->order = make_buffer(dev, vals[side].release(), (size_t)n * 4, true);
    (void)g->inv.free();
    const hipError_t e = g->inv.alloc_raw((size_t)n * 4);
    if (e != hipSuccess) return gs_fail(GS_ERR_OUT_OF_MEMORY, (size_t)n * 4, 0, 0, "hipMalloc failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(gs::k_invert_order, dim3((n + 255u) / 256u), dim3(256), 0, st,
                       (const uint32_t *)g->order->ptr, n, (uint32_t *)g->inv.ptr);
    if (hipGetLastError() != hipSuccess) return gs_fail(GS_ERR_HIP, 0, 0, 0, "spatial order launch failed");
    return GS_OK;
}

static gs_status ensure_planar(gs_gaussians_buffer *g, hipStream_t st) {
    size_t len = gs_gaussians_buffer_len(g);
    size_t stride = (len + gs::PLANAR_BLOCK - 1) / gs::PLANAR_BLOCK * gs::PLANAR_BLOCK;   // whole blocks
    uint32_t chunks = (uint32_t)(pod_stride(g) / 16);
    if (!g->planar.ptr || g->planar_stride != stride) {
        GS_HIP_AS("hipFree(g->planar)", g->planar.free());
        GS_HIP_AS("hipFree(g->block_bounds)", g->block_bounds.free());
        // (when this fails the mirror is gone and the stride stale: the next frame comes through here again)
        GS_HIP_AS("hipMalloc(&g->planar, (stride ? stride : gs::PLANAR_BLOCK) * 16 * chunks)",
                  g->planar.alloc_raw((stride ? stride : gs::PLANAR_BLOCK) * 16 * chunks));
        g->planar_stride = stride;
        g->mark_all();
    }
    size_t lo = g->dirty_lo, hi = g->dirty_hi < len ? g->dirty_hi : len;
    // Re-sort policy: a partial update keeps the slots of the Gaussians it rewrites, so the spatial
    // order decays under an editor's stream of update_range calls (moved Gaussians stay in the
    // blocks of their old neighbourhood: block bounds grow, culling gets weaker — results never
    // change).  Once the partial updates since the last ordering add up to a quarter of the buffer,
    // the next frame rebuilds the order (one Morton sort + ordered repack, ~2 ms per 10 M).
    if (g->spatial && g->order && lo < hi && g->partial_since_order > len / 4) {
        lo = 0;
        hi = len;
        g->keep_order = false;
    }
    if (lo < hi) {
        // the records may have been edited on another stream (gs_gaussians_buffer_edit only enqueues)
        GS_TRY(wait_for_edits(g, st));
        const bool whole = lo == 0 && hi == len && !g->keep_order;
        if (whole) g->partial_since_order = 0;
        const bool want_order = g->spatial && len > 1;
        if (whole || want_order != (g->order != nullptr)) {
            // whole-buffer (re)mirror: this is where the spatial order is (re)computed or dropped
            g->order_epoch++;
            if (want_order) {
                GS_TRY(build_spatial_order(g, st, len));
            } else {
                if (g->order) gs_buffer_release(g->order);
                g->order = nullptr;
                GS_HIP_AS("hipFree(g->inv)", g->inv.free());
            }
            lo = 0;
            hi = len;
        }
        uint64_t count = hi - lo;
        if (g->order && lo == 0 && hi == len) {
            uint32_t grid = (uint32_t)((count + gs::REPACK_GROUP - 1) / gs::REPACK_GROUP);
            hipLaunchKernelGGL(gs::k_repack_planar_ordered, dim3(grid), dim3(256), 0, st,
                               (const uint4 *)g->buf->ptr, (uint4 *)g->planar.ptr, (const uint32_t *)g->order->ptr,
                               count, chunks);
        } else if (g->order) {
            uint64_t total = count * chunks;
            uint32_t grid = (uint32_t)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
            hipLaunchKernelGGL(gs::k_repack_planar_scatter, dim3(grid), dim3(256), 0, st,
                               (const uint4 *)g->buf->ptr, (uint4 *)g->planar.ptr, (const uint32_t *)g->inv.ptr,
                               (uint64_t)lo, count, chunks);
        } else {
            uint32_t grid = (uint32_t)((count + gs::REPACK_GROUP - 1) / gs::REPACK_GROUP);
            hipLaunchKernelGGL(gs::k_repack_planar, dim3(grid), dim3(256), 0, st,
                               (const uint4 *)g->buf->ptr, (uint4 *)g->planar.ptr, (uint64_t)lo, count, chunks);
        }
        GS_HIP(hipGetLastError());
        // per-block bounds for the preprocess kernels' block culling (recomputed for every block:
        // 48 bytes per Gaussian, cheaper than tracking which blocks a partial update touched)
        const uint32_t nblocks = (uint32_t)((len + gs::PLANAR_BLOCK - 1) / gs::PLANAR_BLOCK);
        if (!g->block_bounds.ptr)
            GS_HIP_AS("hipMalloc(&g->block_bounds, (stride / gs::PLANAR_BLOCK + 1) * 32)", g->block_bounds.alloc_raw((stride / gs::PLANAR_BLOCK + 1) * 32));
        hipLaunchKernelGGL(k_tbl_block_bounds[g->sh][g->cov], dim3(nblocks), dim3(gs::PP_THREADS), 0, st,
                           (const uint4 *)g->planar.ptr, (uint32_t)len, (float *)g->block_bounds.ptr);
        GS_HIP(hipGetLastError());
        if (!g->mirror_ready) GS_HIP_AS("hipEventCreateWithFlags(&g->mirror_ready, hipEventDisableTiming)", g->mirror_ready.create());
        GS_HIP(hipEventRecord(g->mirror_ready, st));
        g->mirror_stream = st;
    } else if (g->mirror_ready && st != g->mirror_stream) {
        // the mirror was built on another stream: order this stream behind that build
        GS_HIP(hipStreamWaitEvent(st, g->mirror_ready, 0));
    }
    g->dirty_lo = g->dirty_hi = 0;
    g->keep_order = false;
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_set_spatial_order(gs_gaussians_buffer *g, int32_t enabled) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    if (g->spatial != (enabled != 0)) {
        g->spatial = enabled != 0;
        g->mark_all();
    }
    return GS_OK;
}

extern "C" int32_t gs_gaussians_buffer_spatial_order(const gs_gaussians_buffer *g) {
    return g && g->spatial ? 1 : 0;
}

extern "C" gs_status gs_gaussians_buffer_download_order(gs_gaussians_buffer *g, gs_stream *s,
                                                        uint32_t *order_out, size_t count) {
    if (!g || (count && !order_out)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    size_t len = gs_gaussians_buffer_len(g);
    if (count != len)
        return gs_fail(GS_ERR_COUNT_MISMATCH, count, len, 0, "Gaussians count mismatch: %zu != %zu", count, len);
    GS_TRY(use_device(g->buf->dev));
    hipStream_t st = stream_of(g->buf->dev, s);
    GS_TRY(ensure_planar(g, st));
    if (!g->order) {
        for (size_t i = 0; i < len; i++) order_out[i] = (uint32_t)i;
        return GS_OK;
    }
    GS_HIP(hipStreamSynchronize(st));
    hipError_t e = hipMemcpy(order_out, g->order->ptr, len * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    return GS_OK;
}

// roctx ranges around the stages of a frame (the tracing hook of this path).  The marker
// library is looked up at run time and only when GS3D_ROCTX=1, so the product has no link-time
// dependency on a profiler and pays nothing otherwise.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        if (!switches().roctx) return;
        for (const char *name : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
            if (push && pop) return;
            push = nullptr;
            pop = nullptr;
        }
    }
};
static Roctx &roctx() {
    static Roctx r;
    return r;
}
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char *name) : on(roctx().push != nullptr) {
        if (on) roctx().push(name);
    }
    void next(const char *name) {
        if (on) {
            roctx().pop();
            roctx().push(name);
        }
    }
    ~RoctxRange() {
        if (on) roctx().pop();
    }
};

static const gsp::PolicyParams k_policy_params = {(uint32_t)gs::BKT_CAP, (uint32_t)gs::BKT_CAP_SMALL, (uint32_t)gs::MSD_TOP_BITS,
                                                  (uint32_t)gs::RADIX_BITS_MAX};

// ---- what the previous frames told us (never blocks: an unfinished frame is simply not consulted) ----
// The snapshot carries the renderer's shape epoch of THIS moment.  gs_render_frame bumps the epoch later (stage_preprocess),
// but only in a sizing frame (or with n == 0), and every rule that compares a report's epoch is guarded by !sizing: a
// snapshot taken before the bump answers the same as a read behind it.
static gsp::History read_history(gs_renderer *r) {
    gsp::History h;
    h.shape_epoch = r->shape_epoch;
    for (int i = 0; i < 2; i++) {
        if (switches().frame_event) {
            if (!r->done_valid[i] || hipEventQuery(r->done[i]) != hipSuccess) continue;
        } else if (!r->done_gen[i]) {
            continue;
        }
        const gs::FrameResult &fr = r->results.ptr[i];
        // gen is published last with a system-scope release (publish_result): read it first — and once more behind the
        // fields (a frame two generations on may be overwriting the block while it is read)
        if (__atomic_load_n(&fr.gen, __ATOMIC_ACQUIRE) != r->done_gen[i]) continue;
        gsp::Report p;
        p.pairs = fr.pairs_total;
        p.visible = fr.visible;
        const uint32_t f_flags = fr.flags;
        p.depth_bucket_max = fr.depth_bucket_max;
        p.tile_bucket_max = fr.tile_bucket_max;
        p.tiles_done = fr.tiles_done;
        p.tiles_open = fr.tiles_open;
        p.round_pairs_max = fr.round_pairs_max;
        if (__atomic_load_n(&fr.gen, __ATOMIC_ACQUIRE) != r->done_gen[i] || p.pairs > 0xfffffff0ull) continue;
        p.gen = r->done_gen[i];
        p.shape_epoch = r->done_shape[i];
        p.rounds = r->done_rounds[i];
        p.round_k = r->done_round_k[i];
        h.rep[i] = p;
        if (f_flags & gs::FRAME_FLAG_RANK_FAULT) h.rank_fault_seen = true;
    }
    (void)hipGetLastError();   // hipEventQuery reports hipErrorNotReady through the sticky error too
    return h;
}

static gs_status reserve_pairs(gs_renderer *r, uint64_t pairs, bool wide) {
    if (pairs <= r->pair_capacity && r->tkeys[0].ptr && wide == r->wide_tiles) return GS_OK;
    uint64_t cap = pairs;
    if (cap < r->pair_capacity) cap = r->pair_capacity;
    if (cap > 0xfffffff0ull) cap = 0xfffffff0ull;   // pair indices are 32-bit
    for (int i = 0; i < 2; i++) {
        GS_TRY(dev_reserve(r->tkeys[i], cap * (wide ? 4 : 2) + 64));
        GS_TRY(dev_reserve(r->tvals[i], cap * 4 + 64));
    }
    GS_TRY(dev_reserve(r->cursors, (size_t)(cap / gs::CURSOR_SLOTS + 2) * sizeof(gs::PairCursorRec)));
    r->pair_capacity = cap;
    r->wide_tiles = wide;
    return GS_OK;
}

static uint32_t float_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// device memory that must start out as zeros (the frame state: V and D live there between kernels)
static gs_status reserve_zeroed(DevArray &a, size_t bytes, hipStream_t st) {
    if (a.bytes >= bytes && a.ptr) return GS_OK;
    GS_TRY(dev_reserve(a, bytes));
    GS_HIP(hipMemsetAsync(a.ptr, 0, a.bytes, st));
    return GS_OK;
}

// stage boundaries of a frame: timing events and roctx ranges
struct StageMarks {
    gs_renderer *r;
    hipStream_t st;
    bool timing;
    RoctxRange range{"gs3d:frame"};
    RoctxRange stage{"gs3d:setup"};
    void mark(int i) {
        static const char *const k_stage_names[ST_COUNT] = {"gs3d:repack", "gs3d:preprocess", "gs3d:sizing", "gs3d:depth_sort",
                                                            "gs3d:expand", "gs3d:tile_sort", "gs3d:ranges", "gs3d:blend",
                                                            "gs3d:end"};
        if (timing) (void)hipEventRecord(r->ev[i], st);
        stage.next(k_stage_names[i]);
    }
};

// From the frame's first launch on, kernels of this frame may be in the stream.  Whatever way the function is left — also
// through GS_TRY / GS_HIP after an allocation or launch failure — the end-of-frame event of this
// generation is recorded behind them, so the next frame on ANOTHER stream waits for exactly these
// kernels before it touches the shared scratch and state buffers (a frame that failed half-way used
// to leave done[gen & 1] pointing at frame gen - 2).  Its result block carries no `gen`, so the
// capacity history skips it.
struct DoneGuard {
    gs_renderer *r;
    hipStream_t st;
    uint32_t gen;
    bool record;
    ~DoneGuard() {
        if (record) {
            (void)hipEventRecord(r->done[gen & 1u], st);
            r->done_valid[gen & 1u] = true;
        } else {
            r->done_valid[gen & 1u] = false;      // recorded when (if) the renderer moves to another stream
        }
        r->done_gen[gen & 1u] = gen;
        r->done_shape[gen & 1u] = r->shape_epoch;
        r->done_rounds[gen & 1u] = r->two_round ? 2 : 1;
        r->done_round_k[gen & 1u] = r->two_round ? r->round1 : 0u;
    }
};

// What the stages of one frame share.  aux: the depth / pick planes (gs_render_frame_aux, checked there), or null.  Only
// stage_blend looks at it: the frame makes every other choice as it would without it.
struct Frame {
    gs_renderer *r;
    hipStream_t st;
    gs_gaussians_buffer *g;
    const gs_aux_targets *aux;
    float *rgba;
    const gs_frame_selection *fs;     // hide / tint selections (gs_render_frame_sel, checked there), or null: the plain frame
    StageMarks marks;
    gs::FrameConsts fc;
    FrameShape shape;
    gsp::FrameNums nums;
    gsp::History hist;
    gsp::FramePlan plan;
    SortCtx sort;
    uint32_t mode, gen = 0, n = 0, nchunks = 0, num_tiles = 0, exp_grid = 0;
    uint32_t near_bits = 0, far_bits = 0;
    size_t nn = 1, nc = 1, nslots = 0;
    gs::FrameState *state = nullptr;
    gs::FrameResult *result = nullptr;
    // slices of zero_region: tile ranges, the two rounds' super-chunk sums, the finished / open tile bits
    uint32_t *zero = nullptr, *esb = nullptr, *esb2 = nullptr, *done_bits = nullptr, *open_bits = nullptr;
    gs::TileKeys tile_keys{nullptr, nullptr, 0u, 0u, 0u, 0u, nullptr, nullptr};   // null keys: the blend reads its ranges from the range array
    gs::SelIO sel{};                  // selection frames: what the preprocess kernels read (stage_selection)
    gs_buffer *contrib = nullptr;     // contribution frames (gs_render_frame_contrib, checked there): the records the blend adds to, or null
    gsp::Requests requests() const {
        gsp::Requests q;
        q.depth_msd = r->depth_msd_req;
        q.tile_msd = r->tile_msd_req;
        q.tile_masks = r->tile_masks_req;
        q.rounds = r->rounds_req;
        q.round1 = r->round1_req;
        q.single_round = contrib != nullptr;
        return q;
    }
};

// the frame's scratch that depends on N alone
static gs_status reserve_frame_scratch(Frame &F) {
    gs_renderer *r = F.r;
    const size_t nn = F.nn, nc = F.nc;
    // per-slot outputs of preprocess: whole chunks — a list frame addresses them in list space, where the
    // buffer's last, partial block may sit anywhere and its lanes past N are written too (as "culled")
    const size_t nslots = F.nslots;
    GS_TRY(dev_reserve(r->recs, nslots * 4 * gs::REC_WORDS + 16));
    GS_TRY(dev_reserve(r->depth, nslots * 4));
    GS_TRY(dev_reserve(r->rect, nslots * 8));
    GS_TRY(dev_reserve(r->sorted_rect, (nn + 1024) * 8));   // padded: k_pairs_emit reads whole batches
    GS_TRY(dev_reserve(r->chunk_tiles, nc * 4));
    GS_TRY(dev_reserve(r->chunk_vis, nc * 4));
    GS_TRY(dev_reserve(r->chunk_hist, nc * (size_t)(gs::PRE_HIST_BINS / 2) * 4));
    GS_TRY(dev_reserve(r->scan_tmp, nc * 4));
    for (int i = 0; i < 2; i++) {
        GS_TRY(dev_reserve(r->dkeys[i], nn * 4));
        GS_TRY(dev_reserve(r->dvals[i], (nn + 1024) * 4));
    }
    {
        // The sorts' histogram rows and digit totals at the largest size any depth pass of this scene may ask for (the top-digit
        // histogram of an MSD-first sort or of a partitioned two-round frame: 1024 rows): reserved HERE, in the frame that sizes
        // the scene, because growing them later means a hipFree under frames in flight — a device-wide wait at best (and under
        // rocprofv3 --pmc the 10 M bench hung in it: the first partitioned frame doubled `ghist` behind eight queued frames).
        const size_t depth_tile = (size_t)gs::SORT_THREADS * depth_sort_items(F.n);
        GS_TRY(dev_reserve(r->ghist, ((size_t)nn + depth_tile - 1) / depth_tile * ((size_t)4 << gs::MSD_TOP_BITS)));
        GS_TRY(dev_reserve(r->digit_totals, (size_t)4 << gs::MSD_TOP_BITS));
    }
    GS_TRY(dev_reserve(r->exp_sums, (size_t)(F.exp_grid ? F.exp_grid : 1) * 4));
    GS_TRY(reserve_zeroed(r->state, sizeof(gs::FrameState), F.st));
    return GS_OK;
}

// Watchdog of the LDS-atomic rank (scatter_ranked): a completed frame reported a rank that was not the
// ballot-based one -> this device sorts with the ballot-based rank from now on, and the flag is cleared in
// stream order (the kernels that could set it are no longer launched).  Fills the frame's sort context but its sample.
static gs_status arm_rank_watchdog(Frame &F) {
    gs_renderer *r = F.r;
    gs::FrameState *fs = (gs::FrameState *)r->state.ptr;
    if (F.hist.rank_fault_seen) {
        // (the word is this renderer's own and is cleared whoever switched the device: see gs_renderer_wait_frame)
        r->dev->lds_atomic_ordered.store(false);
        GS_HIP(hipMemsetAsync(&fs->rank_fault, 0, sizeof(uint32_t), F.st));
    }
    // GS3D_TEST_RANK_FAULT=1 (tests): the watchdog's expectation is off by one, so it fires in the first frame
    if (switches().test_rank_fault && !r->rank_inject_set) {
        const uint32_t one = 1u;
        GS_HIP(hipMemcpyAsync(&fs->rank_inject, &one, sizeof(one), hipMemcpyHostToDevice, F.st));
        GS_HIP(hipStreamSynchronize(F.st));      // `one` lives on this stack frame
        r->rank_inject_set = true;
    }
    F.sort.dev = r->dev;
    F.sort.st = F.st;
    F.sort.ghist = &r->ghist;
    F.sort.digit_totals = &r->digit_totals;
    F.sort.launches = &r->launches;
    // read ONCE per frame: every scatter of the frame ranks the same way, whatever another renderer's thread does
    F.sort.fast_rank = r->dev->lds_atomic_ordered.load();
    F.sort.rank_fault = F.sort.fast_rank ? &fs->rank_fault : nullptr;
    return GS_OK;
}

// The blend launch of one round (0: the frame's only one).
static gs_status stage_blend(Frame &F, uint32_t round) {
    gs_renderer *r = F.r;
    if (!F.nums.band_tiles) return GS_OK;
    const int groups = gsp::plan_blend_groups(switches(), round);
    const uint32_t mode = F.mode;
    typedef void (*blend_fn)(uint32_t *, const uint32_t *, const uint32_t *, gs::FrameConsts, float4 *,
                             const gs::FrameState *, gs::TileKeys);
    static const blend_fn tbl[3][4] = {
        {gs::k_blend<0>, gs::k_blend_grouped<0, 2>, gs::k_blend_grouped<0, 4>, gs::k_blend_grouped<0, 8>},
        {gs::k_blend<1>, gs::k_blend_grouped<1, 2>, gs::k_blend_grouped<1, 4>, gs::k_blend_grouped<1, 8>},
        {gs::k_blend<2>, gs::k_blend_grouped<2, 2>, gs::k_blend_grouped<2, 4>, gs::k_blend_grouped<2, 8>}};
    static const blend_fn tbl_rounds[3][3] = {
        {gs::k_blend_grouped<0, 2, true>, gs::k_blend_grouped<0, 4, true>, gs::k_blend_grouped<0, 8, true>},
        {gs::k_blend_grouped<1, 2, true>, gs::k_blend_grouped<1, 4, true>, gs::k_blend_grouped<1, 8, true>},
        {gs::k_blend_grouped<2, 2, true>, gs::k_blend_grouped<2, 4, true>, gs::k_blend_grouped<2, 8, true>}};
    // column of the grouped tables: 2 -> 8x8 blocks, 8 -> 4x4 blocks, anything else -> 8x4 blocks (an aux frame: also for 1)
    const int gcol = groups == 2 ? 0 : groups == 8 ? 2 : 1;
    if (round != 0u && groups == 1) return gs_fail(GS_ERR_INVALID_ARGUMENT, round, 0, 0, "two-round frames need the grouped blend");
    F.tile_keys.round = round;
    F.tile_keys.free_min_live = gsp::plan_blend_free_min_live(switches(), gs::BLEND_FREE_MIN_LIVE);
    if (F.contrib) {
        // the accumulation rides in the grouped blend of the frame's only round (G = 4 where the plain frame would take k_blend)
        typedef void (*contrib_fn)(uint32_t *, const uint32_t *, const uint32_t *, gs::FrameConsts, float4 *,
                                   const gs::FrameState *, gs::TileKeys, gs::ContribIO);
        static const contrib_fn tbl_contrib[3][3] = {
            {gs::k_blend_grouped<0, 2, false, false>, gs::k_blend_grouped<0, 4, false, false>, gs::k_blend_grouped<0, 8, false, false>},
            {gs::k_blend_grouped<1, 2, false, false>, gs::k_blend_grouped<1, 4, false, false>, gs::k_blend_grouped<1, 8, false, false>},
            {gs::k_blend_grouped<2, 2, false, false>, gs::k_blend_grouped<2, 4, false, false>, gs::k_blend_grouped<2, 8, false, false>}};
        if (round != 0u || F.aux) return gs_fail(GS_ERR_INVALID_ARGUMENT, round, 0, 0, "contribution frames take one round and no planes");
        gs::ContribIO cio;
        cio.rec = (uint4 *)F.contrib->ptr;
        cio.block_list = r->list_mode ? (const uint32_t *)r->block_list.ptr : nullptr;
        cio.order = r->last_order ? (const uint32_t *)r->last_order->ptr : nullptr;
        hipLaunchKernelGGL(tbl_contrib[mode][gcol], dim3(F.nums.band_tiles), dim3(gs::BLEND_THREADS), 0, F.st,
                           (uint32_t *)r->zero_region.ptr, (const uint32_t *)r->tvals[r->tsorted_side].ptr,
                           (const uint32_t *)r->recs.ptr, F.fc, (float4 *)F.rgba, (const gs::FrameState *)r->state.ptr, F.tile_keys,
                           cio);
    } else if (F.aux) {
        // the depth / pick planes ride in the grouped blend (G = 4 where the plain frame would take k_blend)
        typedef void (*aux_fn)(uint32_t *, const uint32_t *, const uint32_t *, gs::FrameConsts, float4 *,
                               const gs::FrameState *, gs::TileKeys, gs::AuxIO);
        static const aux_fn tbl_aux[2][3][3] = {
            {{gs::k_blend_grouped<0, 2, false, true>, gs::k_blend_grouped<0, 4, false, true>, gs::k_blend_grouped<0, 8, false, true>},
             {gs::k_blend_grouped<1, 2, false, true>, gs::k_blend_grouped<1, 4, false, true>, gs::k_blend_grouped<1, 8, false, true>},
             {gs::k_blend_grouped<2, 2, false, true>, gs::k_blend_grouped<2, 4, false, true>, gs::k_blend_grouped<2, 8, false, true>}},
            {{gs::k_blend_grouped<0, 2, true, true>, gs::k_blend_grouped<0, 4, true, true>, gs::k_blend_grouped<0, 8, true, true>},
             {gs::k_blend_grouped<1, 2, true, true>, gs::k_blend_grouped<1, 4, true, true>, gs::k_blend_grouped<1, 8, true, true>},
             {gs::k_blend_grouped<2, 2, true, true>, gs::k_blend_grouped<2, 4, true, true>, gs::k_blend_grouped<2, 8, true, true>}}};
        gs::AuxIO aio;
        aio.depth = F.aux->depth;
        aio.pick = F.aux->pick;
        aio.tcut = 1.0f - F.aux->pick_threshold;
        aio.key_bias = r->key_bias;
        aio.depth_keys = (const uint32_t *)r->depth.ptr;
        aio.block_list = r->list_mode ? (const uint32_t *)r->block_list.ptr : nullptr;
        aio.order = r->last_order ? (const uint32_t *)r->last_order->ptr : nullptr;
        hipLaunchKernelGGL(tbl_aux[round != 0u ? 1 : 0][mode][gcol], dim3(F.nums.band_tiles), dim3(gs::BLEND_THREADS), 0, F.st,
                           (uint32_t *)r->zero_region.ptr, (const uint32_t *)r->tvals[r->tsorted_side].ptr,
                           (const uint32_t *)r->recs.ptr, F.fc, (float4 *)F.rgba, (const gs::FrameState *)r->state.ptr, F.tile_keys,
                           aio);
    } else {
        const blend_fn blend = round != 0u ? tbl_rounds[mode][gcol] : tbl[mode][groups == 1 ? 0 : 1 + gcol];
        hipLaunchKernelGGL(blend, dim3(F.nums.band_tiles), dim3(gs::BLEND_THREADS), 0, F.st,
                           (uint32_t *)r->zero_region.ptr, (const uint32_t *)r->tvals[r->tsorted_side].ptr,
                           (const uint32_t *)r->recs.ptr, F.fc, (float4 *)F.rgba, (const gs::FrameState *)r->state.ptr, F.tile_keys);
    }
    GS_HIP(hipGetLastError());
    r->launches++;
    return GS_OK;
}

// n == 0: nothing to project: clear the ranges, blend the background
static gs_status stage_empty_frame(Frame &F) {
    gs_renderer *r = F.r;
    GS_TRY(dev_reserve(r->zero_region, (size_t)F.num_tiles * 8));
    GS_HIP(hipMemsetAsync(r->zero_region.ptr, 0, (size_t)F.num_tiles * 8, F.st));
    GS_TRY(reserve_pairs(r, 1, F.nums.wide));
    hipLaunchKernelGGL(gs::k_publish_result, dim3(1), dim3(64), 0, F.st, F.result, F.state, F.gen, r->flags_target);
    GS_HIP(hipGetLastError());
    r->launches++;
    for (int i : {ST_SCAN, ST_DSORT, ST_EXPAND, ST_TSORT, ST_RANGES}) F.marks.mark(i);
    r->sort_passes = 0;
    r->dsorted_side = r->tsorted_side = 0;
    return GS_OK;
}

// Block list (k_block_cull, see gsp::plan_use_list): the surviving blocks, handed to the preprocess kernel through `po`
static gs_status stage_block_cull(Frame &F, gs::PreOut &po) {
    gs_renderer *r = F.r;
    const uint32_t gen = F.gen, nchunks = F.nchunks;
    const uint32_t groups = (nchunks + 255u) / 256u;
    GS_TRY(dev_reserve(r->block_list, (size_t)nchunks * 4));
    GS_TRY(dev_reserve(r->cull_status, (size_t)groups * 4));
    // Tag of this frame's status words: 22 bits of the generation.  A word must never hold this tag
    // before its group publishes: consecutive list frames over the same groups overwrite every word
    // with the previous tag; in every other case (first use, a gap of frames without the list, another
    // group count) the words are cleared first, and the tag 0 is skipped.
    const uint32_t tag = (gen & 0x3fffffu) ? (gen & 0x3fffffu) : 0x3fffffu;
    if (r->cull_last_gen + 1u != gen || r->cull_last_groups != groups || (gen & 0x3fffffu) <= 1u)
        GS_HIP(hipMemsetAsync(r->cull_status.ptr, 0, (size_t)groups * 4, F.st));
    r->cull_last_gen = gen;
    r->cull_last_groups = groups;
    if (F.sel.block_hidden)
        hipLaunchKernelGGL(gs::k_block_cull<const uint32_t *>, dim3(groups), dim3(256), 0, F.st, (const float *)F.g->block_bounds.ptr, nchunks,
                           F.fc, (uint32_t *)r->block_list.ptr, F.state, (uint32_t *)r->cull_status.ptr, tag, groups, F.sel.block_hidden);
    else
        hipLaunchKernelGGL(gs::k_block_cull<>, dim3(groups), dim3(256), 0, F.st, (const float *)F.g->block_bounds.ptr, nchunks, F.fc,
                           (uint32_t *)r->block_list.ptr, F.state, (uint32_t *)r->cull_status.ptr, tag, groups);
    GS_HIP(hipGetLastError());
    r->launches++;
    po.block_list = (const uint32_t *)r->block_list.ptr;
    po.block_count = &F.state->list_blocks;
    r->list_mode = true;
    return GS_OK;
}

// First frame of this shape: measure D before sizing the pair buffers (the only blocking
// step; steady-state frames take the capacity from the history instead)
static gs_status stage_sizing(Frame &F) {
    gs_renderer *r = F.r;
    gs::ScanJob jt{(const uint32_t *)r->chunk_tiles.ptr, (uint32_t *)r->scan_tmp.ptr, r->host_counters.ptr, F.nchunks,
                   r->list_mode ? &F.state->list_blocks : nullptr};
    hipLaunchKernelGGL(gs::k_scan_chunks, dim3(1), dim3(1024), 0, F.st, jt, jt);
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(F.st));
    const uint32_t d = r->host_counters.ptr[0];
    if (d == 0xffffffffu) {
        r->shape = FrameShape();
        return gs_fail(GS_ERR_PAIR_OVERFLOW, F.n, 0, 0,
                    "the frame needs more than 2^32 (tile, Gaussian) pairs; pair indices are 32-bit");
    }
    r->rounds_fb.full_pairs = d;              // (the visible count it belongs to comes with the frame's report)
    r->rounds_fb.full_pairs_v = 0;
    const uint64_t cap = gsp::capacity_for(d) > F.plan.want_capacity ? gsp::capacity_for(d) : F.plan.want_capacity;
    return reserve_pairs(r, cap, F.nums.wide);
}

// Selection frames: the renderer's mirror-slot-ordered copies of the hide / tint masks.  A copy is
// gathered again (k_selection_to_slots, one launch) only when its selection was modified since (every mutating call gives
// the selection a new generation) or it was gathered through another buffer or another build of the mirror order.
static gs_status stage_selection(Frame &F) {
    gs_renderer *r = F.r;
    const gs_selection *sels[2] = {F.fs->hide, F.fs->tint};
    const uint64_t *slots[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++) {
        if (!sels[k]) continue;
        gs_renderer::SlotMaskKey key;
        key.generation = sels[k]->generation;
        key.buffer = F.g->uid;
        key.order_epoch = F.g->order_epoch;
        key.n = F.n;
        GS_TRY(dev_reserve(r->sel_slots[k], F.nslots / 8));
        if (k == 0) GS_TRY(dev_reserve(r->sel_block_hidden, F.nc * 4));
        if (!(key == r->sel_key[k])) {
            r->sel_key[k] = gs_renderer::SlotMaskKey();
            hipLaunchKernelGGL(gs::k_selection_to_slots, dim3(F.nchunks), dim3(gs::PP_THREADS), 0, F.st, sels[k]->bits(),
                               F.g->order ? (const uint32_t *)F.g->order->ptr : nullptr, F.n, (uint64_t *)r->sel_slots[k].ptr,
                               k == 0 ? (uint32_t *)r->sel_block_hidden.ptr : nullptr);
            GS_HIP(hipGetLastError());
            r->launches++;
            r->sel_key[k] = key;
        }
        slots[k] = (const uint64_t *)r->sel_slots[k].ptr;
    }
    F.sel.hide = slots[0];
    F.sel.tint = slots[1];
    F.sel.block_hidden = slots[0] ? (const uint32_t *)r->sel_block_hidden.ptr : nullptr;
    const float a = sels[1] ? F.fs->tint_rgba[3] : 0.0f;
    F.sel.tint_keep = 1.0f - a;
    for (int c = 0; c < 3; c++) F.sel.tint_add[c] = sels[1] ? a * F.fs->tint_rgba[c] : 0.0f;
    return GS_OK;
}

// the zero region and the pair buffers, the block list, the preprocess kernel and — a shape's first frame — the sizing pass
static gs_status stage_preprocess(Frame &F) {
    gs_renderer *r = F.r;
    gs_gaussians_buffer *g = F.g;
    const gsp::FramePlan &plan = F.plan;
    const bool sizing = F.nums.sizing, wide = F.nums.wide;
    // the clear job of this frame, spread over the preprocess grid: tile ranges + the
    // expansion's super-chunk sums
    const size_t ranges_words = (size_t)F.num_tiles * 2;                                   // even: keeps the u64 sums aligned
    const size_t esb_words = 2 * ((size_t)F.exp_grid / gs::EXP_SB + 1);                    // u64 super-chunk sums of the expansion
    const size_t done_words = ((size_t)F.num_tiles + 31) / 32 + 1;                        // two-round frames: finished tiles
    // (a two-round frame needs the sums of both rounds and the bits; cleared in every frame: ~1 KB)
    const size_t zero_words = ranges_words + 2 * esb_words + 2 * done_words;
    GS_TRY(dev_reserve(r->zero_region, zero_words * 4));
    F.zero = (uint32_t *)r->zero_region.ptr;
    F.esb = F.zero + ranges_words;
    F.esb2 = F.esb + esb_words;
    F.done_bits = F.esb2 + esb_words;
    F.open_bits = F.done_bits + done_words;

    if (!sizing && plan.want_capacity > r->pair_capacity) GS_TRY(reserve_pairs(r, plan.want_capacity, wide));
    if (!sizing) GS_TRY(reserve_pairs(r, r->pair_capacity, wide));   // key width may have changed

    F.fc.mask_culled_records = plan.mask_culled_records;
    F.fc.nt_loads = plan.nt_loads;
    if (!plan.block_cull || !g->block_bounds.ptr) F.fc.cull_gain = 0.0f;

    gs::PreOut po;
    po.recs = (uint32_t *)r->recs.ptr;
    po.rect = (uint2 *)r->rect.ptr;
    po.depth = (uint32_t *)r->depth.ptr;
    po.chunk_tiles = (uint32_t *)r->chunk_tiles.ptr;
    po.chunk_vis = (uint32_t *)r->chunk_vis.ptr;
    po.zero_ptr = F.zero;
    po.zero_words = (uint32_t)zero_words;
    po.key_bias = F.near_bits;
    po.block_bounds = (const float *)g->block_bounds.ptr;
    po.chunk_hist = (uint32_t *)r->chunk_hist.ptr;
    const bool top_hist = plan.depth_msd || plan.partition;      // the chunk rows count the TOP 10 bits (else the LSD sort's first digit)
    po.digit_mask = top_hist ? (1u << gs::MSD_TOP_BITS) - 1u : first_digit_mask(F.nums.dbits, depth_radix_bits(F.nums.dbits));
    po.digit_shift = top_hist ? gsp::msd_low_bits(F.nums, k_policy_params) : 0u;
    po.hist_words = top_hist ? (1u << gs::MSD_TOP_BITS) / 2u : (uint32_t)gs::PP_THREADS;
    po.block_list = nullptr;
    po.block_count = nullptr;
    r->list_mode = false;
    if (F.fc.cull_gain > 0.0f && plan.use_list) GS_TRY(stage_block_cull(F, po));
    const int nt = F.fc.nt_loads ? 1 : 0;
    if (F.fs)
        hipLaunchKernelGGL((plan.banded ? k_tbl_preprocess_banded_sel[nt][switches().pre_serial ? 0 : 1] : k_tbl_preprocess_sel[nt])[g->sh][g->cov],
                           dim3(F.nchunks), dim3(gs::PP_THREADS), 0, F.st, (const uint4 *)g->planar.ptr, F.n, F.fc, po, F.sel);
    else
        hipLaunchKernelGGL((plan.banded ? k_tbl_preprocess_banded[nt][switches().pre_serial ? 0 : 1] : k_tbl_preprocess[nt])[g->sh][g->cov], dim3(F.nchunks),
                           dim3(gs::PP_THREADS), 0, F.st, (const uint4 *)g->planar.ptr, F.n, F.fc, po);
    GS_HIP(hipGetLastError());
    r->launches++;
    F.marks.mark(ST_SCAN);
    if (sizing) GS_TRY(stage_sizing(F));
    if (!(r->shape == F.shape)) r->shape_epoch++;
    r->shape = F.shape;
    return GS_OK;
}

// ---- depth sort of the visible Gaussians; its first pass reads the dense per-slot keys and
//      compacts (count V stays on the device, grids from N) ----
// pred: which Gaussians the compacting first pass takes (all visible ones; or one side of a partitioned frame's
// threshold); their count goes to *visible_out.  Returns the side of dvals that holds the order; adds its passes.
static gs_status stage_depth_sort(Frame &F, const gs::CompactPred &pred, uint32_t *visible_out, const uint32_t *dense_dev, int &dside,
                                  uint32_t &dpasses) {
    gs_renderer *r = F.r;
    const uint32_t n = F.n, dbits = F.nums.dbits;
    void *k2[2] = {r->dkeys[0].ptr, r->dkeys[1].ptr};
    void *v2[2] = {r->dvals[0].ptr, r->dvals[1].ptr};
    SortCompact cp;
    cp.dense_keys = (const uint32_t *)r->depth.ptr;
    cp.chunk_vis = (const uint32_t *)r->chunk_vis.ptr;
    cp.visible_out = visible_out;
    cp.dense_count = n;
    // list frame: only the surviving blocks' slots; round 2 of a partitioned frame: none when the gate found nothing left
    cp.dense_count_dev = dense_dev ? dense_dev : r->list_mode ? &F.state->list_slots : nullptr;
    // (a partitioned frame's chunk rows count the top digit of ALL visible keys: its passes count their own)
    cp.chunk_hist = pred.tau_dev ? nullptr : (const uint32_t *)r->chunk_hist.ptr;
    cp.pred = pred;
    cp.bucket_max = &F.state->depth_bucket_max;
    const gs::SortCount dc{n, visible_out};
    uint32_t passes = 0;
    if (F.plan.depth_msd) {
        // scratch of the bucket kernel's chunked path: the LSD sort's side 0 keys and the (not yet written)
        // depth-ordered rects — the dense keys themselves stay intact for the parity taps
        const uint32_t top_range = ((F.far_bits - F.near_bits) >> gsp::msd_low_bits(F.nums, k_policy_params)) + 1u;
        GS_TRY(with_depth_items(n, [&](auto items) {
            return run_depth_msd_items<decltype(items)::value>(F.sort, r, cp, dbits, top_range, r->dkeys[0].ptr, r->sorted_rect.ptr, passes);
        }));
        dside = 0;
    } else if (depth_radix_bits(dbits) == (uint32_t)gs::RADIX_BITS_MAX)
        GS_TRY((run_sort_rb<uint32_t, gs::RADIX_BITS_MAX>(F.sort, k2, v2, dc, dbits, &cp, dside, passes)));
    else
        GS_TRY((run_sort_rb<uint32_t, gs::RADIX_BITS>(F.sort, k2, v2, dc, dbits, &cp, dside, passes)));
    dpasses += passes;
    return GS_OK;
}

// a partitioned frame: the totals of the top digit (the histogram half of the MSD-first sort's pass), then the cut;
// pred1 = round 1: the keys in front of the threshold
static gs_status stage_round_threshold(Frame &F, gs::CompactPred &pred1) {
    gs_renderer *r = F.r;
    const uint32_t *dense_dev = r->list_mode ? &F.state->list_slots : nullptr;
    GS_TRY(with_depth_items(F.n, [&](auto items) { return run_top_digit_totals<decltype(items)::value>(r, F.st, F.n, dense_dev); }));
    gs::ThresholdIO ti;
    ti.totals = (const uint32_t *)r->digit_totals.ptr;
    ti.state = F.state;
    ti.target = F.plan.round_k;
    ti.low_bits = gsp::msd_low_bits(F.nums, k_policy_params);
    hipLaunchKernelGGL(gs::k_round_threshold, dim3(1), dim3(512), 0, F.st, ti);
    GS_HIP(hipGetLastError());
    r->launches += 3;
    GS_TRY(dev_reserve(r->keep_bits, F.nslots / 8 + 64));
    pred1.tau_dev = &F.state->depth_tau;
    pred1.keep_bits = (const uint32_t *)r->keep_bits.ptr;      // (side 0 loads and ignores them)
    pred1.side = 0u;
    return GS_OK;
}

// the tile ranges of one round's sorted pairs (gsp::plan_ranges)
static gs_status stage_tile_ranges(Frame &F, uint32_t round, bool tile_msd, int tside, gs::SortCount tc) {
    gs_renderer *r = F.r;
    const uint32_t capacity = F.plan.capacity, num_tiles = F.num_tiles;
    const bool wide = F.nums.wide;
    switch (gsp::plan_ranges(F.nums, switches(), capacity, tile_msd, round)) {
    case gsp::RANGES_NONE: break;
    case gsp::RANGES_IN_BLEND:
        F.tile_keys.keys = r->tkeys[tside].ptr;
        F.tile_keys.count_dev = &F.state->pairs;
        F.tile_keys.count_bound = capacity;
        F.tile_keys.wide = wide ? 1u : 0u;
        break;
    case gsp::RANGES_SEARCH:
        if (wide)
            hipLaunchKernelGGL(gs::k_tile_ranges_search<uint32_t>, dim3((num_tiles + 3u) / 4u), dim3(256), 0, F.st,
                               (const uint32_t *)r->tkeys[tside].ptr, tc, F.zero, num_tiles);
        else
            hipLaunchKernelGGL(gs::k_tile_ranges_search<uint16_t>, dim3((num_tiles + 3u) / 4u), dim3(256), 0, F.st,
                               (const uint16_t *)r->tkeys[tside].ptr, tc, F.zero, num_tiles);
        GS_HIP(hipGetLastError());
        r->launches++;
        break;
    case gsp::RANGES_PASS:
        if (wide)
            hipLaunchKernelGGL(gs::k_tile_ranges<uint32_t>, dim3((uint32_t)(((uint64_t)capacity + 1023) / 1024)), dim3(256), 0, F.st,
                               (const uint32_t *)r->tkeys[tside].ptr, tc, F.zero);
        else
            hipLaunchKernelGGL(gs::k_tile_ranges<uint16_t>, dim3((uint32_t)(((uint64_t)capacity + 2047) / 2048)), dim3(256), 0, F.st,
                               (const uint16_t *)r->tkeys[tside].ptr, tc, F.zero);
        GS_HIP(hipGetLastError());
        r->launches++;
        break;
    }
    return GS_OK;
}

// ---- pairs in depth order, tile sort, tile ranges: once per round ----
// round: 0 the frame's only one; 1: the nearest `limit` Gaussians of the depth order; 2: the survivors of
// k_round2_write (order_r2).  Returns the side of tkeys / tvals that holds the sorted pairs and the tile sort's passes.
static gs_status stage_pairs_round(Frame &F, uint32_t round, const uint32_t *order, const uint32_t *count_dev, uint32_t limit, uint32_t *esb_r,
                                   int &tside, uint32_t &tpasses) {
    gs_renderer *r = F.r;
    hipStream_t st = F.st;
    const uint32_t capacity = F.plan.capacity;
    if (round <= 1u) F.marks.mark(ST_EXPAND);
    gs::ExpandIO eo;
    eo.order = order;
    eo.rect = (const uint2 *)r->rect.ptr;
    eo.sorted_rect = (uint2 *)r->sorted_rect.ptr;
    eo.count_dev = count_dev;
    eo.limit = limit;
    eo.round = round;
    eo.sums = (uint32_t *)r->exp_sums.ptr;
    eo.sb_sums = (unsigned long long *)esb_r;
    eo.tvals = (uint32_t *)r->tvals[0].ptr;
    eo.state = F.state;
    eo.result = F.result;
    eo.capacity = capacity;
    eo.tiles_x = F.fc.tiles_x;
    eo.gen = F.gen;
    eo.sb_bound = F.exp_grid / gs::EXP_SB + 1;
    eo.rect32 = F.fc.rect32;
    eo.flags_dev = r->flags_target;
    eo.wt_stores = r->wt_pairs ? 1u : 0u;
    const bool cursor_kernel = gsp::plan_cursor_kernel(switches(), eo.sb_bound);
    eo.cursors = cursor_kernel ? (gs::PairCursorRec *)r->cursors.ptr : nullptr;
    // XCD-aware span order of the gather: XCD x takes C consecutive spans of every group of 8 C, so that its L2
    // serves part of the gather (neighbours in depth order are often neighbours in the mirror).  Same-box sweep
    // (gpurun_out/r04q/ab*.log): C = 0 / 16 / 64 / 256 / 1024 -> 58.3 / 53.3 / 49.1 / 54.3 / 90.6 us at 10 M, 261 / 258 /
    // 231 / 228 / 293 us at 50 M, 12.0 / - / 10.5 / 21 / 26 us at 1 M.  GS3D_EXPAND_XCD=<C> forces, 0 = dispatch order.
    const int exp_xcd = switches().expand_xcd;
    uint32_t count_grid = (F.exp_grid + gs::EXP_COUNT_CHUNKS - 1) / gs::EXP_COUNT_CHUNKS;
    eo.xcd_chunk = 0;
    if (exp_xcd > 0 && count_grid >= 256u) {
        eo.xcd_chunk = (uint32_t)exp_xcd;
        count_grid = 8u * eo.xcd_chunk * ((count_grid + 8u * eo.xcd_chunk - 1u) / (8u * eo.xcd_chunk));
    }
    if (eo.rect32)
        hipLaunchKernelGGL(gs::k_expand_count<true>, dim3(count_grid), dim3(gs::EXP_CHUNK), 0, st, eo);
    else
        hipLaunchKernelGGL(gs::k_expand_count<false>, dim3(count_grid), dim3(gs::EXP_CHUNK), 0, st, eo);
    r->launches++;
    if (cursor_kernel) {
        hipLaunchKernelGGL(gs::k_pairs_cursors, dim3(eo.sb_bound), dim3(gs::EXP_SB), 0, st, eo);
        r->launches++;
    }
    GS_HIP(hipGetLastError());
    if (round <= 1u) F.marks.mark(ST_TSORT);

    // ---- stable sort on the tile id alone (pairs are generated in depth order by its first pass) ----
    tside = 0;
    const gs::SortCount tc{capacity, &F.state->pairs};
    const bool tile_msd = round == 0u && F.plan.tile_msd;      // (gsp::plan_tile_msd)
    r->tile_msd = tile_msd;
    if (tile_msd) {
        if (F.nums.tile_bits > (uint32_t)gs::MSD_TOP_BITS + 6u) return gs_fail(GS_ERR_INVALID_ARGUMENT, F.nums.tile_bits, 0, 0, "tile id bits");
        GS_TRY((run_tile_msd_items<gs::SortCfg<uint16_t>::ITEMS>(F.sort, r, eo, tc, F.nums.tile_bits, F.num_tiles, F.zero,
                                                                  &F.state->tile_bucket_max, tpasses)));
        tside = 0;
    } else {
        // (a frame whose tile sort is LSD reports no bucket size: the next result must not carry a stale one)
        if (r->state_tile_bmax_dirty) GS_HIP(hipMemsetAsync(&F.state->tile_bucket_max, 0, sizeof(uint32_t), st));
        void *k2[2] = {r->tkeys[0].ptr, r->tkeys[1].ptr};
        void *v2[2] = {r->tvals[0].ptr, r->tvals[1].ptr};
        if (F.nums.wide)
            GS_TRY((run_sort_rb<uint32_t, gs::RADIX_BITS>(F.sort, k2, v2, tc, F.nums.tile_bits, nullptr, tside, tpasses, &eo)));
        else
            GS_TRY((run_sort_rb<uint16_t, gs::RADIX_BITS>(F.sort, k2, v2, tc, F.nums.tile_bits, nullptr, tside, tpasses, &eo)));
    }
    r->state_tile_bmax_dirty = tile_msd;
    if (round <= 1u) F.marks.mark(ST_RANGES);
    GS_TRY(stage_tile_ranges(F, round, tile_msd, tside, tc));
    r->tsorted_side = tside;          // (stage_blend reads the pairs of THIS round: round 1's blend runs before the frame ends)
    return GS_OK;
}

// Between the rounds: what round 1's blend left open decides which of the remaining Gaussians round 2 renders (the gate,
// the box table, one bit per slot); then their depth order — a partitioned frame sorts them (the side of dvals comes
// back in dside), the others are compacted out of the full order into order_r2.
static gs_status stage_round2_select(Frame &F, int &dside, uint32_t &dpasses) {
    gs_renderer *r = F.r;
    hipStream_t st = F.st;
    const uint32_t n = F.n, num_tiles = F.num_tiles, round_k = F.plan.round_k;
    const bool partition = F.plan.partition;
    if (!partition) GS_TRY(dev_reserve(r->order_r2, (F.nn + 1024) * 4));      // (its largest size at once; padded like the sorts' values)
    gs::Round2IO ro;
    ro.order = (const uint32_t *)r->dvals[dside].ptr + round_k;
    ro.rect = (const uint2 *)r->rect.ptr;
    ro.done = F.done_bits;
    ro.open = F.open_bits;
    ro.order_out = (uint32_t *)r->order_r2.ptr;
    ro.state = F.state;
    ro.first = round_k;
    ro.groups = (n - round_k + gs::R2_GROUP - 1u) / gs::R2_GROUP;
    ro.tiles_x = F.fc.tiles_x;
    ro.num_tiles = num_tiles;
    // (per-slot arrays cover whole chunks: nslots; a list frame's live in list space, bounded by the same)
    ro.slots = (uint32_t)F.nslots;
    GS_TRY(dev_reserve(r->keep_bits, F.nslots / 8 + 64));
    ro.keep_bits = (uint32_t *)r->keep_bits.ptr;
    const uint32_t bits_grid = (uint32_t)((F.nslots + 256u * gs::R2_SLOT_ITEMS - 1u) / (256u * gs::R2_SLOT_ITEMS));
    {
        typedef void (*bits_fn)(gs::Round2IO);
        static const bits_fn tbl[2][2] = {{gs::k_round2_slot_bits<false, false>, gs::k_round2_slot_bits<false, true>},
                                          {gs::k_round2_slot_bits<true, false>, gs::k_round2_slot_bits<true, true>}};
        GS_TRY(dev_reserve(r->box_table, ((size_t)num_tiles + 8) * 2));
        ro.box_table = (const uint16_t *)r->box_table.ptr;
        hipLaunchKernelGGL(gs::k_round2_gate, dim3(1), dim3(256), 0, st, ro, F.nums.band_tiles, n,
                           r->list_mode ? (const uint32_t *)&F.state->list_slots : (const uint32_t *)nullptr);
        hipLaunchKernelGGL(gs::k_round2_box_table, dim3((num_tiles + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)F.done_bits,
                           (uint16_t *)r->box_table.ptr, F.fc.tiles_x, F.fc.tiles_y, (const gs::FrameState *)F.state);
        r->launches += 2;
        const bool lds = num_tiles <= gs::R2_LDS_TILES;
        const size_t lds_bytes = lds ? ((size_t)num_tiles + 7) / 8 * 16 : 0;
        const uint32_t persistent = bits_grid < 1024u ? bits_grid : 1024u;      // (4 / 2 workgroups per CU at 1080p / 4K)
        hipLaunchKernelGGL(tbl[F.fc.rect32 ? 1 : 0][lds ? 1 : 0], dim3(persistent), dim3(256), lds_bytes, st, ro);
    }
    GS_HIP(hipGetLastError());
    r->launches++;
    if (partition) {
        // the depth sort of what is left: keys behind the threshold whose slot bit is set
        gs::CompactPred pred2;
        pred2.tau_dev = &F.state->depth_tau;
        pred2.keep_bits = (const uint32_t *)r->keep_bits.ptr;
        pred2.side = 1u;
        GS_TRY(stage_depth_sort(F, pred2, &F.state->round2_visible, &F.state->round2_dense, dside, dpasses));
    } else {
        GS_TRY(dev_reserve(r->r2_scan, ((size_t)F.nn / gs::R2_GROUP + 1) * (2 * 4 + 32 * 8) + 64));      // (its largest size: never regrown under frames in flight)
        ro.masks = (unsigned long long *)r->r2_scan.ptr;
        ro.counts = (uint32_t *)(ro.masks + (size_t)ro.groups * 32);
        ro.offsets = ro.counts + ro.groups;
        hipLaunchKernelGGL(gs::k_round2_count, dim3(ro.groups), dim3(256), 0, st, ro);
        gs::ScanJob js{ro.counts, ro.offsets, &F.state->round2_visible, ro.groups, nullptr};
        hipLaunchKernelGGL(gs::k_scan_chunks, dim3(1), dim3(1024), 0, st, js, js);
        hipLaunchKernelGGL(gs::k_round2_write, dim3(ro.groups), dim3(256), 0, st, ro);
        r->launches += 3;
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// everything between the preprocess kernel and the frame's last blend: depth sort, then one round of pairs or two
static gs_status stage_sort_and_rounds(Frame &F) {
    gs_renderer *r = F.r;
    gs::FrameState *state = F.state;
    const gsp::FramePlan &plan = F.plan;
    int dside = 0, tside = 0;
    uint32_t dpasses = 0, tpasses = 0;
    gs::CompactPred pred1;
    if (plan.partition) GS_TRY(stage_round_threshold(F, pred1));
    GS_TRY(stage_depth_sort(F, pred1, plan.partition ? &state->round1_visible : &state->visible, nullptr, dside, dpasses));
    r->two_round = plan.two_round;
    r->round1 = plan.round_k;
    if (!plan.two_round) {
        GS_TRY(stage_pairs_round(F, 0u, (const uint32_t *)r->dvals[dside].ptr, &state->visible, 0xffffffffu, F.esb, tside, tpasses));
    } else {
        F.tile_keys.done = F.done_bits;
        F.tile_keys.open = F.open_bits;
        if (plan.partition)
            GS_TRY(stage_pairs_round(F, 1u, (const uint32_t *)r->dvals[dside].ptr, &state->round1_visible, 0xffffffffu, F.esb, tside, tpasses));
        else
            GS_TRY(stage_pairs_round(F, 1u, (const uint32_t *)r->dvals[dside].ptr, &state->visible, plan.round_k, F.esb, tside, tpasses));
        F.marks.mark(ST_BLEND);
        GS_TRY(stage_blend(F, 1u));
        GS_TRY(stage_round2_select(F, dside, dpasses));
        GS_TRY(stage_pairs_round(F, 2u, plan.partition ? (const uint32_t *)r->dvals[dside].ptr : (const uint32_t *)r->order_r2.ptr,
                                 &state->round2_visible, 0xffffffffu, F.esb2, tside, tpasses));
    }
    r->sort_passes = dpasses + tpasses;
    r->dsorted_side = dside;
    r->tsorted_side = tside;
    return GS_OK;
}

// Frames of one renderer share its scratch buffers and result blocks, so they must run one after
// the other.  On one stream that is stream order; a caller that moves the renderer to ANOTHER
// stream gets the same guarantee from the previous frame's end-of-frame event (a device-side wait,
// the host does not block).
// No event at the end of every frame (round 4: it cost ~4 us of a pipelined 1 M frame).  The event a stream change
// needs is recorded on the PREVIOUS stream when the change happens (everything enqueued there is in front of it),
// and the capacity history reads the self-validating result blocks (gen stored last, read first and last)
// without asking an event first.  GS3D_FRAME_EVENT=1 restores the per-frame event (and the query in front of
// every history read).
static gs_status take_over_stream(gs_renderer *r, hipStream_t st) {
    if (r->have_frame && (st != r->last_stream || r->last_stream_gone)) {
        // (a stream that has been destroyed since recorded the event on its way out: gs_stream_destroy; a new stream may
        // have received the old handle's value, hence the flag and not the comparison alone)
        if (!switches().frame_event && !r->last_stream_gone) {
            GS_HIP(hipEventRecord(r->done[r->gen & 1u], r->last_stream));
            r->done_valid[r->gen & 1u] = true;
        }
        if (r->done_valid[r->gen & 1u]) GS_HIP(hipStreamWaitEvent(st, r->done[r->gen & 1u], 0));
    }
    return GS_OK;
}

static gs_status check_frame_args(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *g, const gs_gaussian_transform_pod *gt,
                                  const gs_model_transform_pod *mt, const gs_camera *cam, float *rgba) {
    if (!r || !s || !g || !gt || !mt || !cam || !rgba)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (g->buf->dev != r->dev || s->dev != r->dev)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (cam->width == 0 || cam->height == 0 || cam->width > 65535u * 16u || cam->height > 65535u * 16u)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, cam->width, cam->height, 0, "bad image size");
    if ((uintptr_t)rgba & 15u)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(uintptr_t)rgba, 16, 0,
                    "the RGBA frame must be 16-byte aligned (pixels are stored as float4)");
    if (gt->flags[0] > GS_DISPLAY_POINT)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, gt->flags[0], 0, 0, "unknown GaussianDisplayMode %u", gt->flags[0]);
    if (!(cam->near_plane >= 0.0f))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the near plane must be >= 0 (depth keys are the bits of a positive float)");
    return GS_OK;
}

static gs_status render_frame(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *g, const gs_gaussian_transform_pod *gt,
                              const gs_model_transform_pod *mt, const gs_camera *cam, uint32_t band_ty0,
                              uint32_t band_ty1, float *rgba, const gs_aux_targets *aux, const gs_frame_selection *fs = nullptr,
                              gs_buffer *contrib = nullptr) {
    GS_TRY(check_frame_args(r, s, g, gt, mt, cam, rgba));
    if (contrib) GS_TRY(check_contrib_buffer(contrib, r->dev, gs_gaussians_buffer_len(g)));
    GS_TRY(use_device(r->dev));
    hipStream_t st = s->s;
    GS_TRY(collect_timing(r));
    GS_TRY(take_over_stream(r, st));
    Frame F{r, st, g, aux, rgba, fs, StageMarks{r, st, r->timing && r->ev_valid}};
    F.mode = gt->flags[0];
    F.contrib = contrib;
    gs::FrameConsts &fc = F.fc;
    make_frame_consts(gt, mt, cam, band_ty0, band_ty1, fc);
    const size_t n64 = gs_gaussians_buffer_len(g);
    gsp::FrameNums &nums = F.nums;
    nums.pod_bytes = (uint64_t)gs::pod_words(g->sh, g->cov) * 4u;
    // (make_frame_consts only records that the display mode allows rect version 4: gsp::plan_tile_masks decides)
    F.plan.tile_masks = gsp::plan_tile_masks(fc.tile_masks != 0u, n64, nums.pod_bytes, F.requests(), switches());
    fc.tile_masks = F.plan.tile_masks ? 1u : 0u;
    r->tile_masks = F.plan.tile_masks;
    r->wt_pairs = fc.wt_pairs != 0u;
    if (n64 > 0xfffffff0ull) return gs_fail(GS_ERR_INVALID_ARGUMENT, n64, 0, 0, "too many Gaussians");
    const uint32_t n = F.n = (uint32_t)n64;
    F.nchunks = (n + gs::PP_CHUNK - 1) / gs::PP_CHUNK;
    F.num_tiles = fc.tiles_x * fc.tiles_y;
    // one 256-Gaussian expansion chunk may touch at most 256 * num_tiles pairs: keep that inside 32 bits
    if ((uint64_t)fc.tiles_x * fc.tiles_y > (1ull << 22))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, cam->width, cam->height, 0, "more than 2^22 tiles");
    // tile rects are packed as 16-bit tile coordinates
    if (fc.tiles_x > 0xffffu || fc.tiles_y > 0xffffu)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, cam->width, cam->height, 0, "more than 65535 tiles along one axis");
    F.nn = n ? n : 1;
    F.nc = F.nchunks ? F.nchunks : 1;
    F.nslots = F.nc * (size_t)gs::PP_CHUNK;
    F.exp_grid = (n + gs::EXP_CHUNK - 1) / gs::EXP_CHUNK;   // V <= N

    F.hist = read_history(r);
    F.shape.n = n;
    F.shape.width = cam->width;
    F.shape.height = cam->height;
    F.shape.band0 = fc.band_ty0;
    F.shape.band1 = fc.band_ty1;

    F.marks.mark(ST_REPACK);
    GS_TRY(ensure_planar(g, st));
    if (r->last_order != g->order) {
        if (r->last_order) gs_buffer_release(r->last_order);
        r->last_order = g->order ? gs_buffer_retain(g->order) : nullptr;
    }
    F.marks.mark(ST_PRE);
    GS_TRY(reserve_frame_scratch(F));
    GS_TRY(arm_rank_watchdog(F));

    r->gen++;
    const uint32_t gen = F.gen = r->gen;
    // the rank watchdog's sample of this frame (GS3D_TEST_RANK_WATCH=<n> pins it: tests)
    F.sort.watch = switches().test_rank_watch_set ? switches().test_rank_watch : gen;
    DoneGuard done_guard{r, st, gen, switches().frame_event};
    F.state = (gs::FrameState *)r->state.ptr;
    F.result = &r->results.ptr[gen & 1u];
    r->n = n;
    r->tiles_x = fc.tiles_x;
    r->tiles_y = fc.tiles_y;
    r->rect32 = fc.rect32 != 0u;
    r->width = cam->width;
    r->height = cam->height;
    r->last_stream = st;
    r->last_stream_gone = false;
    r->have_frame = true;
    r->launches = 0;
    r->list_mode = false;
    r->two_round = false;

    // depth keys = bits of the (positive) view depth minus the bits of the near plane: every visible
    // depth lies in (near, far), so only bit_length(bits(far) - bits(near)) bits need sorting — a
    // bound the host knows without looking at the scene
    F.near_bits = float_bits(cam->near_plane > 0.0f ? cam->near_plane : 0.0f);
    F.far_bits = cam->far_plane > 0.0f ? float_bits(cam->far_plane) : 0u;
    r->key_bias = F.near_bits;

    // ---- the frame's plan (gs_policy.h): everything that is decided before the first launch ----
    nums.n = n;
    nums.gen = gen;
    nums.num_tiles = F.num_tiles;
    nums.tiles_y = fc.tiles_y;
    nums.band_rows = fc.band_ty1 - fc.band_ty0;
    nums.band_tiles = nums.band_rows * fc.tiles_x;
    nums.dbits = F.far_bits > F.near_bits ? bit_length(F.far_bits - F.near_bits) : 0u;
    nums.tile_bits = bit_length(F.num_tiles ? F.num_tiles - 1 : 0);
    nums.wide = F.num_tiles > 65536u;
    nums.sizing = n != 0 && (r->pair_capacity == 0 || !(F.shape == r->shape));
    nums.pair_capacity = r->pair_capacity;
    nums.has_sh = g->sh != GS_SH_NONE;
    nums.has_order = g->order != nullptr;
    gsp::plan_frame(F.hist, nums, F.requests(), switches(), k_policy_params, r->sort_fb, r->rounds_fb, F.plan);
    r->partitioned = F.plan.partition;

    if (n == 0) {
        GS_TRY(stage_empty_frame(F));
    } else {
        if (F.fs) GS_TRY(stage_selection(F));
        GS_TRY(stage_preprocess(F));
        // ... and what depends on the size of the pair buffers (the sizing pass may just have set it)
        gsp::plan_pairs(F.hist, nums, r->pair_capacity, F.requests(), switches(), k_policy_params, r->sort_fb, r->rounds_fb, F.plan);
        r->frame_capacity = F.plan.capacity;
        F.marks.mark(ST_DSORT);
        GS_TRY(stage_sort_and_rounds(F));
    }
    if (!r->two_round) F.marks.mark(ST_BLEND);
    GS_TRY(stage_blend(F, r->two_round ? 2u : 0u));
    F.marks.mark(ST_FRAME);
    if (F.marks.timing) {
        (void)hipEventRecord(r->ev[ST_COUNT], st);
        r->ev_pending = true;
    }
    return GS_OK;   // done_guard records the end-of-frame event
}

extern "C" gs_status gs_render_frame(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *g,
                                     const gs_gaussian_transform_pod *gt,
                                     const gs_model_transform_pod *mt, const gs_camera *cam,
                                     uint32_t band_ty0, uint32_t band_ty1, float *rgba) {
    return render_frame(r, s, g, gt, mt, cam, band_ty0, band_ty1, rgba, nullptr);
}

// gs_aux_targets as the frame takes it: null when it names no plane
static gs_status check_aux(const gs_aux_targets *&aux) {
    if (aux) {
        if (aux->reserved != 0u) return gs_fail(GS_ERR_INVALID_ARGUMENT, aux->reserved, 0, 0, "gs_aux_targets.reserved must be 0");
        if (!aux->depth && !aux->pick) {
            aux = nullptr;      // no planes: the plain frame, whatever the threshold says
        } else {
            // tcut = 1 - t in f32 must lie in (0, 1): a t below 2^-25 rounds it to 1, which no step can cross
            const float tcut = 1.0f - aux->pick_threshold;
            if (!(aux->pick_threshold > 0.0f && aux->pick_threshold < 1.0f) || !(tcut < 1.0f))
                return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0,
                            "the pick threshold must lie in (0, 1), and 1 - threshold must be below 1 in f32 (threshold > 2^-25)");
            if (((uintptr_t)aux->depth & 3u) || ((uintptr_t)aux->pick & 3u))
                return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(uintptr_t)aux->depth, (uint64_t)(uintptr_t)aux->pick, 4,
                            "the depth and pick planes must be 4-byte aligned");
        }
    }
    return GS_OK;
}

extern "C" gs_status gs_render_frame_aux(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *g,
                                         const gs_gaussian_transform_pod *gt,
                                         const gs_model_transform_pod *mt, const gs_camera *cam,
                                         uint32_t band_ty0, uint32_t band_ty1, float *rgba,
                                         const gs_aux_targets *aux) {
    GS_TRY(check_aux(aux));
    return render_frame(r, s, g, gt, mt, cam, band_ty0, band_ty1, rgba, aux);
}

static gs_status check_frame_selection(const gs_renderer *r, const gs_gaussians_buffer *g, const gs_frame_selection *&fs) {
    if (!fs) return GS_OK;
    if (fs->reserved[0] != 0u || fs->reserved[1] != 0u)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, fs->reserved[0], fs->reserved[1], 0, "gs_frame_selection.reserved must be 0");
    if (!fs->hide && !fs->tint) {
        fs = nullptr;           // no selection: the plain frame, whatever the tint says
        return GS_OK;
    }
    if (!r || !g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    const size_t len = gs_gaussians_buffer_len(g);
    for (const gs_selection *sel : {fs->hide, fs->tint}) {
        if (!sel) continue;
        if (sel->dev != r->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the selection belongs to another device");
        if (sel->n != len)
            return gs_fail(GS_ERR_INVALID_ARGUMENT, sel->n, len, 0, "the selection has %zu bits, the buffer %zu Gaussians", sel->n, len);
    }
    if (fs->tint) {
        const float *t = fs->tint_rgba;
        if (!std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2]) || !(t[3] >= 0.0f && t[3] <= 1.0f))
            return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the tint colour must be finite and its alpha in [0, 1]");
    }
    return GS_OK;
}

extern "C" gs_status gs_render_frame_sel(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *g,
                                         const gs_gaussian_transform_pod *gt,
                                         const gs_model_transform_pod *mt, const gs_camera *cam,
                                         uint32_t band_ty0, uint32_t band_ty1, float *rgba,
                                         const gs_aux_targets *aux, const gs_frame_selection *fs) {
    GS_TRY(check_aux(aux));
    GS_TRY(check_frame_selection(r, g, fs));
    return render_frame(r, s, g, gt, mt, cam, band_ty0, band_ty1, rgba, aux, fs);
}

extern "C" gs_status gs_render_frame_contrib(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *g,
                                             const gs_gaussian_transform_pod *gt,
                                             const gs_model_transform_pod *mt, const gs_camera *cam,
                                             uint32_t band_ty0, uint32_t band_ty1, float *rgba,
                                             const gs_frame_selection *fs, gs_buffer *contrib) {
    GS_TRY(check_frame_selection(r, g, fs));
    return render_frame(r, s, g, gt, mt, cam, band_ty0, band_ty1, rgba, nullptr, fs, contrib);
}

static gs_status download_sync(gs_renderer *r, void *dst, const void *src, size_t bytes) {
    if (!bytes) return GS_OK;
    GS_HIP(sync_last_frame(r));
    hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    return GS_OK;
}

// Which Gaussian every OUTPUT slot of the last frame holds (0xffffffff: none — padding past N).  The
// per-slot arrays of a frame (records, depth keys, rects, the values of the sorts) are indexed by
// mirror slot, or — when k_block_cull handed the preprocess kernel its blocks — by LIST slot: list
// position * 1024 + lane.  Either way the taps translate back to Gaussian indices here: through the
// block list (if any) and the buffer's mirror order (if any).
static gs_status download_slot_map(gs_renderer *r, std::vector<uint32_t> &gaussian_of_slot) {
    gaussian_of_slot.clear();
    if (!r->have_frame || !r->n) return GS_OK;
    std::vector<uint32_t> order;
    if (r->last_order) {
        order.resize(r->n);
        GS_TRY(download_sync(r, order.data(), r->last_order->ptr, r->n * 4));
    }
    if (!r->list_mode) {
        gaussian_of_slot.resize(r->n);
        for (size_t slot = 0; slot < r->n; slot++) gaussian_of_slot[slot] = order.empty() ? (uint32_t)slot : order[slot];
        return GS_OK;
    }
    gs::FrameState fs;
    GS_TRY(download_sync(r, &fs, r->state.ptr, sizeof(fs)));
    std::vector<uint32_t> list(fs.list_blocks);
    GS_TRY(download_sync(r, list.data(), r->block_list.ptr, (size_t)fs.list_blocks * 4));
    gaussian_of_slot.assign((size_t)fs.list_blocks * gs::PP_CHUNK, 0xffffffffu);
    for (size_t b = 0; b < list.size(); b++)
        for (size_t l = 0; l < gs::PP_CHUNK; l++) {
            const size_t slot = (size_t)list[b] * gs::PP_CHUNK + l;
            if (slot < r->n) gaussian_of_slot[b * gs::PP_CHUNK + l] = order.empty() ? (uint32_t)slot : order[slot];
        }
    return GS_OK;
}

// depth bits of every output slot of the last frame (0xffffffff = culled): the dense keys of
// preprocess plus the key bias; chunks without visible Gaussians may be block-culled and stale
static gs_status download_slot_depths(gs_renderer *r, size_t slots, std::vector<uint32_t> &depth) {
    depth.assign(slots, 0xffffffffu);
    if (!r->have_frame || !slots) return GS_OK;
    const size_t nchunks = (slots + gs::PP_CHUNK - 1) / gs::PP_CHUNK;
    std::vector<uint32_t> chunk_vis(nchunks);
    GS_TRY(download_sync(r, depth.data(), r->depth.ptr, slots * 4));
    GS_TRY(download_sync(r, chunk_vis.data(), r->chunk_vis.ptr, nchunks * 4));
    for (size_t slot = 0; slot < slots; slot++) {
        if (chunk_vis[slot / gs::PP_CHUNK] == 0u) depth[slot] = 0xffffffffu;
        else if (depth[slot] != 0xffffffffu) depth[slot] += r->key_bias;
    }
    return GS_OK;
}

// The device keeps the projected data as dense per-slot arrays (36-byte blend record, tile rect)
// plus the compacted depth keys; the 48-byte gs_projected view of DESIGN.md §3.3 is assembled here.
extern "C" gs_status gs_renderer_download_projected(gs_renderer *r, gs_projected *proj_out,
                                                    uint32_t *tiles_out, size_t n) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    if (n > r->n) return gs_fail(GS_ERR_INVALID_ARGUMENT, n, r->n, 0, "n exceeds last frame");
    GS_TRY(use_device(r->dev));
    static_assert(sizeof(gs_projected) == 48, "record size");
    if (!n) return GS_OK;
    // a Gaussian whose block the list dropped has no slot at all: it is culled
    if (tiles_out) std::memset(tiles_out, 0, n * sizeof(uint32_t));
    if (proj_out) std::memset(proj_out, 0, n * sizeof(gs_projected));
    // the device arrays are indexed by output slot; a partial request (n < N) still needs all slots
    std::vector<uint32_t> slot_map, depth;
    GS_TRY(download_slot_map(r, slot_map));
    const size_t total = slot_map.size();
    if (!total) return GS_OK;
    std::vector<uint32_t> recs(total * gs::REC_WORDS);
    std::vector<uint2> rect(total);
    std::vector<uint32_t> kept(total);      // tiles of the rect that the frame emits pairs for (all of them, or — rect version 4 — fewer)
    GS_TRY(download_sync(r, recs.data(), r->recs.ptr, total * 4 * gs::REC_WORDS));
    GS_TRY(download_slot_depths(r, total, depth));
    if (r->rect32) {
        std::vector<uint32_t> packed(total);
        GS_TRY(download_sync(r, packed.data(), r->rect.ptr, total * 4));
        for (size_t k = 0; k < total; k++) {      // (culled slots: never looked at)
            uint32_t rows;
            gs::rect_unpack32(packed[k], r->tiles_x ? r->tiles_x : 1u, rect[k].x, rect[k].y, rows);
            kept[k] = gs::rect_count32(packed[k]);
        }
    } else {
        std::vector<uint2> raw(total);
        GS_TRY(download_sync(r, raw.data(), r->rect.ptr, total * 8));
        for (size_t k = 0; k < total; k++) {
            uint32_t rows;
            gs::rect_unpack64(raw[k], rect[k].x, rect[k].y, rows);
            kept[k] = gs::rect_count64(raw[k]);
        }
    }
    for (size_t slot = 0; slot < total; slot++) {
        const size_t i = slot_map[slot];   // Gaussian index of this slot
        if (i >= n) continue;
        // a slot absent from the depth keys is culled (its chunk may even have been block-culled,
        // in which case its per-slot arrays are stale)
        const bool vis = depth[slot] != 0xffffffffu;
        if (tiles_out) tiles_out[i] = vis ? kept[slot] : 0u;
        if (proj_out) {
            gs_projected &p = proj_out[i];
            if (vis) {
                std::memcpy(&p, &recs[slot * gs::REC_WORDS], 36);
                std::memcpy(&p.depth, &depth[slot], 4);
                p.tx0 = (uint16_t)(rect[slot].x & 0xffffu);
                p.ty0 = (uint16_t)(rect[slot].x >> 16);
                p.tx1 = (uint16_t)(rect[slot].y & 0xffffu);
                p.ty1 = (uint16_t)(rect[slot].y >> 16);
            }
        }
    }
    return GS_OK;
}

// The frame sorts (depth) and (tile) separately; the canonical 64-bit key of DESIGN.md §3.4 is
// rebuilt here as tile << 32 | depth bits of the pair's Gaussian.
extern "C" gs_status gs_renderer_download_sorted(gs_renderer *r, uint64_t *keys_out, uint32_t *idx_out,
                                                 uint64_t capacity, uint64_t *pairs_out) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    if (r->have_frame && r->two_round)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 2, 0, 0, "the last frame took two rounds: its pair arrays hold the second round only");
    GS_TRY(use_device(r->dev));
    GS_HIP(sync_last_frame(r));
    uint64_t d = r->have_frame ? last_result(r).pairs_total : 0;
    if (d > r->pair_capacity) d = r->pair_capacity;     // an overflowed frame only holds this many
    if (pairs_out) *pairs_out = d;
    uint64_t m = d < capacity ? d : capacity;
    if (!m) return GS_OK;
    std::vector<uint32_t> idx(m), slot_map;   // output slots of the pairs; slot -> Gaussian
    GS_TRY(download_sync(r, idx.data(), r->tvals[r->tsorted_side].ptr, m * 4));
    GS_TRY(download_slot_map(r, slot_map));
    if (idx_out)
        for (uint64_t j = 0; j < m; j++) idx_out[j] = slot_map[idx[j]];
    if (keys_out) {
        std::vector<uint32_t> depth;
        GS_TRY(download_slot_depths(r, slot_map.size(), depth));
        if (r->wide_tiles) {
            std::vector<uint32_t> t(m);
            GS_TRY(download_sync(r, t.data(), r->tkeys[r->tsorted_side].ptr, m * 4));
            for (uint64_t j = 0; j < m; j++) keys_out[j] = ((uint64_t)t[j] << 32) | depth[idx[j]];
        } else {
            std::vector<uint16_t> t(m);
            GS_TRY(download_sync(r, t.data(), r->tkeys[r->tsorted_side].ptr, m * 2));
            for (uint64_t j = 0; j < m; j++) keys_out[j] = ((uint64_t)t[j] << 32) | depth[idx[j]];
        }
    }
    return GS_OK;
}

extern "C" gs_status gs_renderer_download_ranges(gs_renderer *r, uint32_t *ranges_out,
                                                 size_t num_tiles) {
    if (!r || !ranges_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (num_tiles > (size_t)r->tiles_x * r->tiles_y)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, num_tiles, 0, 0, "too many tiles");
    if (r->have_frame && r->two_round)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 2, 0, 0, "the last frame took two rounds: its tile ranges are the second round's");
    GS_TRY(use_device(r->dev));
    return download_sync(r, ranges_out, r->zero_region.ptr, num_tiles * 8);
}

// ------------------------------------------------------------------------------------------------
// select what the last frame shows
// ------------------------------------------------------------------------------------------------

extern "C" gs_status gs_renderer_select_visible(gs_renderer *r, gs_stream *s, gs_selection *sel, float x0, float y0, float x1, float y1,
                                                const uint8_t *mask, gs_select_op op) {
    if (!r) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null renderer");
    GS_TRY(check_selection(sel, s));
    GS_TRY(check_select_op(op));
    if (sel->dev != r->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (!r->have_frame) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the renderer has no last frame");
    if (sel->n != r->n) return gs_fail(GS_ERR_INVALID_ARGUMENT, sel->n, r->n, 0, "the selection has %zu bits, the last frame %zu Gaussians", sel->n, (size_t)r->n);
    hipStream_t st = s->s;
    // behind the last frame; from here on the renderer's newest work is on `st`, so its next frame — on whatever stream —
    // is ordered behind this call the way it is ordered behind a frame
    GS_TRY(take_over_stream(r, st));
    r->last_stream = st;
    r->last_stream_gone = false;
    if (!sel->nwords) {
        sel->generation = next_object_id();
        return GS_OK;
    }
    GS_TRY(dev_reserve(sel->scratch, sel->nwords * 4));
    GS_HIP(hipMemsetAsync(sel->scratch.ptr, 0, sel->nwords * 4, st));
    const size_t nchunks = ((size_t)r->n + gs::PP_CHUNK - 1) / gs::PP_CHUNK;
    gs::VisibleIO io;
    io.depth = (const uint32_t *)r->depth.ptr;
    io.chunk_vis = (const uint32_t *)r->chunk_vis.ptr;
    io.recs = (const uint32_t *)r->recs.ptr;
    io.block_list = r->list_mode ? (const uint32_t *)r->block_list.ptr : nullptr;
    io.list_blocks = &((const gs::FrameState *)r->state.ptr)->list_blocks;
    io.order = r->last_order ? (const uint32_t *)r->last_order->ptr : nullptr;
    io.n = (uint32_t)r->n;
    io.nslots = (uint32_t)(nchunks * gs::PP_CHUNK);
    io.x0 = x0; io.y0 = y0; io.x1 = x1; io.y1 = y1;
    io.mask = mask;
    io.width = r->width;
    io.height = r->height;
    io.scratch = (uint32_t *)sel->scratch.ptr;
    hipLaunchKernelGGL(gs::k_select_visible, dim3(io.nslots / 256u), dim3(256), 0, st, io);
    GS_HIP(hipGetLastError());
    GS_TRY(selection_combine_words(sel, st, op, (const uint32_t *)sel->scratch.ptr));
    if (switches().frame_event) {
        // (per-frame events: the end-of-frame event moves behind this call, which `st` has ordered behind the frame)
        GS_HIP(hipEventRecord(r->done[r->gen & 1u], st));
        r->done_valid[r->gen & 1u] = true;
    }
    return GS_OK;
}

// ------------------------------------------------------------------------------------------------
// stand-alone primitives
// ------------------------------------------------------------------------------------------------

extern "C" gs_status gs_sort_pairs_u64(gs_device *dev, gs_stream *s, uint64_t *keys, uint32_t *values,
                                       uint64_t count, uint32_t end_bit) {
    if (!dev || (count && (!keys || !values)) || end_bit > 64 || count > 0xfffffff0ull)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, count, end_bit, 0, "bad argument");
    GS_TRY(use_device(dev));
    if (!count) return GS_OK;
    hipStream_t st = stream_of(dev, s);
    // (the returns after a failed copy or sort free with that work queued, as the common tail did: hipFree waits)
    DevArray k[2], v[2], gh, dt;
    for (int i = 0; i < 2; i++) {
        GS_TRY(dev_reserve(k[i], count * 8));
        GS_TRY(dev_reserve(v[i], count * 4));
    }
    hipError_t e = hipMemcpyAsync(k[0].ptr, keys, count * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(v[0].ptr, values, count * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "upload failed: %s", hipGetErrorString(e));
    int side = 0;
    uint32_t passes = 0;
    void *k2[2] = {k[0].ptr, k[1].ptr};
    void *v2[2] = {v[0].ptr, v[1].ptr};
    GS_TRY(sort_pairs_device<uint64_t>(dev, k2, v2, gh, dt, (uint32_t)count, end_bit, st, side, passes));
    e = hipMemcpyAsync(keys, k[side].ptr, count * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(values, v[side].ptr, count * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    return GS_OK;
}

namespace gs {
// chunk sums for the stand-alone scan (the frame fuses this into k_preprocess)
__global__ __launch_bounds__(PP_THREADS) void k_chunk_sums(const uint32_t *__restrict__ in, uint32_t n,
                                                           uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_red[4];
    uint32_t base = blockIdx.x * PP_CHUNK + threadIdx.x * PP_ITEMS;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < PP_ITEMS; k++) v += base + k < n ? in[base + k] : 0u;
    v = wave_reduce_add(v);
    if ((threadIdx.x & 63u) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// per-chunk exclusive scan written out
__global__ __launch_bounds__(PP_THREADS) void k_chunk_scan_write(const uint32_t *__restrict__ in,
                                                                 const uint32_t *__restrict__ chunk_offsets,
                                                                 uint32_t n, uint32_t *__restrict__ out) {
    __shared__ uint32_t s_scan[4];
    uint32_t base = blockIdx.x * PP_CHUNK + threadIdx.x * PP_ITEMS;
    uint32_t c[PP_ITEMS], sum = 0;
#pragma unroll
    for (int k = 0; k < PP_ITEMS; k++) {
        c[k] = base + k < n ? in[base + k] : 0u;
        sum += c[k];
    }
    uint32_t total;
    uint32_t off = chunk_offsets[blockIdx.x] + block_exclusive_scan_256(sum, s_scan, total);
#pragma unroll
    for (int k = 0; k < PP_ITEMS; k++) {
        if (base + k < n) out[base + k] = off;
        off += c[k];
    }
}
}  // namespace gs

extern "C" gs_status gs_exclusive_scan_u32(gs_device *dev, gs_stream *s, const uint32_t *in,
                                           uint32_t *out, uint64_t count, uint64_t *total_out) {
    if (!dev || (count && (!in || !out)) || count > 0xfffffff0ull)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, count, 0, 0, "bad argument");
    GS_TRY(use_device(dev));
    if (total_out) *total_out = 0;
    if (!count) return GS_OK;
    hipStream_t st = stream_of(dev, s);
    uint32_t n = (uint32_t)count;
    uint32_t nchunks = (n + gs::PP_CHUNK - 1) / gs::PP_CHUNK;
    DevArray din, dout, sums, offs, tot;
    GS_TRY(dev_reserve(din, count * 4));
    GS_TRY(dev_reserve(dout, count * 4));
    GS_TRY(dev_reserve(sums, (size_t)nchunks * 4));
    GS_TRY(dev_reserve(offs, (size_t)nchunks * 4));
    GS_TRY(dev_reserve(tot, 16));
    uint32_t total = 0;
    hipError_t e = hipMemcpyAsync(din.ptr, in, count * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(gs::k_chunk_sums, dim3(nchunks), dim3(gs::PP_THREADS), 0, st,
                           (const uint32_t *)din.ptr, n, (uint32_t *)sums.ptr);
        scan_chunks_enqueue(st, (const uint32_t *)sums.ptr, (uint32_t *)offs.ptr, (uint32_t *)tot.ptr, nchunks);
        hipLaunchKernelGGL(gs::k_chunk_scan_write, dim3(nchunks), dim3(gs::PP_THREADS), 0, st,
                           (const uint32_t *)din.ptr, (const uint32_t *)offs.ptr, n,
                           (uint32_t *)dout.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, count * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, tot.ptr, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // (a failure frees with that work queued, as the common tail did: hipFree waits.  *total_out stays 0 then.)
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "scan failed: %s", hipGetErrorString(e));
    if (total_out) *total_out = total;
    return GS_OK;
}
