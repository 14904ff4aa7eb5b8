// gs_policy.h — what a frame decides before and between its launches: pure arithmetic on the reports of the finished
// frames, the frame's shape numbers, the requests of the API, the environment switches and the renderer's feedback
// state.  No HIP header, no HIP call, no launch: tests/cpp/test_policy.cpp compiles this file with a host compiler.
// The device-side constants the rules refer to come in through PolicyParams (the render unit, gs3d.hip, fills it from gs_render_kernels.h).
#pragma once

#include <cstdint>

namespace gsp {

// ------------------------------------------------------------------------------------------------
// switches: every GS3D_* environment variable the library reads once per process (read_switches() in gs_core.hip fills
// the table on first use; the defaults here are the values of an empty environment).  -1 = "not set": the renderer
// chooses.  Precedence everywhere: gs_renderer_set_* request, then the environment, then the renderer's own choice.
// ------------------------------------------------------------------------------------------------
struct Switches {
    bool roctx = false;             // GS3D_ROCTX=1: roctx ranges around the stages of a frame
    bool event_fence = false;       // GS3D_EVENT_FENCE=1: system-scope fence at the end-of-frame events
    bool frame_event = false;       // GS3D_FRAME_EVENT=1: an event at the end of every frame, queried before the history is read
    bool test_rank_fault = false;   // GS3D_TEST_RANK_FAULT=1 (tests): the rank watchdog's expectation is off by one
    bool test_rank_watch_set = false;   // GS3D_TEST_RANK_WATCH=<n> (tests): pins the rank watchdog's sample
    uint32_t test_rank_watch = 0;
    bool rect_v1 = false;           // GS3D_RECT_V1=1: the unclipped tile rect of spec version 1
    bool rect32_off = false;        // GS3D_RECT32=0: tile rects always as uint2
    int wt_stores = 3;              // GS3D_WT_STORES: write-through stores, bit 0 = the pairs of k_pairs_emit, bit 1 = the image
    int wt_records = 0;             // GS3D_WT_RECORDS: write-through stores of the records (two bits)
    bool scan_rows_small_off = false;   // GS3D_SCAN_ROWS_SMALL=0: always the one-workgroup-per-row scan
    int nt_scatter = -1;            // GS3D_NT_SCATTER=0/1: non-temporal reads of the scatter's input
    bool chunk_hist_off = false;    // GS3D_CHUNK_HIST=0: the compacting pass counts its histogram from the keys again
    bool narrow_keys_off = false;   // GS3D_NARROW_KEYS=0: no 16-bit keys in the depth sort's last pass
    bool xcd_remap_off = false;     // GS3D_XCD_REMAP=0: radix passes in dispatch order
    int xcd_remap_c = 0;            // GS3D_XCD_REMAP_C=<n>: forces the span of the XCD-aware tile order
    int depth_sort_large = -1;      // GS3D_DEPTH_SORT_LARGE=0/1: 4096- / 8192-key tiles for 32-bit keys
    int tile_sort_large = -1;       // GS3D_TILE_SORT_LARGE=0/1: 4096- / 8192-key tiles for the 16-bit tile keys
    int tile_masks = -1;            // GS3D_TILE_MASKS=0/1: tile rect version 3 / 4
    int depth_msd = -1;             // GS3D_DEPTH_MSD=0/1: LSD / MSD-first depth sort
    int blend_groups = 0;           // GS3D_BLEND_GROUPS = 1 (half-tile lists), 2 (8x8 blocks), 4 (8x4 blocks) or 8 (4x4 blocks); 0: plan_blend_groups
    int blend_free_body = -1;       // GS3D_BLEND_FREE_BODY=0/1: the grouped blend's trip loop always branchy / always branch-free; unset: plan_blend_free_min_live
    int rounds = -1;                // GS3D_ROUNDS=0/1: one round / two
    long round1 = 0;                // GS3D_ROUND1=<k>: Gaussians of round 1
    int round_partition = -1;       // GS3D_ROUND_PARTITION=0/1: two-round frames sort each round on its own
    int force_banded = -1;          // GS3D_FORCE_BANDED=0/1: single-phase / two-phase preprocess kernel
    int mask_rec = -1;              // GS3D_MASK_REC=0/1: records of culled Gaussians are (not) written
    int nt_loads = -1;              // GS3D_NT_LOADS=0/1: non-temporal loads of the mirror
    bool block_cull_off = false;    // GS3D_BLOCK_CULL=0: no block culling
    int block_list = -1;            // GS3D_BLOCK_LIST=0/1: block test inside the preprocess kernel / k_block_cull's list
    bool pre_serial = false;        // GS3D_PRE_PIPELINE=0: the two-phase kernel without the prefetch of the next Gaussian's geometry chunks
    int cursor_kernel = -1;         // GS3D_CURSOR_KERNEL=0/1: k_pairs_emit searches its start / looks it up (k_pairs_cursors)
    int expand_xcd = 64;            // GS3D_EXPAND_XCD=<C>: span of the gather's XCD-aware order, 0 = dispatch order
    int tile_msd = -1;              // GS3D_TILE_MSD=0/1: LSD / MSD-first tile sort
    bool tile_msd_auto = false;     // GS3D_TILE_MSD_AUTO=1: the renderer may choose the MSD-first tile sort by itself
    int ranges_in_blend = -1;       // GS3D_RANGES_IN_BLEND=0/1: the blend workgroups search their tile's range themselves
    int ranges_search = -1;         // GS3D_RANGES_SEARCH=0/1: k_tile_ranges / k_tile_ranges_search
    long export_slice = 0;          // GS3D_EXPORT_SLICE=<records>: source records per kernel of the PLY export, a multiple of 1024 (tests)
};

// what gs_renderer_set_sort_mode / _set_tile_masks / _set_rounds asked for (-1 / 0: the renderer chooses)
struct Requests {
    int depth_msd = -1, tile_msd = -1, tile_masks = -1, rounds = -1;
    uint32_t round1 = 0;
    // a contribution frame (gs_render_frame_contrib): one round, whatever the pin — planned as under rounds = 0, round1 = 0.
    // A frame skipped for pair capacity must leave the accumulators untouched, and round 1's adds could not be undone.
    bool single_round = false;
};

// constants of the kernels the rules compare against
struct PolicyParams {
    uint32_t bkt_cap = 0;          // gs::BKT_CAP: largest bucket of the depth bucket sort's register path
    uint32_t bkt_cap_small = 0;    // gs::BKT_CAP_SMALL: ... of the tile bucket sort's
    uint32_t msd_top_bits = 0;     // gs::MSD_TOP_BITS
    uint32_t radix_bits_max = 0;   // gs::RADIX_BITS_MAX
};

// ------------------------------------------------------------------------------------------------
// history: the (up to two) self-validated reports of finished frames
// ------------------------------------------------------------------------------------------------
struct Report {
    uint32_t gen = 0;               // 0: no report in this block
    uint64_t pairs = 0;
    uint32_t visible = 0, depth_bucket_max = 0, tile_bucket_max = 0, tiles_done = 0, tiles_open = 0, round_pairs_max = 0;
    uint32_t shape_epoch = 0;       // the frame's shape epoch, rounds and round-1 length (host-side knowledge of the frame)
    uint32_t rounds = 1, round_k = 0;
};

struct History {
    Report rep[2];
    uint32_t shape_epoch = 0;       // the renderer's epoch when the snapshot was taken
    bool rank_fault_seen = false;
    // the newest report, whatever its shape (the block-list choice, and "is there any report at all")
    const Report *newest_any() const {
        const Report &p = rep[rep[0].gen > rep[1].gen ? 0 : 1];
        return p.gen ? &p : nullptr;
    }
    // the newest finished report if it belongs to the current shape epoch, or none
    const Report *newest() const {
        const Report *p = newest_any();
        return p && p->shape_epoch == shape_epoch ? p : nullptr;
    }
};

// ------------------------------------------------------------------------------------------------
// the frame's shape numbers
// ------------------------------------------------------------------------------------------------
struct FrameNums {
    uint32_t n = 0, gen = 0;
    uint32_t num_tiles = 0, tiles_y = 0, band_rows = 0, band_tiles = 0;
    uint32_t dbits = 0, tile_bits = 0;
    bool wide = false;               // more than 65536 tiles: u32 tile keys
    bool sizing = false;             // the frame measures its pair count before it sizes the buffers
    uint64_t pair_capacity = 0;      // the buffers' capacity when the frame starts
    uint64_t pod_bytes = 0;          // bytes of one Gaussian in the mirror
    bool has_sh = false, has_order = false;
};

// ------------------------------------------------------------------------------------------------
// feedback state of the renderer (gs_renderer::sort_fb / rounds_fb): what the rules below remember between frames
// ------------------------------------------------------------------------------------------------
// Depth sort of the frame: MSD-first (one scatter on the top digit + k_bucket_sort) or the LSD passes.  The choice
// follows the largest top-digit bucket the last frames reported (FrameResult::depth_bucket_max): MSD-first while
// the buckets fit a workgroup's registers, LSD while they do not; a shape's first frame guesses from N.
struct SortFeedback {
    bool depth_msd = false;               // mode of the last frame
    uint32_t depth_bucket_seen = 0;       // newest reported bucket size the mode was chosen from (diagnostic)
    uint64_t tile_msd_fail_d = 0;         // pair count at which the MSD-first tile sort last reported an oversized bucket (0: never)
};

// what the renderer's own choice of the rounds rests on: the pair count of a single-round frame of this shape (the
// sizing pass's, or the newest single-round report with the visible count it came with), the rounds of the frames
// behind the two result blocks, and the feedback state (the length of round 1 is scaled up while round 1 finishes
// too few tiles; past 3.4 x the renderer stays with one round until the shape changes)
struct RoundsFeedback {
    uint64_t full_pairs = 0;
    uint32_t full_pairs_v = 0, rounds_epoch = 0, rounds_fb_gen = 0;
    float round_scale = 1.0f;
    bool rounds_off = false;
    uint32_t rounds_off_gen = 0;          // the frame that switched the rounds off (another try 512 frames later)
    uint64_t round_cap = 0;               // the pair bound the last two-round frame used for its grids (0: the buffers' capacity)
    uint32_t round_cap_k = 0;             // ... and the length of round 1 it was measured with
    bool auto_deep = false;               // the renderer's last own choice (kept while no report is available)
    bool auto_all_done = false;           // the newest two-round report of this shape: round 1 finished every tile (round 2 was skipped)
    uint64_t auto_k = 0;
};

enum RangeMode { RANGES_NONE = 0, RANGES_IN_BLEND, RANGES_SEARCH, RANGES_PASS };

struct FramePlan {
    // decided before anything is launched (plan_frame)
    uint64_t want_capacity = 0;
    bool tile_masks = false;
    bool depth_msd = false;
    bool two_round = false;
    uint32_t round_k = 0;
    bool partition = false;
    bool use_list = false, banded = false, block_cull = false;
    uint32_t nt_loads = 0, mask_culled_records = 0;
    // decided once the pair buffers have their size (plan_pairs)
    uint32_t capacity = 0;                // pair bound of every round of this frame
    bool tile_msd = false;                // (single-round frames only)
};

// pair capacity for a frame expected to produce `d` pairs: 25 % head room for a moving camera
inline uint64_t capacity_for(uint64_t d) { return d + d / 4 + 65536; }

inline uint64_t plan_capacity(const History &h, uint64_t pair_capacity) {
    uint64_t want_capacity = pair_capacity;
    for (const Report &p : h.rep) {
        // grow when the last measured D leaves less than 1/8 of head room
        if (p.gen && p.pairs + p.pairs / 8 > pair_capacity && capacity_for(p.pairs) > want_capacity) want_capacity = capacity_for(p.pairs);
    }
    // A camera that keeps closing in: D grows frame over frame, and this frame is two or three frames
    // ahead of the newest result (frames are pipelined).  Extrapolate the last step three frames ahead
    // and size for that, so that a steady zoom does not run into the skip path.
    // Only a TREND is extrapolated: both results must come from the current shape epoch (same N, image
    // size and band — a switch from a band to the full frame, or a resize, is a discontinuity, not a zoom),
    // and the extrapolation is capped at twice the newest D: one jump of the camera must not turn into
    // pair buffers of 4 x D that never shrink.
    const Report &a = h.rep[0], &b = h.rep[1];
    if (a.gen && b.gen && (a.gen + 1u == b.gen || b.gen + 1u == a.gen) && a.shape_epoch == h.shape_epoch && b.shape_epoch == h.shape_epoch) {
        const uint64_t d_new = a.gen > b.gen ? a.pairs : b.pairs, d_old = a.gen > b.gen ? b.pairs : a.pairs;
        if (d_new > d_old) {
            uint64_t ahead = d_new + 3u * (d_new - d_old);
            if (ahead > 2u * d_new) ahead = 2u * d_new;
            if (ahead + ahead / 8 > pair_capacity && capacity_for(ahead) > want_capacity) want_capacity = capacity_for(ahead);
        }
    }
    return want_capacity;
}

// Tile rect version 4: pinned by the caller or the environment, otherwise on where the preprocess kernel waits for
// HBM long enough to hide the test's ~120 instructions per Gaussian: records of 200 bytes or more (f32 SH) in a
// scene beyond the Infinity Cache.  Same-box A/B, frame time with / without (gpurun_out/r05i/ab_masks3.txt): 10 M x
// 224 B at 4K 1.521 / 1.558 ms, at 1080p 0.926-0.951 / 0.926-0.959 (tile sort -12 us); 50 M x 144 B 3.37-3.45 /
// 3.31-3.37 (preprocess +65..130 us, tile sort -20..55); 1 M x 48 B 0.318 / 0.320 (preprocess +5 us).
// clip_rect: the display mode allows it; n64 / pod_bytes: Gaussians in the buffer and bytes of one of them in the mirror
inline bool plan_tile_masks(bool clip_rect, uint64_t n64, uint64_t pod_bytes, const Requests &req, const Switches &sw) {
    const int pinned = req.tile_masks >= 0 ? req.tile_masks : sw.tile_masks;
    const bool want = pinned >= 0 ? pinned != 0 : pod_bytes >= 200u && n64 * pod_bytes > (512ull << 20);
    return clip_rect && want;
}

// ---- which depth sort (SortFeedback::depth_msd) ----
// MSD-first needs a top digit of 10 bits and at most two bucket passes (of 9) below it: 11..28 key bits (the bench's planes,
// 0.1 / 100, give 27); with fewer or more bits the LSD passes stand.
inline uint32_t msd_low_bits(const FrameNums &f, const PolicyParams &P) { return f.dbits > P.msd_top_bits ? f.dbits - P.msd_top_bits : 0u; }

inline bool plan_depth_msd(const History &h, const FrameNums &f, const Requests &req, const Switches &sw, const PolicyParams &P,
                           SortFeedback &fb) {
    const bool msd_possible = f.n != 0 && f.dbits > P.msd_top_bits && msd_low_bits(f, P) <= 2u * P.radix_bits_max;
    bool depth_msd = false;
    if (msd_possible) {
        const Report *p = f.sizing ? nullptr : h.newest();
        const int pinned = req.depth_msd >= 0 ? req.depth_msd : sw.depth_msd;
        if (pinned >= 0) {
            depth_msd = pinned != 0;
        } else if (p && p->depth_bucket_max) {
            // hysteresis: leave MSD-first when a bucket no longer fits the register path, come back below 7/8 of it
            const uint32_t b = p->depth_bucket_max;
            fb.depth_bucket_seen = b;
            depth_msd = fb.depth_msd ? b <= P.bkt_cap : b <= P.bkt_cap - P.bkt_cap / 8u;
        } else if (f.sizing) {
            // no report yet: the buckets of a scene this small probably fit (and if not, the bucket kernel's chunked path
            // still sorts them correctly, and the report of this very frame corrects the choice)
            depth_msd = f.n <= (4u << 20);
        } else {
            depth_msd = fb.depth_msd;      // frames in flight between the sizing frame and its report: keep the guess
        }
    }
    fb.depth_msd = depth_msd;
    return depth_msd;
}

// ---- one round, or two (DESIGN.md §4.2 "rounds"): decided before anything is launched, because a partitioned frame
//      changes what the preprocess kernel counts and what the depth sorts see ----
// A deep scene finishes most of its tiles on the nearest fraction of its Gaussians; everything behind them is
// emitted, sorted and staged for nothing.  Two rounds: the frame of the nearest K visible Gaussians first, whose
// blend leaves a bit per finished tile and the pixel state of the others; then the rest, without the Gaussians whose
// (small) rect lies in finished tiles, resumed by the same blend.  The image is the single round's, bit for bit: a
// tile's list is the concatenation of its two lists, and a dropped Gaussian touches finished pixels only.
// Returns two_round; round_k = the length of round 1 (0 with one round... or when no frame of this kind can take two).
inline bool plan_rounds(const History &h, const FrameNums &f, const Requests &req, const Switches &sw, RoundsFeedback &fb, uint32_t &round_k) {
    round_k = 0;
    bool two_round = false;
    if (fb.rounds_epoch != h.shape_epoch) {      // a new shape: the feedback starts over
        fb.rounds_epoch = h.shape_epoch;
        fb.round_scale = 1.0f;
        fb.rounds_off = false;
        fb.auto_deep = false;
        fb.auto_k = 0;
    }
    if (f.band_tiles && sw.blend_groups != 1 && f.n > 4096u) {
        const Report *p = f.sizing ? nullptr : h.newest();
        const bool have = p != nullptr;
        const uint32_t v_est = have ? p->visible : f.n;
        if (have && p->rounds == 1) {
            fb.full_pairs = p->pairs;
            fb.full_pairs_v = p->visible;
        }
        // pairs a single round would emit now: the measured count, scaled with the visible Gaussians since
        const double d_full = fb.full_pairs_v ? (double)fb.full_pairs * (double)v_est / (double)fb.full_pairs_v : (double)fb.full_pairs;
        // The renderer's own choice.  Measured (same-box A/B, gpurun_out/r05r): 10 M at 1080p (2 970 pairs per tile) -9 %,
        // at 4K (1 716) -8 %, 50 M (14 800) -24 %; the 1 M scene (296 pairs per tile) finishes its tiles only at the end of
        // their lists.  Round 1 is given ~250 pairs per tile: the bench scenes finish EVERY tile from ~170 on (k_round2_gate
        // then skips round 2), and a shorter round 1 is a shorter tile sort (same-box sweep, gpurun_out/r05x/ab_k.txt: 10 M
        // 0.813 / 0.801 / 0.790 / 0.786 ms at 400 / 270 / 210 / 170 pairs per tile, 50 M 2.07 / 2.06 / 2.02 / 2.02) — and a frame
        // takes two rounds when that is at most a third of its Gaussians and the pairs to save outweigh the launches of a
        // second round.  The feedback below lengthens a round 1 that turns out too short.
        const double per_tile = d_full / (double)f.band_tiles;
        double k_auto = per_tile > 0.0 ? (double)v_est * 250.0 / per_tile * (double)fb.round_scale : 0.0;
        if (have && p->rounds == 2 && p->gen != fb.rounds_fb_gen) {
            // feedback: a round 1 that finishes less than 60 % of the tiles it has pairs for was too short (or the scene
            // does not occlude)
            fb.rounds_fb_gen = p->gen;
            if ((uint64_t)p->tiles_done * 10u < ((uint64_t)p->tiles_done + p->tiles_open) * 6u) {
                fb.round_scale *= 1.5f;
                if (fb.round_scale > 3.4f) {
                    fb.rounds_off = true;
                    fb.rounds_off_gen = f.gen;
                }
            } else if (p->tiles_open != 0u && (uint64_t)p->tiles_open * 10u <= (uint64_t)p->tiles_done + p->tiles_open &&
                       fb.round_scale < 2.7f) {
                // nearly there (at most a tenth of the tiles with pairs left open): a little longer and round 2 is skipped
                fb.round_scale *= 1.25f;
            }
        }
        if (fb.rounds_off && f.gen - fb.rounds_off_gen > 512u) {
            // ... but not for ever: the camera may have moved into a view that does occlude; another try every 512 frames
            fb.rounds_off = false;
            fb.round_scale = 1.0f;
        }
        bool deep = have && !fb.rounds_off && d_full >= 12.0e6 && per_tile >= 1200.0 && k_auto * 3.0 <= (double)v_est;
        if (!have && !f.sizing && fb.rounds_epoch == h.shape_epoch) {
            // frames in flight: no finished report to consult (both result blocks belong to frames still running):
            // what the last frame with a report decided stands
            deep = fb.auto_deep && !fb.rounds_off;
            k_auto = (double)fb.auto_k;
        }
        fb.auto_deep = deep;
        fb.auto_k = (uint64_t)k_auto;
        const int req_rounds = req.single_round ? 0 : req.rounds;
        const uint32_t req_round1 = req.single_round ? 0u : req.round1;
        const int pinned = req_rounds >= 0 ? req_rounds : sw.rounds;
        two_round = pinned >= 0 ? pinned != 0 : deep;
        const uint64_t k = req_round1 ? req_round1 : sw.round1 > 0 ? (uint64_t)sw.round1 : pinned > 0 && !deep ? v_est / 4u : (uint64_t)k_auto;
        round_k = (uint32_t)((k + 2047u) / 2048u * 2048u < f.n ? (k + 2047u) / 2048u * 2048u : 0u);
        if (round_k == 0u) two_round = false;
    }
    return two_round;
}

// A two-round frame is PARTITIONED when the depth keys have a top digit to cut at (and the frame is not the one that
// sizes the pair buffers): the preprocess kernel counts the top 10 bits of every key, k_round_threshold picks the digit
// boundary with at least round_k Gaussians in front of it, and each round's depth sort — LSD passes whose compacting
// first pass takes only its side of the boundary (gs::CompactPred) — sorts what that round renders: the nearest ones,
// then what k_round2_slot_bits keeps of the rest.  Otherwise round 2 is compacted out of the full depth order
// (k_round2_count / _write).
// Measured, same-box A/B.  With a round 2 that runs (gpurun_out/r05t/ab3.txt): 50 M 2.42 against 2.53 ms (depth-sort stage
// 0.318 against 0.462: a threshold + two sorts whose first pass streams the 200 MB of dense keys for 1-2 M survivors,
// against one full sort + the compaction), 10 M 0.908 against 0.865 (two first passes of ~50 us each at their launch-bound
// floors cost more than the full sort of 7 M keys saves).  With a round 2 that k_round2_gate skips — round 1 finished every
// tile — only round 1's sort remains (gpurun_out/r05x/ab_part.txt): 10 M 0.806 against 0.817, 4K 1.29 against 1.32, 50 M 2.00
// against 2.15.  So: from 32 M Gaussians, or when the newest two-round report of this shape says that round 1 finished
// every tile (kept while no report is available); GS3D_ROUND_PARTITION=0/1 forces.
inline bool plan_partition(const History &h, const FrameNums &f, const Switches &sw, const PolicyParams &P, bool two_round, RoundsFeedback &fb) {
    bool partition_auto = f.n >= (32u << 20);
    if (const Report *p = f.sizing ? nullptr : h.newest()) {
        if (p->rounds == 2) fb.auto_all_done = p->tiles_done == f.band_tiles && p->tiles_open == 0u;
    } else if (f.sizing) {
        fb.auto_all_done = false;
    }
    partition_auto = partition_auto || fb.auto_all_done;
    return two_round && !f.sizing && f.dbits > P.msd_top_bits && f.n < (1u << 30) &&
           (sw.round_partition >= 0 ? sw.round_partition != 0 : partition_auto);
}

// Block list (k_block_cull): one thread per block tests it, the survivors are handed to the first
// workgroups of the preprocess grid.  GS3D_BLOCK_LIST=0 keeps the test inside the preprocess kernel.
// It pays when most blocks are culled (a rank's band of 8 at 50 M: preprocess 0.57 -> 0.41 ms) and
// costs its launch when few are (whole 1080p frame at 10 M: +4 us), so it is taken when the newest
// finished frame of this shape saw less than half of the Gaussians, or — no such frame yet — when
// the frame is a band.  GS3D_BLOCK_LIST=0/1 forces.
// (the newest report WITHOUT the shape test: newest_any)
inline bool plan_use_list(const History &h, const FrameNums &f, const Switches &sw) {
    bool use_list = f.band_rows < f.tiles_y;
    const Report *p = h.newest_any();
    if (!f.sizing && p) use_list = p->visible < f.n / 2u;
    if (sw.block_list >= 0) use_list = sw.block_list != 0;
    // the list frame keeps its outputs in list space: list_slots = blocks * 1024 must fit 32 bits, and the
    // look-back of k_block_cull is written for at most 2^20 groups of 256 blocks
    if (f.n > 0xfffff000u) use_list = false;
    return use_list;
}

// everything decided before the frame's first launch (but the tile rect version: plan_tile_masks, before N is checked)
inline void plan_frame(const History &h, const FrameNums &f, const Requests &req, const Switches &sw, const PolicyParams &P,
                       SortFeedback &sfb, RoundsFeedback &rfb, FramePlan &plan) {
    plan.want_capacity = plan_capacity(h, f.pair_capacity);
    plan.depth_msd = plan_depth_msd(h, f, req, sw, P, sfb);
    plan.two_round = plan_rounds(h, f, req, sw, rfb, plan.round_k);
    plan.partition = plan_partition(h, f, sw, P, plan.two_round, rfb);
    if (plan.partition) {
        plan.depth_msd = false;
        sfb.depth_msd = false;
    }
    // Records with SH take the two-phase kernel (geometry chunks first, SH chunks only for the
    // lanes that survive culling): with the mirror in spatial order whole 128-byte lines of
    // culled Gaussians are never fetched; with a random order it costs the same as the
    // single-phase kernel (measured).  GS3D_FORCE_BANDED=0/1 overrides for experiments.
    plan.banded = f.has_sh && (sw.force_banded >= 0 ? sw.force_banded != 0 : true);
    plan.mask_culled_records = sw.mask_rec >= 0 ? (uint32_t)sw.mask_rec : (f.has_order ? 1u : 0u);
    // Non-temporal loads of the mirror once it no longer fits the 256 MiB Infinity Cache: nothing of
    // it survives until the next frame anyway (10 M x 224 B: preprocess 0.440 -> 0.421 ms); a mirror that
    // does fit is re-read from the caches frame after frame and loses that with nt (1 M x 48 B:
    // 22 -> 27 us).  GS3D_NT_LOADS=0/1 forces.
    plan.nt_loads = sw.nt_loads >= 0 ? (uint32_t)sw.nt_loads : ((uint64_t)f.n * f.pod_bytes > (512ull << 20) ? 1u : 0u);
    // SH-less records are 48 bytes: the block test (one more dependent load per workgroup)
    // costs more than skipping them saves (measured at 1 M: +4 us on a 20 us kernel)
    // (the caller also needs the buffer's block bounds)
    plan.block_cull = !sw.block_cull_off && plan.banded;
    plan.use_list = plan_use_list(h, f, sw);
}

// A two-round frame sizes its grids — and bounds each round — by what a ROUND emitted last time, not by the single-round
// pair count that sized the buffers (50 M: 3 M pairs per round in buffers for 150 M: the emission's and the tile sort's
// 37 000 mostly empty workgroups cost 20-40 us per kernel): twice the larger round of the newest two-round report, with
// the usual head room.  A round that still outgrows it skips the frame like any pair overflow (the next one has the
// report); the first two-round frame of a shape, and any frame without a report, use the buffers' capacity.
// `pair_capacity`: the buffers' capacity now (the sizing pass may just have set it).
inline uint32_t plan_round_capacity(const History &h, const FrameNums &f, uint64_t pair_capacity, bool two_round, uint32_t round_k, RoundsFeedback &fb) {
    uint32_t capacity = (uint32_t)pair_capacity;
    if (two_round) {
        const Report *p = f.sizing ? nullptr : h.newest();
        uint64_t want = 0;
        // (only a report of a frame whose round 1 was as long as this one's says anything about this frame's rounds)
        if (p && p->rounds == 2 && p->round_pairs_max && p->round_k == round_k)
            want = capacity_for(2ull * p->round_pairs_max);
        else if (!f.sizing && !h.newest_any() && fb.round_cap && fb.round_cap_k == round_k)
            want = fb.round_cap;          // frames in flight: the last bound stands
        if (want && want < capacity) capacity = (uint32_t)want;
        fb.round_cap = want;
        fb.round_cap_k = round_k;
    }
    return capacity;
}

// Which tile sort (gs_renderer::tile_msd) of a single-round frame.  MSD-first needs u16 tile ids with more than 10 bits; its
// buckets are 2^(bits - 10) consecutive tiles, so what decides is the pair count: up to an average of a quarter of the register
// path's capacity per bucket it is tried, and a frame that reports a bucket beyond the capacity (FrameResult::
// tile_bucket_max, one frame late) sends the renderer back to the LSD passes until the pair count has dropped by
// a quarter below the count that failed.
inline bool plan_tile_msd(const History &h, const FrameNums &f, const Requests &req, const Switches &sw, const PolicyParams &P, uint32_t capacity,
                          SortFeedback &fb) {
    if (f.wide || f.tile_bits <= P.msd_top_bits || capacity == 0u) return false;
    const int pinned = req.tile_msd >= 0 ? req.tile_msd : sw.tile_msd;
    const Report *p = f.sizing ? nullptr : h.newest();
    // pairs this frame is expected to hold: the newest report of this shape, else what sized the buffers
    const uint64_t d_est = p ? p->pairs : (uint64_t)capacity * 4u / 5u;
    if (p && p->tile_bucket_max > P.bkt_cap_small) fb.tile_msd_fail_d = d_est ? d_est : 1u;
    if (f.sizing) fb.tile_msd_fail_d = 0;
    // Measured at 1 M (gpurun_out/r05c/kt_1m.txt): the 1020 buckets of ~2 500 pairs cost the bucket kernel 22 us (one
    // 1024-thread workgroup with 157 KB of LDS per bucket: four rounds of workgroups whose fixed costs dominate) and
    // the 10-bit first pass 6 us more than the 7-bit one — 60 us against the LSD sort's 55.  So the renderer does
    // not choose it by itself (GS3D_TILE_MSD_AUTO=1 lets it); pinned, it is exact (tests/test_gpu_msd_sort.py).
    if (pinned >= 0) return pinned != 0;
    return sw.tile_msd_auto && d_est <= (uint64_t)P.bkt_cap_small * 256u &&
           (fb.tile_msd_fail_d == 0 || d_est < fb.tile_msd_fail_d - fb.tile_msd_fail_d / 4u);
}

// once the pair buffers have their size: the pair bound of the frame's rounds, whether two rounds remain, the tile sort
inline void plan_pairs(const History &h, const FrameNums &f, uint64_t pair_capacity, const Requests &req, const Switches &sw,
                       const PolicyParams &P, SortFeedback &sfb, RoundsFeedback &rfb, FramePlan &plan) {
    plan.capacity = plan_round_capacity(h, f, pair_capacity, plan.two_round, plan.round_k, rfb);
    if (!plan.capacity) plan.two_round = false;
    plan.tile_msd = !plan.two_round && plan_tile_msd(h, f, req, sw, P, plan.capacity, sfb);
}

// Tile ranges, three ways (the MSD-first tile sort has written them already: k_bucket_sort).  (1) One pass over the sorted keys (k_tile_ranges).  (2) A 32-ary search per tile
// (k_tile_ranges_search) once reading every key again costs more than a few dependent probes per tile: from
// a pair capacity of 8 M (GS3D_RANGES_SEARCH=0/1 forces).  (3) The same search run by the blend workgroups
// themselves (blend_tile_range_wg): no launch in front of the blend, but a workgroup that waits for its
// probes is occupancy the VALU-bound blend misses — same-box A/B (gpurun_out/r04l/ab.log): blend +3.5 us at
// 1 M and 10 M, +10 us at 4K, +12 us at 50 M against 6.8 / 10.5 / 35 / 19 us of range kernel saved: frames
// +1.5 % at 1 M, +-0 at 10 M, -0.5 % at 50 M, -2.3 % at 4K.  It is taken where it pays: images of more than
// 16384 tiles, where neither stand-alone kernel is cheap (GS3D_RANGES_IN_BLEND=0/1 forces).
// Lane groups per wave of the grouped blend (k_blend_grouped<MODE, G>), unless GS3D_BLEND_GROUPS pins them.  4x4 blocks (G = 8)
// walk 15 % fewer wave-steps than 8x4 blocks (G = 4) and test every staged splat against 16 blocks instead of 8.  Measured,
// same box, alternating processes.  Single-round frames, 1 M at 1080p, 3 frames in flight, 5 pairs: 0.2508-0.2550 ms against
// 0.2623-0.2654; one stream: blend 185.8 against 197.3 us, SQ_INSTS_VALU 0.977e8 against 1.02e8.  Two-round frames, whose deep
// tiles skip most steps with finished pixels, so that the staging weighs more (blend stage, G = 4 / G = 8): 10 M 0.2122 / 0.2125,
// 10 M at 4K 0.5131 / 0.5245, 50 M 0.2316 / 0.2438 ms.  So: 8 on single-round frames, 4 on the rounds of a two-round frame.
// round: 0 the frame's only one, else 1 or 2
inline int plan_blend_groups(const Switches &sw, uint32_t round) {
    if (sw.blend_groups != 0) return sw.blend_groups;
    return round != 0u ? 4 : 8;
}

// The grouped blend's choice between the two forms of its trip loop (k_blend_grouped, TileKeys::free_min_live): a wave runs a
// batch branch-free while at least this many of its 128 pixels are live.  rule: gs::BLEND_FREE_MIN_LIVE.  GS3D_BLEND_FREE_BODY=0
// pins the branchy form (129: no wave has that many), =1 the branch-free one (0).
inline uint32_t plan_blend_free_min_live(const Switches &sw, uint32_t rule) {
    return sw.blend_free_body < 0 ? rule : sw.blend_free_body != 0 ? 0u : 129u;
}

// round: 0 the frame's only one, else 1 or 2
inline RangeMode plan_ranges(const FrameNums &f, const Switches &sw, uint32_t capacity, bool tile_msd, uint32_t round) {
    // (a two-round frame: always — the range array is cleared once per frame, and a launch per round is saved)
    const bool ranges_in_blend = round != 0u || (sw.ranges_in_blend >= 0 ? sw.ranges_in_blend != 0 : f.num_tiles > 16384u);
    const bool ranges_search = sw.ranges_search >= 0 ? sw.ranges_search != 0 : capacity >= (8u << 20);
    if (tile_msd || !capacity) return RANGES_NONE;
    return ranges_in_blend ? RANGES_IN_BLEND : ranges_search ? RANGES_SEARCH : RANGES_PASS;
}

// Where a wave of k_pairs_emit starts: found by the wave itself (a search over the super-chunk
// sums: one step per 256 of them) or looked up in a table that k_pairs_cursors writes first.
// The table costs a launch and wins once the search needs more than one step (A/B on one box:
// 1 M 0.369 vs 0.366 ms, 10 M 1.227 vs 1.226, 50 M 4.60 vs 4.80).  GS3D_CURSOR_KERNEL=0/1 forces.
inline bool plan_cursor_kernel(const Switches &sw, uint32_t sb_bound) { return sw.cursor_kernel >= 0 ? sw.cursor_kernel != 0 : sb_bound > 256u; }

}   // namespace gsp
