// The frame plan (wgpu-3dgs-core_amd/csrc/gs_policy.h) on the CPU: every rule as the code states it, with the constants
// of the kernels (gs_render_kernels.h: BKT_CAP = 1024 * 30, BKT_CAP_SMALL = 256 * 32, MSD_TOP_BITS = 10, RADIX_BITS_MAX = 9).
// Built and run by tests/test_policy.py.
#include <cstdio>
#include <cstdlib>

#include "gs_policy.h"

using namespace gsp;

static int g_failed = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

static const PolicyParams P = {30720u, 8192u, 10u, 9u};

static Report report(uint32_t gen, uint64_t pairs, uint32_t visible, uint32_t epoch = 1, uint32_t rounds = 1, uint32_t round_k = 0) {
    Report p;
    p.gen = gen;
    p.pairs = pairs;
    p.visible = visible;
    p.shape_epoch = epoch;
    p.rounds = rounds;
    p.round_k = round_k;
    return p;
}

// a 10 M scene at 1080p, depth planes 0.1 / 100 (27 key bits), steady state
static FrameNums nums_10m() {
    FrameNums f;
    f.n = 10000000u;
    f.gen = 100;
    f.num_tiles = 120 * 68;
    f.tiles_y = 68;
    f.band_rows = 68;
    f.band_tiles = 120 * 68;
    f.dbits = 27;
    f.tile_bits = 13;
    f.pair_capacity = 40000000ull;
    f.pod_bytes = 224;
    f.has_sh = true;
    f.has_order = true;
    return f;
}

static void test_history() {
    History h;
    h.shape_epoch = 3;
    CHECK(h.newest() == nullptr && h.newest_any() == nullptr);
    h.rep[0] = report(7, 100, 10, 3);
    h.rep[1] = report(8, 200, 20, 2);         // the newer report belongs to another shape
    CHECK(h.newest_any() == &h.rep[1]);
    CHECK(h.newest() == nullptr);             // ... so there is none of this shape: the older one is NOT consulted
    h.rep[1].shape_epoch = 3;
    CHECK(h.newest() == &h.rep[1]);
    h.rep[0].gen = 9;
    CHECK(h.newest() == &h.rep[0]);
}

static void test_capacity() {
    CHECK(capacity_for(1000000) == 1000000 + 250000 + 65536);
    History h;
    h.shape_epoch = 1;
    // head room of 1/8 or more: the capacity stays
    h.rep[0] = report(5, 8000000, 1);
    CHECK(plan_capacity(h, 9000000) == 9000000);
    CHECK(plan_capacity(h, 8000000 + 8000000 / 8) == 9000000);
    // less: grows to d + d/4 + 65536
    CHECK(plan_capacity(h, 8999999) == capacity_for(8000000));
    // trend: consecutive generations of this shape, three steps ahead
    h.rep[1] = report(6, 9000000, 1);
    CHECK(plan_capacity(h, 20000000) == 20000000);                 // 12 M ahead still fits
    CHECK(plan_capacity(h, 12000000) == capacity_for(12000000));  // 9 M + 3 x 1 M, less than 1/8 of head room
    // capped at twice the newest count
    h.rep[0] = report(5, 1000000, 1);
    CHECK(plan_capacity(h, 12000000) == capacity_for(18000000));
    // not consecutive: no trend
    h.rep[0] = report(4, 8000000, 1);
    CHECK(plan_capacity(h, 12000000) == 12000000);
    // another shape epoch: no trend.  (a change of the ROUND mode between the two reports is not
    // looked at — a two-round report's pairs against a single-round one's are extrapolated all the same; stated, not wanted.)
    h.rep[0] = report(5, 8000000, 1, 2);
    CHECK(plan_capacity(h, 12000000) == 12000000);
    h.rep[0] = report(5, 8000000, 1, 1, 2, 4096);
    CHECK(plan_capacity(h, 12000000) == capacity_for(12000000));
    // a falling count is not extrapolated
    h.rep[0] = report(7, 8000000, 1);
    CHECK(plan_capacity(h, 12000000) == 12000000);
}

static void test_depth_msd() {
    const Switches sw;
    Requests req;
    FrameNums f = nums_10m();
    History h;
    h.shape_epoch = 1;
    SortFeedback fb;
    // a sizing frame guesses from N: up to 4 Mi
    f.sizing = true;
    CHECK(!plan_depth_msd(h, f, req, sw, P, fb) && !fb.depth_msd);
    f.n = 4u << 20;
    CHECK(plan_depth_msd(h, f, req, sw, P, fb) && fb.depth_msd);
    f.n = (4u << 20) + 1;
    CHECK(!plan_depth_msd(h, f, req, sw, P, fb));
    // frames in flight keep the guess
    f.sizing = false;
    fb.depth_msd = true;
    CHECK(plan_depth_msd(h, f, req, sw, P, fb));
    // hysteresis: stays up to BKT_CAP, leaves above, re-enters at or below 7/8 of it
    // (the bucket size an LSD frame reports is compared like an MSD frame's; stated, not wanted)
    h.rep[0] = report(5, 1, 1);
    h.rep[0].depth_bucket_max = 30720;
    CHECK(plan_depth_msd(h, f, req, sw, P, fb) && fb.depth_bucket_seen == 30720);
    h.rep[0].depth_bucket_max = 30721;
    CHECK(!plan_depth_msd(h, f, req, sw, P, fb));
    h.rep[0].depth_bucket_max = 30720 - 30720 / 8 + 1;
    CHECK(!plan_depth_msd(h, f, req, sw, P, fb));
    h.rep[0].depth_bucket_max = 30720 - 30720 / 8;
    CHECK(plan_depth_msd(h, f, req, sw, P, fb));
    // key bits: 11..28
    f.dbits = 10;
    CHECK(!plan_depth_msd(h, f, req, sw, P, fb));
    f.dbits = 29;
    CHECK(!plan_depth_msd(h, f, req, sw, P, fb));
    f.dbits = 28;
    CHECK(plan_depth_msd(h, f, req, sw, P, fb));
    // precedence: the API's request, then the environment, then the renderer
    Switches env;
    env.depth_msd = 0;
    CHECK(!plan_depth_msd(h, f, req, env, P, fb));
    req.depth_msd = 1;
    CHECK(plan_depth_msd(h, f, req, env, P, fb));
    req.depth_msd = 0;
    env.depth_msd = 1;
    CHECK(!plan_depth_msd(h, f, req, env, P, fb));
}

static void test_rounds() {
    const Switches sw;
    Requests req;
    FrameNums f = nums_10m();
    History h;
    h.shape_epoch = 1;
    RoundsFeedback fb;
    fb.rounds_epoch = 1;
    uint32_t k = 0;
    // a deep scene: 24 M pairs of 7 M visible over 8160 tiles (2 941 per tile): round 1 of 250 pairs per tile
    h.rep[0] = report(99, 24000000, 7000000);
    CHECK(plan_rounds(h, f, req, sw, fb, k));
    const double k_auto = 7000000.0 * 250.0 / (24000000.0 / 8160.0);
    CHECK(k == ((uint64_t)k_auto + 2047) / 2048 * 2048 && k % 2048 == 0);
    CHECK(fb.auto_deep && fb.full_pairs == 24000000 && fb.full_pairs_v == 7000000);
    // too few pairs in all, or per tile: one round
    h.rep[0] = report(99, 11999999, 7000000);
    CHECK(!plan_rounds(h, f, req, sw, fb, k));
    // frames in flight: the last choice stands
    History none;
    none.shape_epoch = 1;
    fb.auto_deep = true;
    fb.auto_k = 5000;
    CHECK(plan_rounds(none, f, req, sw, fb, k) && k == 6144);
    // round_k is rounded up to 2048, and two rounds are dropped when it reaches N
    req.rounds = 1;
    req.round1 = 2049;
    CHECK(plan_rounds(none, f, req, sw, fb, k) && k == 4096);
    req.round1 = f.n - 1;
    CHECK(!plan_rounds(none, f, req, sw, fb, k) && k == 0);
    // pinned without a length and without the renderer's own: a quarter of the visible ones
    req.round1 = 0;
    fb.auto_deep = false;
    h.rep[0] = report(99, 1000000, 800000);
    CHECK(plan_rounds(h, f, req, sw, fb, k) && k == (800000 / 4 + 2047) / 2048 * 2048);
    // the API beats the environment
    Switches env;
    env.rounds = 1;
    env.round1 = 8192;
    req.rounds = 0;
    CHECK(!plan_rounds(h, f, req, env, fb, k));
    req.rounds = -1;
    CHECK(plan_rounds(h, f, req, env, fb, k) && k == 8192);
    // small frames and the ungrouped blend never take two rounds
    f.n = 4096;
    CHECK(!plan_rounds(h, f, req, env, fb, k));
    f = nums_10m();
    env.blend_groups = 1;
    CHECK(!plan_rounds(h, f, req, env, fb, k));
}

static void test_rounds_feedback() {
    const Switches sw;
    const Requests req;
    FrameNums f = nums_10m();
    History h;
    h.shape_epoch = 1;
    RoundsFeedback fb;
    fb.rounds_epoch = 1;
    fb.full_pairs = 24000000;
    fb.full_pairs_v = 7000000;
    uint32_t k = 0;
    // under 60 % of the tiles with pairs finished: the scale grows by 1.5, once per report
    h.rep[0] = report(90, 3000000, 7000000, 1, 2, 614400);
    h.rep[0].tiles_done = 59;
    h.rep[0].tiles_open = 41;
    plan_rounds(h, f, req, sw, fb, k);
    CHECK(fb.round_scale == 1.5f && fb.rounds_fb_gen == 90);
    plan_rounds(h, f, req, sw, fb, k);
    CHECK(fb.round_scale == 1.5f);
    h.rep[0].tiles_done = 60;
    h.rep[0].tiles_open = 40;
    h.rep[0].gen = 91;
    plan_rounds(h, f, req, sw, fb, k);
    CHECK(fb.round_scale == 1.5f);            // 60 %: long enough
    // at most a tenth left open: a little longer
    h.rep[0].tiles_done = 90;
    h.rep[0].tiles_open = 10;
    h.rep[0].gen = 92;
    plan_rounds(h, f, req, sw, fb, k);
    CHECK(fb.round_scale == 1.5f * 1.25f);
    // past 3.4 the rounds go off ...
    fb.round_scale = 2.3f;
    h.rep[0].tiles_done = 1;
    h.rep[0].tiles_open = 99;
    h.rep[0].gen = 93;
    f.gen = 1000;
    CHECK(!plan_rounds(h, f, req, sw, fb, k));
    CHECK(fb.rounds_off && fb.rounds_off_gen == 1000 && fb.round_scale == 2.3f * 1.5f);
    // ... and come back 512 frames later
    h.rep[0] = report(1500, 24000000, 7000000);
    f.gen = 1512;
    CHECK(!plan_rounds(h, f, req, sw, fb, k) && fb.rounds_off);
    f.gen = 1513;
    plan_rounds(h, f, req, sw, fb, k);
    CHECK(!fb.rounds_off && fb.round_scale == 1.0f);
    // a new shape epoch: the feedback starts over
    fb.round_scale = 2.0f;
    fb.rounds_off = true;
    h.shape_epoch = 2;
    plan_rounds(h, f, req, sw, fb, k);
    CHECK(fb.rounds_epoch == 2 && fb.round_scale == 1.0f && !fb.rounds_off);
}

static void test_partition_and_bound() {
    Switches sw;
    FrameNums f = nums_10m();
    History h;
    h.shape_epoch = 1;
    RoundsFeedback fb;
    // from 32 Mi Gaussians, or when round 1 finished every tile
    CHECK(!plan_partition(h, f, sw, P, true, fb));
    f.n = 32u << 20;
    CHECK(plan_partition(h, f, sw, P, true, fb));
    CHECK(!plan_partition(h, f, sw, P, false, fb));
    f.sizing = true;
    CHECK(!plan_partition(h, f, sw, P, true, fb));
    f = nums_10m();
    h.rep[0] = report(9, 3000000, 7000000, 1, 2, 4096);
    h.rep[0].tiles_done = f.band_tiles;
    CHECK(plan_partition(h, f, sw, P, true, fb) && fb.auto_all_done);
    h.rep[0].tiles_open = 1;
    CHECK(!plan_partition(h, f, sw, P, true, fb));
    sw.round_partition = 1;
    CHECK(plan_partition(h, f, sw, P, true, fb));
    f.dbits = 10;
    CHECK(!plan_partition(h, f, sw, P, true, fb));

    // the per-round bound: only from a two-round report with the same round_k
    f = nums_10m();
    fb = RoundsFeedback();
    h.rep[0] = report(9, 3000000, 7000000, 1, 2, 4096);
    h.rep[0].round_pairs_max = 1000000;
    CHECK(plan_round_capacity(h, f, 40000000, true, 4096, fb) == capacity_for(2000000));
    CHECK(fb.round_cap == capacity_for(2000000) && fb.round_cap_k == 4096);
    CHECK(plan_round_capacity(h, f, 40000000, true, 6144, fb) == 40000000);      // another round 1: the buffers' capacity
    CHECK(fb.round_cap == 0);
    // (a report whose round 2 was skipped carries round 1's count alone as round_pairs_max and bounds
    // the next frame's round 2 with it; stated, not wanted)
    h.rep[0].rounds = 1;
    CHECK(plan_round_capacity(h, f, 40000000, true, 4096, fb) == 40000000);
    CHECK(plan_round_capacity(h, f, 40000000, false, 0, fb) == 40000000);
    // frames in flight: the last bound stands
    History none;
    none.shape_epoch = 1;
    fb.round_cap = 3000000;
    fb.round_cap_k = 4096;
    CHECK(plan_round_capacity(none, f, 40000000, true, 4096, fb) == 3000000);
    CHECK(plan_round_capacity(none, f, 40000000, true, 2048, fb) == 40000000);
}

static void test_small_choices() {
    Switches sw;
    Requests req;
    FrameNums f = nums_10m();
    History h;
    h.shape_epoch = 2;
    // the block list: a band without a report; with one, less than half visible — whatever the report's shape
    CHECK(!plan_use_list(h, f, sw));
    f.band_rows = 8;
    CHECK(plan_use_list(h, f, sw));
    h.rep[0] = report(4, 1, 6000000, 1);
    CHECK(!plan_use_list(h, f, sw));
    h.rep[0].visible = 4999999;
    CHECK(plan_use_list(h, f, sw));
    sw.block_list = 0;
    CHECK(!plan_use_list(h, f, sw));
    // tile masks: records of 200 bytes in a mirror beyond 512 MiB, or pinned (API first)
    sw = Switches();
    CHECK(plan_tile_masks(true, 10000000, 224, req, sw));
    CHECK(!plan_tile_masks(true, 1000000, 224, req, sw));
    CHECK(!plan_tile_masks(true, 50000000, 144, req, sw));
    CHECK(!plan_tile_masks(false, 10000000, 224, req, sw));
    sw.tile_masks = 0;
    CHECK(!plan_tile_masks(true, 10000000, 224, req, sw));
    req.tile_masks = 1;
    CHECK(plan_tile_masks(true, 10000000, 224, req, sw));
    // ranges: in the blend for rounds and above 16384 tiles, the search from 8 Mi pairs, nothing behind the MSD-first sort
    sw = Switches();
    f = nums_10m();
    CHECK(plan_ranges(f, sw, 1u << 20, false, 0) == RANGES_PASS);
    CHECK(plan_ranges(f, sw, 8u << 20, false, 0) == RANGES_SEARCH);
    CHECK(plan_ranges(f, sw, 8u << 20, false, 1) == RANGES_IN_BLEND);
    CHECK(plan_ranges(f, sw, 8u << 20, true, 0) == RANGES_NONE);
    f.num_tiles = 16385;
    CHECK(plan_ranges(f, sw, 1u << 20, false, 0) == RANGES_IN_BLEND);
    // the tile sort: never by itself, exact when pinned, u16 ids of more than 10 bits only
    SortFeedback sfb;
    f = nums_10m();
    req = Requests();
    CHECK(!plan_tile_msd(h, f, req, sw, P, 1u << 20, sfb));
    req.tile_msd = 1;
    CHECK(plan_tile_msd(h, f, req, sw, P, 1u << 20, sfb));
    f.tile_bits = 10;
    CHECK(!plan_tile_msd(h, f, req, sw, P, 1u << 20, sfb));
    // the whole plan of a steady 1 M frame: MSD-first depth sort kept, one round, index-order preprocess choices
    f = nums_10m();
    f.n = 1000000;
    f.pod_bytes = 48;
    f.has_sh = false;
    f.pair_capacity = 4000000;
    History h1;
    h1.shape_epoch = 1;
    h1.rep[1] = report(50, 2400000, 700000);
    h1.rep[1].depth_bucket_max = 5000;
    RoundsFeedback rfb;
    rfb.rounds_epoch = 1;
    FramePlan plan;
    sfb = SortFeedback();
    sfb.depth_msd = true;
    plan_frame(h1, f, Requests(), sw, P, sfb, rfb, plan);
    CHECK(plan.depth_msd && !plan.two_round && !plan.partition && !plan.banded && !plan.block_cull && plan.nt_loads == 0 &&
          plan.mask_culled_records == 1 && plan.want_capacity == 4000000);
    plan_pairs(h1, f, 4000000, Requests(), sw, P, sfb, rfb, plan);
    CHECK(plan.capacity == 4000000 && !plan.tile_msd);
}

int main() {
    test_history();
    test_capacity();
    test_depth_msd();
    test_rounds();
    test_rounds_feedback();
    test_partition_and_bound();
    test_small_choices();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("policy OK\n");
    return 0;
}
