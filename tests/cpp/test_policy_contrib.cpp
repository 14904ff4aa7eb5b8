// Contribution frames (gs_render_frame_contrib) in the frame plan (wgpu-3dgs-core_amd/csrc/gs_policy.h):
// Requests::single_round plans ONE round under every pin, environment switch and feedback state, exactly as a frame
// under gs_renderer_set_rounds(r, 0, 0) is planned — the same plan, and the same RoundsFeedback left behind.
// Built and run by tests/test_policy_contrib.py.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

static bool same(const RoundsFeedback &a, const RoundsFeedback &b) {
    return a.full_pairs == b.full_pairs && a.full_pairs_v == b.full_pairs_v && a.rounds_epoch == b.rounds_epoch &&
           a.rounds_fb_gen == b.rounds_fb_gen && a.round_scale == b.round_scale && a.rounds_off == b.rounds_off &&
           a.rounds_off_gen == b.rounds_off_gen && a.round_cap == b.round_cap && a.round_cap_k == b.round_cap_k &&
           a.auto_deep == b.auto_deep && a.auto_all_done == b.auto_all_done && a.auto_k == b.auto_k;
}

static int g_cases = 0, g_would_take_two = 0;

// one state: the contribution request against the frame pinned to one round
static void check_state(const History &h, const FrameNums &f, const Requests &pin, const Switches &sw, const RoundsFeedback &fb0) {
    g_cases++;
    {   // (is this a state in which the renderer's pin would take two rounds?)
        RoundsFeedback fb = fb0;
        uint32_t k = 0;
        if (plan_rounds(h, f, pin, sw, fb, k)) g_would_take_two++;
    }
    Requests contrib = pin;
    contrib.single_round = true;
    Requests one = pin;
    one.rounds = 0;
    one.round1 = 0;
    RoundsFeedback fa = fb0, fb = fb0;
    uint32_t ka = 77, kb = 78;
    const bool ta = plan_rounds(h, f, contrib, sw, fa, ka), tb = plan_rounds(h, f, one, sw, fb, kb);
    CHECK(!ta && !tb);
    CHECK(ka == kb);
    CHECK(same(fa, fb));
    // ... and through the whole plan
    FramePlan pa, pb;
    SortFeedback sa, sb;
    RoundsFeedback ra = fb0, rb = fb0;
    plan_frame(h, f, contrib, sw, P, sa, ra, pa);
    plan_frame(h, f, one, sw, P, sb, rb, pb);
    plan_pairs(h, f, f.pair_capacity, contrib, sw, P, sa, ra, pa);
    plan_pairs(h, f, f.pair_capacity, one, sw, P, sb, rb, pb);
    CHECK(!pa.two_round && !pa.partition && pa.capacity == (uint32_t)f.pair_capacity);
    CHECK(pa.two_round == pb.two_round && pa.partition == pb.partition && pa.round_k == pb.round_k && pa.capacity == pb.capacity &&
          pa.depth_msd == pb.depth_msd && pa.tile_msd == pb.tile_msd && pa.use_list == pb.use_list && pa.want_capacity == pb.want_capacity);
    CHECK(same(ra, rb));
    CHECK(sa.depth_msd == sb.depth_msd);
}

int main() {
    // histories: a deep single-round report (the renderer itself would choose two rounds), a two-round report whose round 1
    // was too short (feedback pending), one that finished every tile, a shallow scene, frames in flight (no report)
    History deep, short2, done2, shallow, none;
    for (History *h : {&deep, &short2, &done2, &shallow, &none}) h->shape_epoch = 1;
    deep.rep[0] = report(99, 24000000, 7000000);
    short2.rep[0] = report(99, 3000000, 7000000, 1, 2, 614400);
    short2.rep[0].tiles_done = 10;
    short2.rep[0].tiles_open = 90;
    short2.rep[0].round_pairs_max = 2000000;
    done2.rep[0] = report(99, 3000000, 7000000, 1, 2, 614400);
    done2.rep[0].tiles_done = 120 * 68;
    done2.rep[0].round_pairs_max = 2000000;
    shallow.rep[0] = report(99, 1000000, 800000);
    // feedback states: fresh, "deep, two rounds chosen", switched off, scaled up, another epoch
    RoundsFeedback fresh, chosen, off, scaled, stale;
    for (RoundsFeedback *fb : {&fresh, &chosen, &off, &scaled}) fb->rounds_epoch = 1;
    chosen.full_pairs = 24000000;
    chosen.full_pairs_v = 7000000;
    chosen.auto_deep = true;
    chosen.auto_k = 600000;
    chosen.auto_all_done = true;
    chosen.round_cap = 5000000;
    chosen.round_cap_k = 614400;
    off = chosen;
    off.rounds_off = true;
    off.rounds_off_gen = 50;
    off.round_scale = 3.45f;
    scaled = chosen;
    scaled.round_scale = 2.25f;
    stale = chosen;
    stale.rounds_epoch = 7;
    const int pins[3] = {-1, 0, 1};
    const uint32_t lens[3] = {0u, 2049u, 614400u};
    for (const History *h : {&deep, &short2, &done2, &shallow, &none})
        for (const RoundsFeedback *fb : {&fresh, &chosen, &off, &scaled, &stale})
            for (int pin : pins)
                for (uint32_t len : lens)
                    for (int env = 0; env < 3; env++)
                        for (int sizing = 0; sizing < 2; sizing++) {
                            Requests req;
                            req.rounds = pin;
                            req.round1 = len;
                            Switches sw;
                            if (env == 1) sw.rounds = 1;
                            if (env == 2) { sw.rounds = 1; sw.round1 = 8192; }
                            FrameNums f = nums_10m();
                            f.sizing = sizing != 0;
                            check_state(*h, f, req, sw, *fb);
                        }
    // the states above do include frames that would otherwise take two rounds: the renderer's own choice among them
    CHECK(g_would_take_two > 100);
    {
        RoundsFeedback fb = chosen;
        uint32_t k = 0;
        Requests own;
        CHECK(plan_rounds(deep, nums_10m(), own, Switches(), fb, k) && k != 0);      // "deep, two rounds chosen" ...
        own.single_round = true;
        fb = chosen;
        CHECK(!plan_rounds(deep, nums_10m(), own, Switches(), fb, k));               // ... and the contribution frame of that renderer
        // it leaves the feedback as a single-round frame of that shape would: the deep choice is still recorded for the next frame
        CHECK(fb.auto_deep && fb.full_pairs == 24000000 && fb.full_pairs_v == 7000000);
    }
    if (g_failed) {
        std::printf("%d checks failed (%d states)\n", g_failed, g_cases);
        return 1;
    }
    std::printf("policy contrib OK (%d states, %d of them two rounds under their pin)\n", g_cases, g_would_take_two);
    return 0;
}
