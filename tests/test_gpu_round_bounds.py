"""The per-round pair bound of two-round frames and their skip path (DESIGN.md §4.2 "rounds", §4.5; gsp::plan_round_capacity,
publish_pairs).  From its second frame on, each round of a two-round frame is bounded by capacity_for(2 * round_pairs_max) of
the newest two-round report with the same round-1 length — usually far below the pair buffers' capacity — and a round that
outgrows the bound skips the whole frame.  Here one renderer renders short SEQUENCES of frames of one shape (n, image size,
band) whose pair counts jump, by the size of the Gaussian transform or by a swap to another buffer of the same length, so
that round 1 or round 2 outgrows the bound (or the buffers), and every frame — the skipped one included — is compared with
the CPU oracle or with the poison the test wrote.

Every figure a sequence rests on is the oracle's and is asserted without a GPU (test_the_oracle_counts_make_...): the pairs
D1 / D2 of each round, the bound B the jump frame is planned with, and which round outgrows it.  The buffer `T` is
TRANSLUCENT (the oracle's alpha stays below 1 - 1e-4 at every pixel): no pixel ever stops, round 1 finishes no tile, round 2
drops nothing, so D1 + D2 = D exactly.  Round 1 of an unpartitioned frame (a renderer's first, or GS3D_ROUND_PARTITION=0) is
the nearest K visible Gaussians in stable depth order; round 1 of a partitioned frame is everything in front of the first
boundary of the depth key's top 10 bits with at least K Gaussians in front of it (k_round_threshold) — round1_members models
both.  tests/conftest.py pins GS3D_ROUND_PARTITION=1; one child process (this file as a script) runs three of the sequences
under GS3D_ROUND_PARTITION=0 and hands its frames back in an .npz that the parent compares with the same oracle frames."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gpu_child  # noqa: E402
import helpers  # noqa: E402
from helpers import POISON, band_rows, bits, capacity_for  # noqa: E402
from round_kinds import (BAND, BAND_TILES, BUFFERS, H, KINDS, N, ROT_SCALE, SH_NONE, TILES_X, TILES_Y, W, host_buffer,  # noqa: E402
                         kind_transforms, oracle_kind, round1_frame, round_counts)

gpu = pytest.mark.gpu

PAIR_OVERFLOW, SKIPPED = 1, 2                      # gs_frame_result.flags
FLAGS_POISON = 0xDEAD
TRANSLUCENT = ("small", "big")
# name: K = set_rounds(1, K) of every frame, the kinds in order, the index of the frame whose pairs jump, and the round of it
# that outgrows the bound first
SEQUENCES = {
    # the bound shrinks to B = capacity_for(2 * D2_small) inside buffers sized for `big`; D1_big <= B < D2_big
    "round2": dict(K=2048, frames=["big", "small", "small", "big", "big"], jump=3, over=2),
    # ... with a round 1 long enough that D1_big > B
    "round1": dict(K=16384, frames=["big", "small", "small", "big", "big"], jump=3, over=1),
    # the sizing frame is `small`: the bound of the jump frame is the buffers' capacity, capacity_for(D_small)
    "buffers2": dict(K=2048, frames=["small", "big", "big"], jump=1, over=2),
    "buffers1": dict(K=16384, frames=["small", "big", "big"], jump=1, over=1),
    # round 1 of `cover` finishes every tile, k_round2_gate skips round 2 and round_pairs_max is round 1's count alone:
    # B = capacity_for(2 * D1_cover); then the tiles open: D1_big <= B < D2_big; and back
    "gated": dict(K=2048, frames=["cover", "cover", "cover", "big", "big", "cover"], jump=3, over=2),
}
CHILD_SEQUENCES = ["round2", "round1", "gated"]


def predict(ob, name, partition):
    """What gs_policy.h makes of a sequence when every frame's report is at hand before the next frame is planned: per
    frame its kind, whether it is partitioned, the oracle's V, D, D1, D2; for the jump frame also the bound of its rounds,
    B = min(capacity_for(2 * round_pairs_max of the frame before), the buffers' capacity), and the buffers' capacity
    capacity_for(D of the sizing frame) — no frame before the jump grows them (plan_capacity: no report leaves less
    than 1/8 of head room, no rising trend of more than a few per cent)."""
    seq = SEQUENCES[name]
    K, out = seq["K"], []
    for i, kind in enumerate(seq["frames"]):
        o = oracle_kind(ob, kind)
        part = bool(partition) and i > 0          # a renderer's first frame sizes the buffers: never partitioned
        d1, d2 = round_counts(ob, kind, K, part)
        out.append(dict(kind=kind, part=part, V=o["V"], D=o["D"], D1=d1, D2=d2))
    j = seq["jump"]
    before = out[j - 1]
    # the frame before the jump: a translucent frame emits D2 in round 2; `cover`'s round 2 is gated (asserted on the
    # device: tiles_done == BAND_TILES and pairs == D1) and emits nothing
    rpm = max(before["D1"], before["D2"]) if before["kind"] in TRANSLUCENT else before["D1"]
    out[j]["capacity"] = capacity_for(out[0]["D"])
    out[j]["B"] = min(capacity_for(2 * rpm), out[j]["capacity"])
    return out


@pytest.mark.parametrize("kind", TRANSLUCENT)
def test_the_translucent_kinds_stop_no_pixel(ob, kind):
    """the condition under which D1 + D2 = D: a pixel stops when its T would fall below 1e-4; the oracle's alpha = 1 - T
    stays below 1 - 1e-4 everywhere, so none does, round 1 finishes no tile and round 2 drops no Gaussian"""
    o = oracle_kind(ob, kind)
    y0, y1 = band_rows(BAND, H)
    a = o["rgba"][y0:y1, :, 3]
    print("%s: V %d, D %d, alpha %.6f .. %.6f" % (kind, o["V"], o["D"], a.min(), a.max()))
    assert a.max() < 1.0 - 1e-4
    assert a.max() > 0.25, "a frame this faint checks little"


@pytest.mark.parametrize("partition", [1, 0])
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_the_oracle_counts_make_the_sequence_what_its_name_says(ob, name, partition):
    seq, p = SEQUENCES[name], predict(ob, name, partition)
    K, j = seq["K"], seq["jump"]
    for i, f in enumerate(p):
        print("%s, partition %d, frame %d %-5s: V %d D %d D1 %d D2 %d%s" % (
            name, partition, i, f["kind"], f["V"], f["D"], f["D1"], f["D2"],
            "  B %d, buffers %d" % (f["B"], f["capacity"]) if i == j else ""))
        assert K < f["V"] < N and 0 < f["D1"] < f["D"], "both rounds must have something to do"
    jump, B = p[j], p[j]["B"]
    for f in p[:j]:
        # the frames before the jump fit: their own bound is at least capacity_for(D) (2 * max(D1, D2) >= D) or the buffers'
        assert f["D"] <= jump["capacity"]
    if name in ("round2", "gated"):
        assert jump["D1"] <= B < jump["D2"] <= jump["capacity"]
        assert B < jump["capacity"], "the bound must lie inside the buffers"
    elif name == "round1":
        assert B < jump["D1"] <= jump["capacity"] and B < jump["capacity"]
    elif name == "buffers2":
        assert B == jump["capacity"] == capacity_for(p[0]["D"]) and jump["D1"] <= B < jump["D2"]
    elif name == "buffers1":
        assert B == jump["capacity"] == capacity_for(p[0]["D"]) and B < jump["D1"]
    assert seq["over"] == (1 if jump["D1"] > B else 2 if jump["D2"] > B else 0)
    if name == "gated":
        assert p[j - 1]["kind"] == "cover" and B == capacity_for(2 * p[j - 1]["D1"])
        assert B < capacity_for(2 * max(p[j - 1]["D1"], p[j - 1]["D2"])), "a round 2 that ran would have hidden the jump"
    else:
        assert B == min(capacity_for(2 * max(p[j - 1]["D1"], p[j - 1]["D2"])), jump["capacity"])
    # the recovery: the report of the skipped frame carries both rounds' true counts, so the next bound holds both
    assert min(capacity_for(2 * max(jump["D1"], jump["D2"])), capacity_for(jump["D"])) >= max(jump["D1"], jump["D2"])


# ------------------------------------------------------------------------------------------------
# the device's side
# ------------------------------------------------------------------------------------------------

INFO = ["word", "flags", "visible", "pairs", "pair_capacity", "rounds", "round1", "tiles_done", "partitioned", "raised", "e_pairs",
        "e_capacity", "e_round"]


class Rig:
    """the two buffers, one poisoned target with its planes and the device word of the frame flags"""

    def __init__(self, gs, ob, device, stream):
        from planes import Planes
        self.gs, self.ob, self.device, self.stream = gs, ob, device, stream
        pod = gs.GaussianPod(SH_NONE, ROT_SCALE)
        self.bufs = {}
        for b in BUFFERS:
            hb = host_buffer(ob, b)
            pods = pod.from_gaussian(hb["g"])
            assert np.array_equal(np.asarray(pods, dtype=np.uint8).reshape(-1), hb["pods"]), "product pack != oracle pack"
            self.bufs[b] = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
            assert np.array_equal(self.bufs[b].download_order(stream), hb["order"]), "buffer %s: not the oracle's spatial order" % b
        self.planes = Planes(gs, device, W, H)
        self.word = gs.Buffer(device, data=np.full(1, FLAGS_POISON, dtype=np.uint32))
        self.frames = {}
        for kind in KINDS:
            ogt, omt, ocam = kind_transforms(ob, kind)
            self.frames[kind] = (gs.GaussianTransformPod.from_buffer_copy(bytes(ogt)), gs.ModelTransformPod.from_buffer_copy(bytes(omt)),
                                 helpers.copy_camera(ocam, gs.Camera))

    def render(self, r, kind, aux=False, check=False):
        """one frame, enqueued and then waited for explicitly: (FrameResult or None, PairCapacityError or None)"""
        gs, pl = self.gs, self.planes
        pl.poison(self.stream, image=True)
        self.word.write(self.stream, 0, np.full(1, FLAGS_POISON, dtype=np.uint32))
        self.stream.synchronize()
        gt, mt, cam = self.frames[kind]
        kw = dict(band=BAND, check=check)
        if aux:
            kw.update(depth_device_ptr=pl.depth.device_ptr(), pick_device_ptr=pl.pick.device_ptr(), pick_threshold=0.5)
        r.render(self.stream, self.bufs[KINDS[kind][0]], gt, mt, cam, pl.img.device_ptr(), **kw)
        try:
            return r.wait_frame(), None
        except gs.PairCapacityError as e:
            return None, e

    def release(self):
        self.planes.release()
        self.word.release()
        for b in self.bufs.values():
            b.destroy()


def run_sequence(rig, name, aux=False, auto=False):
    """The frames of a sequence on one new renderer; returns {"f<i>/info": INFO's figures, "f<i>/rgba" (, "/depth", "/pick")}.
    aux: with the depth and pick planes.  auto: the jump frame is rendered with check=True (it waits and renders again)."""
    gs, seq, rec = rig.gs, SEQUENCES[name], {}
    r = gs.Renderer(rig.device)
    r.set_rounds(1, seq["K"])
    r.set_frame_flags_target(rig.word.device_ptr())
    for i, kind in enumerate(seq["frames"]):
        fr, e = rig.render(r, kind, aux=aux, check=auto and i == seq["jump"])
        si = r.sort_info()
        rgba, depth, pick = rig.planes.get(rig.stream)
        word = int(rig.word.download(rig.stream, np.uint32)[0])
        e_round = 0 if e is None else 1 if "round 1 " in str(e) else 2 if "round 2 " in str(e) else -1
        info = dict(word=word, flags=fr.flags if fr else -1, visible=fr.visible if fr else -1, pairs=fr.pairs if fr else -1,
                    pair_capacity=fr.pair_capacity if fr else -1, rounds=si.rounds, round1=si.round1, tiles_done=si.tiles_done,
                    partitioned=si.partitioned, raised=int(e is not None), e_pairs=e.pairs if e else -1,
                    e_capacity=e.capacity if e else -1, e_round=e_round)
        print("%s frame %d %-5s: %s" % (name, i, kind, " ".join("%s %d" % (k, info[k]) for k in INFO)), flush=True)
        rec["f%d/info" % i] = np.array([info[k] for k in INFO], dtype=np.int64)
        rec["f%d/rgba" % i] = rgba
        if aux:
            rec["f%d/depth" % i], rec["f%d/pick" % i] = depth, pick
    r.destroy()
    return rec


def check_exact(ob, kind, rgba, ctx):
    o = oracle_kind(ob, kind)
    y0, y1 = band_rows(BAND, H)
    bad = bits(rgba[y0:y1]) != bits(o["rgba"][y0:y1])
    assert not bad.any(), "%s: %d words of the image differ from the oracle's frame" % (ctx, bad.sum())
    assert (rgba[:y0] == POISON).all() and (rgba[y1:] == POISON).all(), "%s: rows outside the band were written" % ctx


def check_round1_state(ob, kind, K, partitioned, rgba, ctx):
    """What a frame skipped by its SECOND round leaves in the caller's image: today's documented contract (include/gs3d.h at
    gs_renderer_set_rounds, the "known defect") — round 1's blend has run, so the band holds round 1's pixel state: rgb is
    the colour sum C of round 1's Gaussians, the alpha word is the final alpha of a pixel that stopped in round 1, or the raw
    transmittance +-T (the sign: still live) of one that did not.  Compared with the oracle's frame of round 1's Gaussians
    alone on background 0: rgb bit for bit (fma(T, 0, C) == C), alpha within 2^-24 either way — the oracle's alpha is
    fl(1 - T) of a T in [0, 1], half an ulp of it is at most 2^-25, the margin one binade.  No NaN; rows outside the band
    keep the poison.  This is round 1's state against an independent computation — the per-round tap the suite lacked.
    WHOEVER REPAIRS THE DEFECT (round 1's state kept in renderer-owned memory until round 2 is known to fit) replaces this
    whole block by "the image == poison", as check_untouched asserts for a frame skipped by its first round."""
    want = round1_frame(ob, kind, K, partitioned)
    y0, y1 = band_rows(BAND, H)
    assert (rgba[:y0] == POISON).all() and (rgba[y1:] == POISON).all(), "%s: rows outside the band were written" % ctx
    got = rgba[y0:y1]
    assert not np.isnan(got).any(), "%s: NaN in the band" % ctx
    bad = bits(got[..., :3]) != bits(want[y0:y1, :, :3])
    assert not bad.any(), "%s: %d rgb words differ from the oracle's frame of round 1's Gaussians" % (ctx, bad.sum())
    a, alpha_o = got[..., 3].astype(np.float64), want[y0:y1, :, 3].astype(np.float64)
    final = np.abs(a - alpha_o) <= 2.0 ** -24
    raw = np.abs((1.0 - np.abs(a)) - alpha_o) <= 2.0 ** -24
    assert (final | raw).all(), "%s: %d alpha words are neither round 1's alpha nor its +-T" % (ctx, (~(final | raw)).sum())


def check_untouched(rgba, ctx):
    assert (bits(rgba) == bits(np.full(1, POISON))[0]).all(), "%s: a frame skipped by its first round must leave the image untouched" % ctx


def check_sequence(ob, name, rec, partition, auto=False):
    """every frame of a recorded sequence against predict() and the oracle's frames"""
    seq, p = SEQUENCES[name], predict(ob, name, partition)
    K, j = seq["K"], seq["jump"]
    for i, f in enumerate(p):
        ctx = "%s (partition %d), frame %d (%s)" % (name, partition, i, f["kind"])
        got = dict(zip(INFO, (int(x) for x in rec["f%d/info" % i])))
        rgba = rec["f%d/rgba" % i]
        assert got["rounds"] == 2 and got["round1"] == K, "%s: %d rounds, round 1 of %d" % (ctx, got["rounds"], got["round1"])
        assert got["partitioned"] == int(f["part"]), "%s: partitioned %d" % (ctx, got["partitioned"])
        if i == j and not auto:
            B, over = f["B"], seq["over"]
            assert got["word"] == PAIR_OVERFLOW | SKIPPED, "%s: the device's flags word reads %#x" % (ctx, got["word"])
            assert got["raised"] == 1, "%s: wait_frame did not raise PairCapacityError" % ctx
            # the round that outgrew the bound, its true count, the bound
            assert got["e_round"] == over, "%s: the message names round %d" % (ctx, got["e_round"])
            assert got["e_pairs"] == (f["D1"] if over == 1 else f["D2"]), "%s: %d pairs reported" % (ctx, got["e_pairs"])
            assert got["e_capacity"] == B, "%s: a bound of %d reported, expected %d" % (ctx, got["e_capacity"], B)
            assert got["e_pairs"] > got["e_capacity"], ctx
            if over == 1:
                check_untouched(rgba, ctx)
            else:
                check_round1_state(ob, f["kind"], K, f["part"], rgba, ctx)
            continue
        assert got["raised"] == 0, "%s: skipped (%d pairs, bound %d)" % (ctx, got["e_pairs"], got["e_capacity"])
        assert got["flags"] == 0 and got["word"] == 0, "%s: flags %#x, device word %#x" % (ctx, got["flags"], got["word"])
        assert got["visible"] == f["V"], "%s: %d visible, the oracle %d" % (ctx, got["visible"], f["V"])
        if f["kind"] in TRANSLUCENT:
            assert got["pairs"] == f["D"], "%s: %d pairs, the oracle %d" % (ctx, got["pairs"], f["D"])
        else:
            # `cover`: round 1 finishes every tile, round 2 is gated: the frame's pairs are round 1's
            assert got["tiles_done"] == BAND_TILES, "%s: round 1 finished %d tiles" % (ctx, got["tiles_done"])
            assert got["pairs"] == f["D1"], "%s: %d pairs, round 1 of the oracle %d" % (ctx, got["pairs"], f["D1"])
        if i == j - 1:
            assert got["pair_capacity"] == p[j]["capacity"], "%s: buffers of %d pairs" % (ctx, got["pair_capacity"])
        if i == j + 1:       # recovered in ONE frame, with room for both rounds
            assert got["pair_capacity"] >= max(f["D1"], f["D2"]), ctx
        check_exact(ob, f["kind"], rgba, ctx)


@pytest.fixture(scope="module")
def rig(gs, ob, device):
    stream = device.create_stream()
    rg = Rig(gs, ob, device, stream)
    yield rg
    rg.release()
    stream.synchronize()
    stream.close()


@pytest.fixture(scope="module")
def runs(rig):
    """the recorded frames of a sequence, rendered once per module"""
    done = {}

    def get(name):
        if name not in done:
            done[name] = run_sequence(rig, name)
        return done[name]
    return get


def _partition():
    return int(os.environ.get("GS3D_ROUND_PARTITION", "1"))


@gpu
def test_round_2_outgrows_its_bound_inside_the_buffers(ob, runs):
    """big (sizes the buffers), small, small (the bound shrinks to B), big: D1_big <= B < D2_big <= the buffers' capacity.  The
    jump frame is flagged PAIR_OVERFLOW | SKIPPED, wait_frame names round 2, its count and B; the next pipelined frame is
    the oracle's, bit for bit."""
    check_sequence(ob, "round2", runs("round2"), _partition())


@gpu
def test_check_true_renders_the_jump_frame_again_by_itself(ob, rig):
    """the same jump through render(check=True): it waits, finds the frame skipped and renders it again with the report's
    bound — a flag-free result and the exact image, over round 1's state that the skipped attempt left in the band"""
    check_sequence(ob, "round2", run_sequence(rig, "round2", auto=True), _partition(), auto=True)


@gpu
def test_what_a_frame_skipped_by_round_2_left_behind(ob, runs):
    """check_round1_state on the jump frames of `round2` and `gated` (check_sequence runs it as well; here it stands alone,
    with its own name in the report): round 1's pixel state in the band, the poison outside"""
    for name in ("round2", "gated"):
        seq, p = SEQUENCES[name], predict(ob, name, _partition())
        j = seq["jump"]
        check_round1_state(ob, p[j]["kind"], seq["K"], p[j]["part"], runs(name)["f%d/rgba" % j], "%s, jump frame" % name)


@gpu
def test_round_1_outgrows_its_bound(ob, runs):
    """K = 16 384: D1_big > B.  Round 1's blend returns before it touches a pixel and round 2's does too (publish_pairs: "over |=
    state->overflow"): the whole image is still the poison; wait_frame names round 1; the next frame is exact."""
    check_sequence(ob, "round1", runs("round1"), _partition())


@gpu
@pytest.mark.parametrize("name", ["buffers2", "buffers1"])
def test_a_round_outgrows_the_buffers(ob, runs, name):
    """the sizing frame is `small`: the jump frame's bound is the buffers' capacity itself, round 2 (K = 2 048) or round 1
    (K = 16 384) outgrows it, and the recovery has to grow the buffers as well"""
    check_sequence(ob, name, runs(name), _partition())


@gpu
def test_gated_steady_state_then_the_tiles_open(ob, runs):
    """`cover` x 3: round 1 finishes all 360 tiles, round 2 is gated, round_pairs_max is round 1's count alone and the bound
    shrinks to capacity_for(2 * D1_cover); then `big` on the translucent buffer of the same length: no tile finishes, round 2
    has D2_big > B pairs — skipped, recovered in one frame; and back to `cover`."""
    check_sequence(ob, "gated", runs("gated"), _partition())


@gpu
def test_planes_and_the_flags_word_over_a_skipped_frame(gs, ob, rig):
    """`round2` with the depth and pick planes: the planes keep their poison outside the band over the skipped frame, and after
    the recovery they are those of a single-round frame on a new renderer — whose image and depth plane are the oracle's
    bit for bit and whose pick plane obeys the alpha relation and the float64 walk (tests/test_gpu_render_aux.py), the walk on
    every fourth tile of the band.  (The flags word, 3 then 0, is asserted by check_sequence in every sequence.)"""
    from planes import POISON_PICK, oracle_depth, pick_witness
    name = "round2"
    seq = SEQUENCES[name]
    j = seq["jump"]
    rec = run_sequence(rig, name, aux=True)
    check_sequence(ob, name, rec, _partition())
    y0, y1 = band_rows(BAND, H)
    outside = np.ones(H, bool)
    outside[y0:y1] = False
    assert np.isnan(rec["f%d/depth" % j][outside]).all() and (rec["f%d/pick" % j][outside] == POISON_PICK).all(), \
        "the skipped frame wrote the planes outside its band"
    # the single-round frame of `big`
    one = gs.Renderer(rig.device)
    one.set_rounds(0)
    fr, e = rig.render(one, "big", aux=True)
    assert e is None and fr.flags == 0 and one.sort_info().rounds == 1
    rgba, depth, pick = rig.planes.get(rig.stream)
    one.destroy()
    o = oracle_kind(ob, "big")
    assert fr.pairs == o["D"] and fr.visible == o["V"]
    check_exact(ob, "big", rgba, "single-round big")
    want_depth = oracle_depth(ob, o["proj"], o["idx"], o["ranges"], o["ocam"], o["ogt"], BAND)
    bad = bits(depth[y0:y1]) != bits(want_depth[y0:y1])
    assert not bad.any(), "single-round big: depth differs from the oracle at %d pixels" % bad.sum()
    assert np.array_equal(pick[y0:y1] != gs.PICK_NONE, rgba[y0:y1, :, 3] >= 0.5)      # exact: 1 - T is exact for T >= 0.5
    some = o["ranges"].copy()
    keep = np.zeros(len(some), bool)
    keep[BAND[0] * TILES_X:BAND[1] * TILES_X:4] = True
    some[~keep] = 0
    walked = np.repeat(np.repeat(keep.reshape(TILES_Y, TILES_X), 16, axis=0), 16, axis=1)[:H, :W]
    want_pick, ambiguous = pick_witness(o["proj"], o["idx"], some, W, H, TILES_X, float(np.float32(1.0) - np.float32(0.5)))
    bad = (want_pick != pick.astype(np.uint64)) & ~ambiguous & walked
    assert walked[y0:y1].sum() == 90 * 256 and not bad.any(), "single-round big: pick differs from the float64 walk at %d pixels" % bad.sum()
    assert np.isnan(depth[outside]).all() and (pick[outside] == POISON_PICK).all()
    # ... and the recovered two-round frame's planes are the same
    k = j + 1
    assert np.array_equal(bits(rec["f%d/depth" % k][y0:y1]), bits(depth[y0:y1])), "recovered frame: depth plane"
    assert np.array_equal(rec["f%d/pick" % k][y0:y1], pick[y0:y1]), "recovered frame: pick plane"
    assert np.isnan(rec["f%d/depth" % k][outside]).all() and (rec["f%d/pick" % k][outside] == POISON_PICK).all()


# ------------------------------------------------------------------------------------------------
# round 2 made the other way: GS3D_ROUND_PARTITION=0, one child process
# ------------------------------------------------------------------------------------------------

def _child(out):
    assert os.environ.get("GS3D_ROUND_PARTITION") == "0"
    with gpu_child.child_rig() as (gs, ob, dev, st):
        rg = Rig(gs, ob, dev, st)
        record = {}
        for name in CHILD_SEQUENCES:
            for k, v in run_sequence(rg, name).items():
                record["%s/%s" % (name, k)] = v
        np.savez(out, **record)
        rg.release()


@gpu
def test_the_sequences_with_round_2_compacted_out_of_the_full_order(ob, runs, tmp_path):
    """GS3D_ROUND_PARTITION=0: round 1 is the nearest K of ONE depth sort and round 2 is compacted out of its order
    (k_round2_count / _write) behind the same overflowed or overflowing rounds — `round2`, `round1` and `gated` in one child
    process; the parent checks the child's frames against the oracle.  The parent's own steady frames were partitioned."""
    for i in range(1, len(SEQUENCES["round2"]["frames"])):
        assert int(runs("round2")["f%d/info" % i][INFO.index("partitioned")]) == _partition() == 1
    out = os.path.join(str(tmp_path), "bounds_p0.npz")
    gpu_child.run([os.path.abspath(__file__), out], env={"GS3D_ROUND_PARTITION": "0"}, timeout=120, label="GS3D_ROUND_PARTITION=0")
    rec = gpu_child.load_npz(out)
    for name in CHILD_SEQUENCES:
        sub = {k[len(name) + 1:]: v for k, v in rec.items() if k.startswith(name + "/")}
        for i in range(len(SEQUENCES[name]["frames"])):
            assert int(sub["f%d/info" % i][INFO.index("partitioned")]) == 0
        check_sequence(ob, name, sub, 0)


if __name__ == "__main__":
    _child(sys.argv[1])
