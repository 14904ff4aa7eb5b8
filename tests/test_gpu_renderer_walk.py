"""One renderer, every frame-kind transition.  A gs_renderer carries a dozen pieces of state from one
frame into the next (the ping-pong sides, list mode, the rounds of the last frame, the slot-mask cache ...); all of it may
change how fast a frame is, never what it contains.  Here ONE renderer renders a sequence of KINDS — a kind is the whole
description of a frame: buffer, image size, band, camera, transform, planes, selections and every request — in which every
ordered pair of kinds, self-pairs included, occurs as consecutive frames (helpers.pair_walk: a de Bruijn sequence B(K, 2)),
and every frame is compared bit for bit with the ORACLE's frame of its kind, computed once per kind.  Nothing here compares
against another renderer or an earlier device frame.

The same walk runs in a child process (this file as a script) under GS3D_BLEND_GROUPS=2 — the 8x8-block instantiations of
k_blend_grouped — and under GS3D_BLEND_GROUPS=1 with GS3D_RANGES_IN_BLEND=1 — k_blend<MODE>; the switch is read once per
process.  The child asserts every frame itself (it ends at its first mismatch) and leaves its frames in an .npz that the
parent compares with its own cached oracle frames.

The figures in KINDS' comments (V visible Gaussians, D pairs, the longest tile list) are the oracle's, asserted below
without a GPU; the shapes are the smallest that still reach the paths named."""
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
from frames import Scene  # noqa: E402
from helpers import POISON, band_rows, bits  # noqa: E402
from planes import Planes  # noqa: E402
from walk_kinds import (BUFFERS, FIGURES, KINDS, N, NAMES, ROUND1, SAME_SHAPE_AS_ROUNDS, TINT_RGBA, host_buffer,  # noqa: E402
                        kind_transforms, oracle_frame, selection_masks, walk_sequence)

gpu = pytest.mark.gpu


def test_the_sequence_covers_every_ordered_pair():
    for k in (1, 2, 3, 12, 13):
        seq = helpers.pair_walk(k)
        assert len(seq) == k * k + 1 and set(seq) == set(range(k))
        assert helpers.consecutive_pairs(seq) == {(a, b) for a in range(k) for b in range(k)}
    seq = walk_sequence()
    assert len(NAMES) == 13 and len(seq) == 170
    assert helpers.consecutive_pairs(seq) == {(a, b) for a in NAMES for b in NAMES}


@pytest.mark.parametrize("name", list(FIGURES))
def test_oracle_figures_of_the_kinds(ob, name):
    """the paths a kind is there for depend on these: V < n / 2 (corner), D beyond plain's capacity (fat), lists of many
    staging batches, one tile-sort pass (small)"""
    o = oracle_frame(ob, name)
    V, D, longest = FIGURES[name]
    assert (o["V"], o["D"]) == (V, D)
    if longest is not None:
        assert o["longest"] == longest
    if name == "corner":
        assert o["V"] < N // 2
    if name == "small":
        assert o["num_tiles"] == 6
    if name == "fat":
        cap = 18523 + 18523 // 4 + 65536       # gsp::capacity_for(plain's D)
        assert cap == 88689 and o["D"] > cap and o["longest"] > 8 * 128


def test_rounds_kind_finishes_some_tiles_and_leaves_others_open(ob):
    """the coverage condition of `rounds`: round 1 must finish some tiles and leave others open, or the kind exercises no
    resumption.  Of the 35 tiles 24 come out certainly finished and 11 certainly open; a walk that ends at the first step
    below 1e-4 and calls it undecided when it lies within 0.1 % of it leaves 11 of the 24 undecided (pixels that hover just
    above 1e-4 and are taken below it by a small alpha) — round1_coverage walks on, and their next step decides them."""
    o = oracle_frame(ob, "rounds")
    print("rounds: certainly finished %d, certainly open %d of %d tiles" % (o["finished"], o["open"], o["num_tiles"]))
    assert o["num_tiles"] == 35 and o["V"] > 2 * ROUND1
    assert o["finished"] >= 1 and o["open"] >= 1
    assert o["finished"] + o["open"] <= o["num_tiles"]
    for m in o["model"]:
        # the model's exact counts lie inside the walk's brackets, and round 2 has something to drop
        assert o["finished"] <= m["tiles_done"] <= o["num_tiles"] - o["open"] and not m["gated"]
        assert m["pairs"] < m["pairs_undropped"] == o["D"]


# ------------------------------------------------------------------------------------------------
# the walk
# ------------------------------------------------------------------------------------------------

class Rig:
    """buffers, selections and image planes of a walk: created once, alive until release()"""

    def __init__(self, gs, ob, device, stream):
        self.gs, self.ob, self.device, self.stream = gs, ob, device, stream
        self.scenes, self.bufs = {}, {}
        for b, spec in BUFFERS.items():
            hb = host_buffer(ob, b)
            if spec["n"]:
                sc = Scene(gs, ob, device, stream, spec["sh"], spec["cov"], spec["n"], 16, 16, spatial=spec.get("spatial", True),
                           g=hb["g"])
                assert np.array_equal(np.asarray(sc.pods, dtype=np.uint8).reshape(-1), hb["pods"]), "product pack != oracle pack"
                self.scenes[b], self.bufs[b] = sc, sc.buf
            else:
                self.bufs[b] = gs.GaussiansBuffer.new_empty(device, gs.GaussianPod(spec["sh"], spec["cov"]), 0)
            order = self.bufs[b].download_order(stream)
            assert np.array_equal(order, hb["order"]), "buffer %s: the mirror order is not the oracle's spatial order" % b
        self.planes = {(W, H): Planes(gs, device, W, H) for W, H in sorted({(k["W"], k["H"]) for k in KINDS.values()})}
        hidden, tinted = selection_masks()
        self.hide, self.tint = self.scenes["P"].selection(hidden), self.scenes["P"].selection(tinted)
        self.frames = {}
        for name in KINDS:
            ogt, omt, ocam = kind_transforms(ob, name)
            self.frames[name] = (gs.GaussianTransformPod.from_buffer_copy(bytes(ogt)), gs.ModelTransformPod.from_buffer_copy(bytes(omt)),
                                 helpers.copy_camera(ocam, gs.Camera))

    def render(self, r, name, check=True):
        """one frame of a kind on renderer r: all three requests set, the target (and the aux planes) poisoned first"""
        k = KINDS[name]
        pl = self.planes[(k["W"], k["H"])]
        pl.poison(self.stream, image=True)
        r.set_rounds(*k["rounds"])
        r.set_sort_mode(*k["sort"])
        r.set_tile_masks(k["masks"])
        kw = dict(band=k["band"], check=check)
        if k["aux"]:
            kw.update(depth_device_ptr=pl.depth.device_ptr(), pick_device_ptr=pl.pick.device_ptr(), pick_threshold=0.5)
        if k["sel"]:
            kw.update(hide=self.hide, tint=self.tint, tint_rgba=TINT_RGBA)
        gt, mt, cam = self.frames[name]
        fr = r.render(self.stream, self.bufs[k["buf"]], gt, mt, cam, pl.img.device_ptr(), **kw)
        self.stream.synchronize()
        return fr

    def planes_of(self, name):
        k = KINDS[name]
        return self.planes[(k["W"], k["H"])].get(self.stream)

    def release(self):
        self.hide.destroy()
        self.tint.destroy()
        for pl in self.planes.values():
            pl.release()
        for sc in self.scenes.values():
            sc.release()
        self.bufs["E"].destroy()


def check_image(name, o, rgba, ctx):
    k = KINDS[name]
    y0, y1 = band_rows(k["band"], k["H"])
    bad = bits(rgba[y0:y1]) != bits(o["rgba"][y0:y1])
    assert not bad.any(), "%s: %d words of the image differ from the oracle's frame" % (ctx, bad.sum())
    assert (rgba[:y0] == POISON).all() and (rgba[y1:] == POISON).all(), "%s: rows outside the band were written" % ctx


def check_aux_planes(gs_pick_none, o, rgba, depth, pick, ctx):
    bad = bits(depth) != bits(o["depth"])
    assert not bad.any(), "%s: %d words of the depth plane differ from the oracle's" % (ctx, bad.sum())
    # exact: 1 - T is exact for T >= 0.5 (tests/test_gpu_render_aux.py)
    assert np.array_equal(pick != gs_pick_none, o["rgba"][..., 3] >= 0.5), "%s: pick != NONE <=> alpha >= 0.5 broken" % ctx
    bad = (o["pick"] != pick.astype(np.uint64)) & ~o["pick_ambiguous"]
    assert not bad.any(), "%s: the pick plane differs from the float64 walk at %d pixels" % (ctx, bad.sum())


def check_taps(r, fr, name, o, ctx):
    """single-round frames: D, the sorted keys and caller indices, tiles touched and the records of the visible Gaussians"""
    n = BUFFERS[KINDS[name]["buf"]]["n"]
    assert fr.pairs == o["D"], "%s: %d pairs, the oracle %d" % (ctx, fr.pairs, o["D"])
    keys, idx = r.download_sorted()
    assert np.array_equal(keys, o["keys"]), "%s: sorted keys differ" % ctx
    assert np.array_equal(idx, o["idx"]), "%s: sorted indices differ" % ctx
    proj, tiles = r.download_projected(n)
    assert np.array_equal(tiles, o["tiles"]), "%s: tiles touched differ at %d Gaussians" % (ctx, (tiles != o["tiles"]).sum())
    keep = o["tiles"] > 0
    assert proj[keep].tobytes() == o["proj"][keep].tobytes(), "%s: projected records of visible Gaussians differ" % ctx


def expected_rounds(name, groups):
    """plan_rounds refuses two rounds under GS3D_BLEND_GROUPS=1 (k_blend<MODE> cannot resume)"""
    return 2 if KINDS[name]["rounds"][0] == 1 and groups != 1 else 1


def walk(gs, ob, device, stream, groups=0, record=None, seq=None):
    """groups: GS3D_BLEND_GROUPS of this process (0: unset).  record: a dict that receives every frame's planes and figures.
    seq: a short sequence of kinds instead of the whole walk."""
    whole = seq is None
    if whole:
        seq = walk_sequence()
        assert helpers.consecutive_pairs(seq) == {(a, b) for a in NAMES for b in NAMES}, "the walk misses a transition"
    oracle = {name: oracle_frame(ob, name) for name in dict.fromkeys(seq)}
    if "rounds" in oracle:
        assert oracle["rounds"]["finished"] >= 1 and oracle["rounds"]["open"] >= 1, "round 1 resumes nothing"
    rig = Rig(gs, ob, device, stream)
    r = gs.Renderer(device)
    partitioned_seen = set()
    prev = "(new renderer)"
    for i, name in enumerate(seq):
        ctx = "frame %d, %s -> %s" % (i, prev, name)
        k, o = KINDS[name], oracle[name]
        fr = rig.render(r, name)
        rgba, depth, pick = rig.planes_of(name)
        si = r.sort_info()
        check_image(name, o, rgba, ctx)
        assert fr.flags == 0 and fr.visible == o["V"], "%s: flags %#x, %d visible, the oracle %d" % (ctx, fr.flags, fr.visible, o["V"])
        assert si.rounds == expected_rounds(name, groups), "%s: %d rounds" % (ctx, si.rounds)
        if si.rounds == 1:
            check_taps(r, fr, name, o, ctx)
        else:
            assert si.round1 == ROUND1, "%s: round 1 of %d" % (ctx, si.round1)
            partitioned_seen.add(int(si.partitioned))
            if prev in SAME_SHAPE_AS_ROUNDS:
                assert si.partitioned == 1, "%s: a frame of a known shape must be partitioned" % ctx
            elif prev != "empty":       # (an empty frame leaves the shape of the frame before it)
                assert si.partitioned == 0, "%s: a sizing frame cannot be partitioned" % ctx
            m = o["model"][int(si.partitioned)]
            assert si.tiles_done == m["tiles_done"], "%s: round 1 finished %d tiles, the model %d" % (ctx, si.tiles_done, m["tiles_done"])
            assert fr.pairs == m["pairs"], "%s: %d pairs, the model %d" % (ctx, fr.pairs, m["pairs"])
        if k["aux"]:
            check_aux_planes(gs.PICK_NONE, o, rgba, depth, pick, ctx)
        if record is not None:
            record["f%03d/rgba" % i] = rgba
            record["f%03d/info" % i] = np.array([fr.visible, fr.pairs, si.rounds, si.round1, si.tiles_done, si.partitioned],
                                                dtype=np.int64)
            if k["aux"]:
                record["f%03d/depth" % i], record["f%03d/pick" % i] = depth, pick
        prev = name
    if whole and groups != 1:
        assert partitioned_seen == {0, 1}, "two-round frames were partitioned: %s (both must occur)" % sorted(partitioned_seen)
    if record is not None:
        record["seq"] = np.array([NAMES.index(s) for s in seq], dtype=np.int64)
    r.destroy()
    rig.release()


@gpu
def test_every_transition_on_one_renderer(gs, ob, device, stream):
    walk(gs, ob, device, stream, groups=int(os.environ.get("GS3D_BLEND_GROUPS", "0")))


@gpu
def test_one_selection_pair_on_two_buffers_of_one_length(gs, ob, device, stream):
    """the walk's hide <-> hide_q transitions on their own: the renderer's slot-ordered copies of the two masks were gathered
    through P's mirror order; Q has the same length, the selections the same generation — only SlotMaskKey::buffer tells
    the frames apart"""
    walk(gs, ob, device, stream, seq=["hide", "hide_q", "hide", "hide", "hide_q"])


@gpu
def test_buffer_swap_overflows_an_unchanged_shape(gs, ob, device, stream):
    """`plain` sizes the pair buffers: stage_sizing reserves max(gsp::capacity_for(D), the plan's want_capacity), and a new
    renderer's want_capacity is 0, so the capacity is capacity_for(18 523) = 88 689.  `fat` is the same FrameShape (n, size,
    band) with D = 154 605: no sizing frame, the pipelined frame is skipped, and the renderer recovers.  (The camera-move
    overflow is test_pair_capacity_overflow_is_flagged_and_recovered; here the BUFFER changes under a known shape.)"""
    o_plain, o_fat = oracle_frame(ob, "plain"), oracle_frame(ob, "fat")
    rig = Rig(gs, ob, device, stream)
    r = gs.Renderer(device)
    fr = rig.render(r, "plain")
    assert fr.flags == 0 and fr.pairs == o_plain["D"] and fr.pair_capacity == 88689
    check_image("plain", o_plain, rig.planes_of("plain")[0], "plain (sizing frame)")
    assert o_fat["D"] > fr.pair_capacity
    assert rig.render(r, "fat", check=False) is None
    with pytest.raises(gs.PairCapacityError) as e:
        r.wait_frame()
    assert e.value.pairs == o_fat["D"] and e.value.capacity == 88689
    assert (rig.planes_of("fat")[0] == POISON).all(), "a skipped frame must leave the image untouched"
    prev = "fat (skipped)"
    for name in ("fat", "plain", "fat"):
        ctx = "%s -> %s" % (prev, name)
        fr = rig.render(r, name, check=True)
        assert fr.flags == 0 and fr.visible == oracle_frame(ob, name)["V"], ctx
        check_image(name, oracle_frame(ob, name), rig.planes_of(name)[0], ctx)
        check_taps(r, fr, name, oracle_frame(ob, name), ctx)
        prev = name
    r.destroy()
    rig.release()


# ------------------------------------------------------------------------------------------------
# the same walk under GS3D_BLEND_GROUPS = 2 and = 1: one child process per setting, one at a time
# ------------------------------------------------------------------------------------------------

CHILD_ENV = {2: {"GS3D_BLEND_GROUPS": "2"}, 1: {"GS3D_BLEND_GROUPS": "1", "GS3D_RANGES_IN_BLEND": "1"}}


def _child(groups, out):
    assert os.environ.get("GS3D_BLEND_GROUPS") == str(groups)
    with gpu_child.child_rig() as (gs, ob, dev, st):
        record = {}
        walk(gs, ob, dev, st, groups=groups, record=record)      # an AssertionError ends the child: nonzero, the message on stdout
        np.savez(out, **record)


@pytest.fixture(scope="module")
def child_frames(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("renderer_walk")

    def run(groups):
        out = os.path.join(str(tmp), "walk_g%d.npz" % groups)
        gpu_child.run([os.path.abspath(__file__), str(groups), out], env=CHILD_ENV[groups], timeout=300,
                      label="GS3D_BLEND_GROUPS=%d" % groups)
        return gpu_child.load_npz(out)
    return run


@gpu
@pytest.mark.parametrize("groups", [2, 1])
def test_every_transition_under_the_other_blend_kernels(gs, ob, child_frames, groups):
    """GS3D_BLEND_GROUPS=2: k_blend_grouped<MODE, 2, ROUNDS, AUX>; = 1 (with the ranges searched in the blend, as
    tests/test_gpu_switches.py pairs them): k_blend<MODE>, one round for `rounds`, and the G = 4 aux kernel for `aux`"""
    rec = child_frames(groups)
    seq = [NAMES[i] for i in rec["seq"]]
    assert helpers.consecutive_pairs(seq) == {(a, b) for a in NAMES for b in NAMES}, "the child's walk misses a transition"
    prev = "(new renderer)"
    partitioned_seen = set()
    for i, name in enumerate(seq):
        ctx = "GS3D_BLEND_GROUPS=%d, frame %d, %s -> %s" % (groups, i, prev, name)
        o = oracle_frame(ob, name)
        rgba = rec["f%03d/rgba" % i]
        visible, pairs, rounds, round1, tiles_done, partitioned = [int(x) for x in rec["f%03d/info" % i]]
        check_image(name, o, rgba, ctx)
        assert visible == o["V"] and rounds == expected_rounds(name, groups), ctx
        if rounds == 1:
            assert pairs == o["D"], ctx
        else:
            m = o["model"][partitioned]
            assert round1 == ROUND1 and tiles_done == m["tiles_done"] and pairs == m["pairs"], ctx
            partitioned_seen.add(partitioned)
        if KINDS[name]["aux"]:
            check_aux_planes(gs.PICK_NONE, o, rgba, rec["f%03d/depth" % i], rec["f%03d/pick" % i], ctx)
        prev = name
    assert partitioned_seen == ({0, 1} if groups == 2 else set())


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
