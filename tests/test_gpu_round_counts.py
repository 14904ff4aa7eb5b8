"""Two-round frames: the finished tiles and the pair counts, exactly (DESIGN.md §4.2 "rounds", the count rules).  The image
of a two-round frame is the single round's whatever round 2 drops, so the image tests cannot tell a round 2 that drops
nothing, or too much of what contributes below 1/255, or a threshold one digit off.  tests/rounds_np.py restates the count
rules over the oracle's stage outputs and its blend's "stopped" plane; here every frame of a case — one renderer, frame 1
unpartitioned (it sizes the buffers), frames 2 and 3 partitioned (tests/conftest.py pins GS3D_ROUND_PARTITION=1), the image
poisoned before each — must report the model's visible, pairs, tiles_done, rounds, round1 and partitioned, with flags 0 and
the oracle's single-round image bit for bit.

The conditions the cases rest on (how many tiles done and open, what is dropped and why) are asserted from the oracle alone,
without a GPU, in the first half of the file; their figures are in CASES' comments.

Which case carries which condition.  The issue's full list for a "mixed" case (15 % of the tiles done and 15 % open, done
tiles in the partial last column and row, 100 dropped Gaussians of which 10 with a masked rect, a survivor larger than
3 x 3, a survivor kept by the whole-box rule alone, 5 % between the pair count and the undropped one) is asserted for
mixed16k, unpartitioned and partitioned.  The same scene at K = 4 096 and 8 192 finishes 10 and 49 of its 273 tiles, under the
15 % bar whatever else holds, and near_gate leaves 5 tiles open by design: those cases are pinned by their figures.  The
band has no partial last row (tile rows 5..14 of 23) and stays at 4 % below the undropped count; it is asserted for the rest.

The depth cells kept: all of them — every plane pair of DEPTH_PLANES x every distribution of DEPTH_CASES x K = 4 096 and
16 384 (one test per plane pair and distribution, both K inside).  (0.001, 100) and (0, 1000) place the same Gaussians, but
their keys have 28 and 31 bits and are cut at bit 18 and 21; no cell's path is another's.

The mixed and the band case also run in one child process (this file as a script) per value of GS3D_BLEND_GROUPS whose
kernel has a ROUNDS instantiation other than the default's (k_blend_grouped<MODE, 4, true>): 2 and 8.  The child hands its
frames back in an .npz that the parent checks against the same model."""
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
import rounds_np  # noqa: E402
from helpers import POISON, band_rows, bits  # noqa: E402

gpu = pytest.mark.gpu

SH_SINGLE, SH_NONE, ROT_SCALE, COV_HALF = 0, 3, 0, 2      # gs.SH_* / gs.COV3D_*
MIXED = helpers.ROUNDS_MIXED_SCENE                            # 330 x 200: 21 x 13 tiles, last column 10 px, last row 8 px
NEAR_GATE = dict(n=40000, first=77, opacity=255, scale=8.0)
BAND_SCENE = dict(n=60000, first=31, opacity=255, scale=4.0)
ONE_TILE = helpers.ROUNDS_ONE_TILE_SCENE                       # the scene tests/test_gpu_rounds.py had for its small images
# every fourth splat at scale 9, the others at 0.7: the large ones finish tiles, the small ones behind them have rects to drop
WIDE_SCENE = dict(n=60000, first=5, opacity=255, scale=0.7, big=9.0, every=4)
DEPTH_PLANES = [(0.001, 100.0), (5.0, 20.0), (0.0, 1000.0), (9.99, 10.02), (10.0, 10.0015), (10.0, 10.0005)]
DEPTH_KEY_BITS = [28, 25, 31, 15, 11, 10]
DEPTH_CASES = ["same_depth", "two_depths", "narrow_range", "wide_range"]


def _case(scene, W, H, K, band=None, masks=1, sh=SH_NONE, cov=ROT_SCALE, planes=(0.1, 100.0), depth=None):
    return dict(scene=scene, W=W, H=H, K=K, band=band, masks=masks, sh=sh, cov=cov, planes=planes, depth=depth)


# the scene of tests/test_gpu_rounds.py's test_two_rounds_with_wide_tile_keys_and_unpacked_rects, rendered there with K = 8 192
OLD_WIDE_SCENE = dict(n=30000, first=5, opacity=255, scale=12.0)


# The model's figures, unpartitioned / partitioned: tiles done + open (a tile without pairs in round 1 is neither), Gaussians
# dropped, pairs = round 1's + round 2's
CASES = {
    # 10 + 263 of 273, 64 / 63 dropped, 25 803 + 68 575 / 25 968 + 68 412 pairs
    "mixed4k": _case(MIXED, 330, 200, 4096),
    # 49 + 224, 561 dropped (14 of them masked), 93 581 pairs either way
    "mixed8k": _case(MIXED, 330, 200, 8192),
    # THE mixed case.  164 + 109, 3 907 / 3 859 dropped (166 / 163 masked), 9 survivors larger than 3 x 3, 91 / 90 kept by the
    # whole-box rule alone, 64 525 + 22 537 / 64 906 + 22 257 pairs of 94 451 (round 1 of 16 384 / 16 530 Gaussians)
    "mixed16k": _case(MIXED, 330, 200, 16384),
    # rect version 3: no masked rect, every rect is its whole box
    "mixed16k_v3": _case(MIXED, 330, 200, 16384, masks=0),
    "mixed16k_sh": _case(MIXED, 330, 200, 16384, sh=SH_SINGLE, cov=COV_HALF),
    # 268 + 5 / 269 + 4: 22 618 / 22 889 dropped (5 625 / 5 689 masked), 73 713 / 72 694 pairs of 159 802
    "near_gate": _case(NEAR_GATE, 330, 200, 4096),
    # all 273 done: the gate closes, pairs = round 1's 74 067 / 74 512
    "gated": _case(NEAR_GATE, 330, 200, 8192),
    # tests/test_gpu_round_bounds.py's shape; a band's first frame takes the block list (keep_bits in list space).
    # 152 + 208 / 159 + 201 of 360, 1 774 / 2 160 dropped (109 / 156 masked), 96 660 / 95 631 pairs of 100 545
    "band": _case(BAND_SCENE, 640, 360, 8192, band=(5, 14)),
    # 257 x 40 tiles: 8-byte rects, box table in LDS;  257 x 257: table from global memory, u32 tile keys
    "wide_lds": _case(WIDE_SCENE, 4112, 640, 8192),
    "wide_global": _case(WIDE_SCENE, 4112, 4100, 2048),
    # a tile sort of one pass: 150 tiles, 85 + 65 / 86 + 64;  one tile: nothing done at K = 2 048, the gate at 16 384
    "one_pass": _case(MIXED, 240, 160, 16384),
    "one_tile_open": _case(ONE_TILE, 16, 16, 2048),
    "one_tile_gated": _case(ONE_TILE, 16, 16, 16384),
}
for _pi, _planes in enumerate(DEPTH_PLANES):
    for _dc in DEPTH_CASES:
        for _k in (4096, 16384):
            CASES["depth%d_%s_%d" % (_pi, _dc, _k)] = _case(MIXED, 330, 200, _k, planes=_planes, depth=_dc)
CHILD_CASES = ["mixed16k", "band"]
CHILD_GROUPS = [2, 8]


# ------------------------------------------------------------------------------------------------
# the oracle's side (no GPU)
# ------------------------------------------------------------------------------------------------

_scene_cache, _host_cache, _oracle_cache, _model_cache = {}, {}, {}, {}


def redepth(g, case, near, far):
    """tests/test_gpu_render.py's test_depth_key_ranges: the same Gaussians at one depth, at two adjacent floats, in a range
    1e-4 wide, or log-uniform over (near, far)"""
    g = g.copy()
    rng = np.random.default_rng(11)
    n0 = max(near, 1e-3)
    span = min(far, 95.0) - n0
    lo, hi = n0 + 0.02 * span, n0 + 0.98 * span
    mid = np.float32(0.5 * (lo + hi))
    if case == "same_depth":
        g["pos"][:, 2] = -mid
    elif case == "two_depths":
        g["pos"][:, 2] = np.where(rng.random(len(g)) < 0.5, -mid, -np.nextafter(mid, np.float32(np.inf))).astype(np.float32)
    elif case == "wide_range":
        glo = n0 * 1.02 if n0 * 1.02 < hi else lo
        g["pos"][:, 2] = -np.exp(rng.uniform(np.log(glo), np.log(hi), len(g))).astype(np.float32)
        g["pos"][:, :2] *= (-g["pos"][:, 2:3] / 14.0)
    else:
        assert case == "narrow_range"
        g["pos"][:, 2] = (-mid * (1.0 - rng.random(len(g)) * 1e-4)).astype(np.float32)
        g["pos"][:, :2] *= mid / 14.0
    return g


def scene_gaussians(spec, depth=None, planes=None):
    key = (tuple(sorted(spec.items())), depth, planes if depth else None)
    if key not in _scene_cache:
        g = helpers.deep_scene(spec["n"], first=spec["first"], opacity=spec["opacity"], scale=spec["scale"])
        if "big" in spec:
            g["scale"][::spec["every"]] *= np.float32(spec["big"] / spec["scale"])
        if depth:
            g = redepth(g, depth, *planes)
        _scene_cache[key] = g
    return key, _scene_cache[key]


def host_buffer(ob, name):
    """Gaussians, records and mirror order of a case's buffer, shared by the cases of one scene and layout"""
    c = CASES[name]
    skey, g = scene_gaussians(c["scene"], c["depth"], c["planes"])
    key = (skey, c["sh"], c["cov"])
    if key not in _host_cache:
        pods = ob.pack(c["sh"], c["cov"], g)
        _host_cache[key] = dict(key=key, g=g, pods=pods, order=ob.spatial_order(c["sh"], c["cov"], pods))
    return _host_cache[key]


def forget(ob, name):
    """drops a case's Gaussians and records (the depth cells: 24 scenes that nothing else shares); its oracle frame stays"""
    hb = host_buffer(ob, name)
    _host_cache.pop(hb["key"], None)
    _scene_cache.pop(hb["key"][0], None)


def case_transforms(ob, name):
    c = CASES[name]
    ogt = ob.gaussian_transform(sh_deg=3 if c["sh"] != SH_NONE else 0)
    ocam = helpers.default_camera(ob, c["W"], c["H"], near=c["planes"][0], far=c["planes"][1])
    return ogt, ob.model_transform(), ocam


def oracle_case(ob, name):
    """the oracle's single-round frame of a case in stages, once per module (cases that differ in K alone share it)"""
    c = CASES[name]
    hb = host_buffer(ob, name)
    key = (hb["key"], c["W"], c["H"], c["band"], c["masks"], c["planes"])
    if key not in _oracle_cache:
        ogt, omt, ocam = case_transforms(ob, name)
        version = ob.rect_version()
        try:
            ob.set_rect_version(4 if c["masks"] else 3)
            proj, tiles = ob.preprocess(c["sh"], c["cov"], hb["pods"], ogt, omt, ocam, band=c["band"])
            rgba = rounds_np.blend_lists(ob, proj, tiles, hb["order"], ocam, ogt, c["band"])[1]
        finally:
            ob.set_rect_version(version)
        _oracle_cache[key] = dict(proj=proj, tiles=tiles, order=hb["order"], ogt=ogt, omt=omt, ocam=ocam, rgba=rgba)
    return _oracle_cache[key]


def model(ob, name, partitioned):
    """rounds_np.frame of a case's unpartitioned (a renderer's first) or partitioned frame"""
    key = (name, bool(partitioned))
    if key not in _model_cache:
        c, o = CASES[name], oracle_case(ob, name)
        _model_cache[key] = rounds_np.frame(ob, o["proj"], o["tiles"], o["order"], o["ocam"], o["ogt"], c["band"], c["K"],
                                            partitioned, n=c["scene"]["n"])
    return _model_cache[key]


def describe(name, part, m):
    if m["rounds"] == 1:
        return "%s: a single round" % name
    return "%s, %s: V %d, round 1 of %d Gaussians, %d done + %d open of %d tiles%s, %d dropped (%d masked), pairs %d + %d of %d" % (
        name, "partitioned" if m["partitioned"] else "partitioned asked, refused" if part else "unpartitioned", m["visible"],
        int(m["member"].sum()), m["tiles_done"], int(m["open"].sum()), m["band_tiles"], " (gated)" if m["gated"] else "",
        len(m["dropped"]), int(m["masked"][m["dropped"]].sum()), m["D1"], m["pairs"] - m["D1"], m["D"])


def test_the_model_reproduces_the_figures_of_the_round_bound_sequences(ob):
    """tests/test_gpu_round_bounds.py asserts on the device: the translucent kinds finish no tile and emit D = D1 + D2, `cover`
    finishes all 360 tiles of the band with a round 1 of 2 048 and emits round 1's 63 555 pairs alone"""
    import round_kinds as rb
    want = {"small": (23501, 55345, {2048: 10613, 16384: 42774}), "big": (28468, 309085, {2048: 76478, 16384: 237078}),
            "cover": (27773, 258918, {2048: 63555})}
    for kind, (V, D, d1) in want.items():
        o = rb.oracle_kind(ob, kind)
        for K, D1 in d1.items():
            for part in (0, 1):
                m = rounds_np.frame(ob, o["proj"], o["tiles"], o["order"], o["ocam"], o["ogt"], rb.BAND, K, part, n=rb.N)
                print(describe(kind, part, m))
                assert (m["rounds"], m["round1"], m["partitioned"], m["visible"], m["D"]) == (2, K, part, V, D)
                assert m["band_tiles"] == rb.BAND_TILES == 360
                assert m["D1"] == rb.round_counts(ob, kind, K, part)[0]
                if not part:
                    assert m["D1"] == D1 and int(m["member"].sum()) == K
                if kind == "cover":
                    assert m["gated"] and m["tiles_done"] == 360 and m["pairs"] == m["D1"]
                else:
                    assert m["tiles_done"] == 0 and len(m["dropped"]) == 0 and m["pairs"] == D


@pytest.mark.parametrize("which", ["walk_rounds", "mixed4k"])
def test_the_model_agrees_with_the_float64_walk(ob, which):
    """an independent computation of round 1's coverage (tests/walk_kinds.py's round1_coverage: float64, its own
    arithmetic, a 0.1 % undecided margin): every tile it calls certainly finished is done, no done tile is certainly open"""
    import walk_kinds as tw
    if which == "walk_rounds":
        o = tw.oracle_frame(ob, "rounds")
        W, H, order = 100, 70, tw.host_buffer(ob, "R")["order"]
        m = o["model"][0]
        sure_done, sure_open = tw.round1_coverage_masks(o, order, W, H, tw.ROUND1)
    else:
        c, oc = CASES[which], oracle_case(ob, which)
        W, H, order = c["W"], c["H"], oc["order"]
        m = model(ob, which, 0)
        tiles_x = (W + 15) // 16
        keys, idx = ob.build_keys(oc["proj"], oc["tiles"], tiles_x, order=order)
        skeys, sidx = ob.sort_pairs(keys, idx)
        o = dict(proj=oc["proj"], idx=sidx, ranges=ob.tile_ranges(skeys, tiles_x * ((H + 15) // 16)), tiles=np.asarray(oc["tiles"]),
                 tiles_x=tiles_x)
        sure_done, sure_open = tw.round1_coverage_masks(o, order, W, H, c["K"])
    done = m["done"].ravel()
    print("%s: the walk %d certainly finished, %d certainly open; the model %d done, %d open" % (
        which, sure_done.sum(), sure_open.sum(), done.sum(), m["open"].sum()))
    assert sure_done.sum() >= 1 and sure_open.sum() >= 1
    assert not (sure_done & ~done).any(), "a certainly finished tile is not done"
    assert not (done & sure_open).any(), "a done tile is certainly open"


@pytest.mark.parametrize("part", [0, 1])
def test_the_mixed_case_is_mixed(ob, part):
    """what makes mixed16k tell a wrong round 2 from a right one: enough tiles done and open, done tiles in the partial last
    column and row, dropped Gaussians with plain and with masked rects, survivors that are too large, survivors that only
    the whole-box rule keeps, and a pair count far from the undropped one"""
    name = "mixed16k"
    c, o, m = CASES[name], oracle_case(ob, name), model(ob, name, part)
    print(describe(name, part, m))
    kept = rounds_np.kept_by_whole_box_only(m, o["proj"], o["tiles"])
    large = int((~m["small"])[m["survivors"]].sum())
    print("survivors larger than 3 x 3: %d, kept by the whole-box rule alone: %d, undropped %d" % (large, len(kept), m["pairs_undropped"]))
    assert (c["W"] % 16, c["H"] % 16, m["band_tiles"]) == (10, 8, 273)
    assert m["partitioned"] == part and not m["gated"]
    assert m["tiles_done"] >= 0.15 * 273 and m["open"].sum() >= 0.15 * 273
    assert m["done"][:, -1].any() and m["done"][-1].any()
    assert len(m["dropped"]) >= 100 and m["masked"][m["dropped"]].sum() >= 10
    assert large >= 1 and len(kept) >= 1
    assert m["pairs_undropped"] - m["pairs"] >= 0.05 * m["pairs"]
    # the figures of CASES' comment
    got = (m["tiles_done"], int(m["open"].sum()), len(m["dropped"]), int(m["masked"][m["dropped"]].sum()), large, m["D1"], m["pairs"] - m["D1"],
           m["pairs_undropped"], int(m["member"].sum()))
    assert got == ((164, 109, 3907, 166, 9, 64525, 22537, 94451, 16384), (164, 109, 3859, 163, 9, 64906, 22257, 94451, 16530))[part]


@pytest.mark.parametrize("part", [0, 1])
def test_the_other_cases_are_what_their_comments_say(ob, part):
    want = {      # name: (done, open, dropped, masked among them, pairs), unpartitioned / partitioned
        "mixed4k": ((10, 263, 64, 0, 94378), (10, 263, 63, 0, 94380)),
        "mixed8k": ((49, 224, 561, 14, 93581), (49, 224, 561, 14, 93581)),
        "near_gate": ((268, 5, 22618, 5625, 73713), (269, 4, 22889, 5689, 72694)),
        "gated": ((273, 0, 21217, 5214, 74067), (273, 0, 21140, 5185, 74512)),
        "band": ((152, 208, 1774, 109, 96660), (159, 201, 2160, 156, 95631)),
    }
    for name, w in want.items():
        m = model(ob, name, part)
        print(describe(name, part, m))
        got = (m["tiles_done"], int(m["open"].sum()), len(m["dropped"]), int(m["masked"][m["dropped"]].sum()), m["pairs"])
        assert got == w[part], name
        assert m["gated"] == (name == "gated") and m["partitioned"] == part
        if name == "band":
            # mixed: at least 15 % of the band's tiles done and as many open, masked rects among the dropped, large survivors
            assert m["band_tiles"] == 360 and got[0] >= 54 and got[1] >= 54 and got[2] >= 100 and got[3] >= 10
            assert (~m["small"])[m["survivors"]].any()
            assert not m["done"][:5].any() and not m["done"][14:].any()
    m = model(ob, "mixed16k_v3", part)
    print(describe("mixed16k_v3", part, m))
    assert not m["masked"].any() and m["tiles_done"] >= 41 and m["open"].sum() >= 41 and len(m["dropped"]) >= 100
    m = model(ob, "mixed16k_sh", part)
    print(describe("mixed16k_sh", part, m))
    assert m["tiles_done"] >= 41 and m["open"].sum() >= 41 and len(m["dropped"]) >= 100


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("name", ["wide_lds", "wide_global", "one_pass"])
def test_the_other_instantiations_have_done_and_open_tiles_and_something_to_drop(ob, name, part):
    """(WIDE_SCENE mixes two sizes: test_why_the_wide_cases_have_a_scene_of_their_own)"""
    m = model(ob, name, part)
    print(describe(name, part, m))
    assert m["rounds"] == 2 and m["partitioned"] == part and not m["gated"]
    assert m["tiles_done"] >= 1 and m["open"].sum() >= 1
    assert len(m["dropped"]) >= 100 and len(m["survivors"]) >= 100
    assert m["band_tiles"] == {"wide_lds": 257 * 40, "wide_global": 257 * 257, "one_pass": 150}[name]


@pytest.mark.parametrize("part", [0, 1])
def test_the_single_tile_finishes_nothing_or_everything(ob, part):
    m = model(ob, "one_tile_open", part)
    print(describe("one_tile_open", part, m))
    assert (m["band_tiles"], m["tiles_done"], int(m["open"].sum()), len(m["dropped"]), m["pairs"]) == (1, 0, 1, 0, m["D"])
    m = model(ob, "one_tile_gated", part)
    print(describe("one_tile_gated", part, m))
    assert m["gated"] and m["tiles_done"] == 1 and m["pairs"] == m["D1"] < m["D"]


def test_the_small_image_scenes_of_the_rounds_tests_drop_something(ob):
    """tests/test_gpu_rounds.py's test_two_rounds_on_small_images renders small_image_scene at 240 x 160, 387 x 144 and 16 x 16
    with K = 2 048 and 16 384: at the two larger sizes the longer round 1 must finish some tiles, leave others open and drop
    Gaussians (its old scene finished none at either K)"""
    g = helpers.small_image_scene(240, 160)
    assert g is helpers.small_image_scene(387, 144) and np.array_equal(g, scene_gaussians(MIXED)[1])
    assert np.array_equal(helpers.small_image_scene(16, 16), scene_gaussians(ONE_TILE)[1])
    pods = ob.pack(SH_NONE, ROT_SCALE, g)
    order = ob.spatial_order(SH_NONE, ROT_SCALE, pods)
    ogt, omt = ob.gaussian_transform(sh_deg=0), ob.model_transform()
    for W, H in ((240, 160), (387, 144)):
        ocam = helpers.default_camera(ob, W, H)
        proj, tiles = ob.preprocess(SH_NONE, ROT_SCALE, pods, ogt, omt, ocam)
        for part in (0, 1):
            m = rounds_np.frame(ob, proj, tiles, order, ocam, ogt, None, 16384, part)
            print(describe("%d x %d" % (W, H), part, m))
            assert m["tiles_done"] >= 10 and m["open"].sum() >= 10 and len(m["dropped"]) >= 100


def test_why_the_wide_cases_have_a_scene_of_their_own(ob):
    """the scene tests/test_gpu_rounds.py renders at 4112 x 640 and 4112 x 4100 cannot carry a count test: at 4112 x 640 its
    round 1 of 8 192 finishes all 10 280 tiles (the gate closes, round 2 is never judged), and at 4112 x 4100 not one visible
    Gaussian has a rect of 3 x 3 tiles or less, so round 2 has nothing it may drop whatever round 1 finishes"""
    g = helpers.deep_scene(OLD_WIDE_SCENE["n"], first=OLD_WIDE_SCENE["first"], opacity=OLD_WIDE_SCENE["opacity"], scale=OLD_WIDE_SCENE["scale"])
    pods = ob.pack(SH_NONE, ROT_SCALE, g)
    order = ob.spatial_order(SH_NONE, ROT_SCALE, pods)
    ogt, omt = ob.gaussian_transform(sh_deg=0), ob.model_transform()
    ocam = helpers.default_camera(ob, 4112, 640)
    proj, tiles = ob.preprocess(SH_NONE, ROT_SCALE, pods, ogt, omt, ocam)
    m = rounds_np.frame(ob, proj, tiles, order, ocam, ogt, None, 8192, 0)
    print(describe("the old scene at 4112 x 640", 0, m))
    assert m["gated"] and m["tiles_done"] == 257 * 40
    proj, tiles = ob.preprocess(SH_NONE, ROT_SCALE, pods, ogt, omt, helpers.default_camera(ob, 4112, 4100))
    vis = np.asarray(tiles) > 0
    w, h = proj["tx1"].astype(int) - proj["tx0"], proj["ty1"].astype(int) - proj["ty0"]
    print("the old scene at 4112 x 4100: %d visible, %d of them with a rect of at most 3 x 3 tiles" % (vis.sum(), (vis & (w <= 3) & (h <= 3)).sum()))
    assert vis.sum() > 10000 and not (vis & (w <= 3) & (h <= 3)).any()


@pytest.mark.parametrize("pi", range(len(DEPTH_PLANES)))
def test_the_depth_cells_reach_what_they_are_there_for(ob, pi):
    """per plane pair: the key width, whether a frame can be partitioned at all, and what the model makes of the four
    distributions — one or two depths in front of the cut: a partitioned round 1 takes every visible Gaussian and round 2
    is empty; one depth, unpartitioned: round 1 cuts a run of equal keys in mirror order"""
    near, far = DEPTH_PLANES[pi]
    dbits = rounds_np.depth_key_bits(near, far)[1]
    assert dbits == DEPTH_KEY_BITS[pi]
    can = dbits > 10
    some_drop = False
    for dc in DEPTH_CASES:
        for K in (4096, 16384):
            name = "depth%d_%s_%d" % (pi, dc, K)
            for part in (0, 1):
                m = model(ob, name, part)
                print(describe(name, part, m))
                assert m["rounds"] == 2 and m["round1"] == K and m["partitioned"] == (part if can else 0)
                assert m["visible"] > 10000
                members = int(m["member"].sum())
                if m["partitioned"] and dc in ("same_depth", "two_depths"):
                    assert members == m["visible"] and len(m["rest"]) == 0 and m["pairs"] == m["D"] == m["D1"]
                elif not m["partitioned"]:
                    assert members == min(K, m["visible"])
                else:
                    assert members >= min(K, m["visible"])
                if not m["partitioned"] and dc == "same_depth":
                    o = oracle_case(ob, name)
                    vis = rounds_np.visible_in_order(o["tiles"], o["order"])
                    assert len(np.unique(o["proj"]["depth"][vis])) == 1 and m["member"][vis[:K]].all() and not m["member"][vis[K:]].any()
                some_drop = some_drop or (not m["gated"] and len(m["dropped"]) >= 100)
        forget(ob, name)
    assert some_drop, "no cell of these planes drops anything in a round 2 that runs"


# ------------------------------------------------------------------------------------------------
# the device's side
# ------------------------------------------------------------------------------------------------

INFO = ["flags", "visible", "pairs", "rounds", "round1", "tiles_done", "partitioned", "tile_masks"]
FRAMES = 3


class Rig:
    """device buffers by scene and layout, created on first use, alive until release()"""

    def __init__(self, gs, ob, device, stream):
        self.gs, self.ob, self.device, self.stream = gs, ob, device, stream
        self.bufs, self.images = {}, {}

    def buffer(self, name):
        c, hb = CASES[name], host_buffer(self.ob, name)
        if hb["key"] not in self.bufs:
            gs = self.gs
            pod = gs.GaussianPod(c["sh"], c["cov"])
            pods = pod.from_gaussian(hb["g"])
            assert np.array_equal(np.asarray(pods, dtype=np.uint8).reshape(-1), hb["pods"]), "product pack != oracle pack"
            buf = gs.GaussiansBuffer.new_with_pods(self.device, pod, pods)
            assert np.array_equal(buf.download_order(self.stream), hb["order"]), "%s: not the oracle's spatial order" % name
            self.bufs[hb["key"]] = buf
        return self.bufs[hb["key"]]

    def image(self, W, H):
        if (W, H) not in self.images:
            self.images[(W, H)] = self.gs.Buffer(self.device, data=np.full(W * H * 4, POISON, dtype=np.float32))
        return self.images[(W, H)]

    def drop_buffer(self, name):
        buf = self.bufs.pop(host_buffer(self.ob, name)["key"], None)
        if buf is not None:
            buf.destroy()
        forget(self.ob, name)

    def release(self):
        for b in self.bufs.values():
            b.destroy()
        for i in self.images.values():
            i.release()
        self.bufs, self.images = {}, {}


def run_case(rig, name):
    """FRAMES frames of a case on one new renderer: {"f<i>/info": INFO's figures, "f<i>/rgba"}"""
    gs, ob, c = rig.gs, rig.ob, CASES[name]
    W, H = c["W"], c["H"]
    ogt, omt, ocam = case_transforms(ob, name)
    gt, mt = gs.GaussianTransformPod.from_buffer_copy(bytes(ogt)), gs.ModelTransformPod.from_buffer_copy(bytes(omt))
    cam = helpers.copy_camera(ocam, gs.Camera)
    buf, img = rig.buffer(name), rig.image(W, H)
    poison = np.full(W * H * 4, POISON, dtype=np.float32)
    r = gs.Renderer(rig.device)
    r.set_rounds(1, c["K"])
    r.set_tile_masks(c["masks"])
    rec = {}
    for i in range(FRAMES):
        img.write(rig.stream, 0, poison)
        rig.stream.synchronize()
        r.render(rig.stream, buf, gt, mt, cam, img.device_ptr(), band=c["band"], check=False)
        fr = r.wait_frame()
        si = r.sort_info()
        info = dict(flags=fr.flags, visible=fr.visible, pairs=fr.pairs, rounds=si.rounds, round1=si.round1, tiles_done=si.tiles_done,
                    partitioned=si.partitioned, tile_masks=si.tile_masks)
        print("%s frame %d: %s" % (name, i, " ".join("%s %d" % (k, info[k]) for k in INFO)), flush=True)
        rec["f%d/info" % i] = np.array([info[k] for k in INFO], dtype=np.int64)
        rec["f%d/rgba" % i] = img.download(rig.stream, np.float32).reshape(H, W, 4)
    r.destroy()
    return rec


def check_case(ob, name, rec, ctx=""):
    """every frame of a recorded case against the model of its kind and the oracle's single-round image"""
    c, o = CASES[name], oracle_case(ob, name)
    y0, y1 = band_rows(c["band"], c["H"])
    for i in range(FRAMES):
        where = "%s%s, frame %d" % (ctx, name, i)
        m = model(ob, name, i > 0)        # a renderer's first frame sizes the buffers: never partitioned
        got = dict(zip(INFO, (int(x) for x in rec["f%d/info" % i])))
        rgba = rec["f%d/rgba" % i]
        print(describe(name, i > 0, m))
        print("%s: %s" % (where, got))
        bad = bits(rgba[y0:y1]) != bits(o["rgba"][y0:y1])
        assert not bad.any(), "%s: %d words of the image differ from the oracle's single-round frame" % (where, bad.sum())
        assert (rgba[:y0] == POISON).all() and (rgba[y1:] == POISON).all(), "%s: rows outside the band were written" % where
        assert got["flags"] == 0, "%s: flags %#x" % (where, got["flags"])
        assert got["tile_masks"] == c["masks"], where
        for k in ("visible", "pairs", "tiles_done", "rounds", "round1", "partitioned"):
            assert got[k] == m[k], "%s: %s is %d, the model says %d" % (where, k, got[k], m[k])


@pytest.fixture(scope="module")
def rig(gs, ob, device):
    stream = device.create_stream()
    rg = Rig(gs, ob, device, stream)
    yield rg
    rg.release()
    stream.synchronize()
    stream.close()


@gpu
@pytest.mark.parametrize("name", ["mixed4k", "mixed8k", "mixed16k", "near_gate", "gated"])
def test_mixed_frames_report_the_models_counts(ob, rig, name):
    check_case(ob, name, run_case(rig, name))


@gpu
def test_rect_version_3_has_no_masked_rect_to_judge(ob, rig):
    """set_tile_masks(0) on the device, set_rect_version(3) in the oracle (and back): every rect is plain"""
    check_case(ob, "mixed16k_v3", run_case(rig, "mixed16k_v3"))


@gpu
def test_sh_f32_and_cov_f16_records(ob, rig):
    check_case(ob, "mixed16k_sh", run_case(rig, "mixed16k_sh"))
    rig.drop_buffer("mixed16k_sh")


@gpu
def test_a_band_whose_first_frame_takes_the_block_list(ob, rig):
    """keep_bits of a list frame live in list space, the round-2 gather reads them there"""
    check_case(ob, "band", run_case(rig, "band"))


@gpu
@pytest.mark.parametrize("name", ["wide_lds", "wide_global"])
def test_unpacked_rects_and_the_box_table_in_lds_and_in_global_memory(ob, rig, name):
    check_case(ob, name, run_case(rig, name))


@gpu
@pytest.mark.parametrize("name", ["one_pass", "one_tile_open", "one_tile_gated"])
def test_a_tile_sort_of_one_pass_or_none(ob, rig, name):
    check_case(ob, name, run_case(rig, name))
    if name == "one_tile_gated":
        rig.drop_buffer(name)


@gpu
@pytest.mark.parametrize("dc", DEPTH_CASES)
@pytest.mark.parametrize("pi", range(len(DEPTH_PLANES)))
def test_depth_planes_and_distributions_under_two_rounds(ob, rig, pi, dc):
    for K in (4096, 16384):
        name = "depth%d_%s_%d" % (pi, dc, K)
        check_case(ob, name, run_case(rig, name))
    rig.drop_buffer(name)


# ------------------------------------------------------------------------------------------------
# the other blend kernels with a ROUNDS instantiation: one child process per GS3D_BLEND_GROUPS, one at a time
# ------------------------------------------------------------------------------------------------

def _child(groups, out):
    assert os.environ.get("GS3D_BLEND_GROUPS") == str(groups)
    with gpu_child.child_rig() as (gs, ob, dev, st):
        rg = Rig(gs, ob, dev, st)
        record = {}
        for name in CHILD_CASES:
            for k, v in run_case(rg, name).items():
                record["%s/%s" % (name, k)] = v
        np.savez(out, **record)
        rg.release()


@gpu
@pytest.mark.parametrize("groups", CHILD_GROUPS)
def test_the_counts_under_the_other_blend_kernels(ob, tmp_path, groups):
    """GS3D_BLEND_GROUPS=2 / 8: k_blend_grouped<MODE, 2, true> / <MODE, 8, true> set the done and open bits"""
    out = os.path.join(str(tmp_path), "counts_g%d.npz" % groups)
    gpu_child.run([os.path.abspath(__file__), str(groups), out], env={"GS3D_BLEND_GROUPS": str(groups)}, timeout=90,
                  label="GS3D_BLEND_GROUPS=%d" % groups)
    rec = gpu_child.load_npz(out)
    for name in CHILD_CASES:
        sub = {k[len(name) + 1:]: v for k, v in rec.items() if k.startswith(name + "/")}
        check_case(ob, name, sub, ctx="GS3D_BLEND_GROUPS=%d, " % groups)


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
