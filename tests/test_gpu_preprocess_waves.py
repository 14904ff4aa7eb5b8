"""The wave-uniform exit of the preprocess stage: in k_preprocess a wave of 64 mirror slots none of which
has a radius rect on the screen (project_geom: `dead`) leaves behind that rect and stores no records.  That may not change
a bit of a frame; k_preprocess_banded (which prefetches the next Gaussian and does not take the exit) runs the same cases.

Two families, every frame against the ORACLE's: V, D, tiles touched (the key and rect taps: a culled slot reads 0), the
projected records of the visible Gaussians byte for byte, the sorted pairs, the tile ranges and the image bit for bit.

 * sizes: N around every item boundary of a thread (256 slots) and the partial last block — partial waves that exit, and
   the banded kernel's prefetch guard `inext < n` — through k_preprocess (records without SH) and k_preprocess_banded
   (records with SH);
 * waves by construction: a buffer in INDEX order (mirror slot = index, asserted through download_order), 64 Gaussians per
   wave, each wave built to be culled for one reason, to keep one lane, or to be visible (WAVES below).  What each wave
   is, the oracle confirms without a GPU (test_the_waves_are_what_they_are_named).  The same Gaussians also go through
   the spatially ordered mirror, where the waves are the Morton order's.

The constructed frames run again in child processes under GS3D_MASK_REC=0, GS3D_MASK_REC=1 and GS3D_BLOCK_LIST=1 (the
switches are read once per process)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gpu_child  # noqa: E402
import helpers  # noqa: E402
import synth  # noqa: E402
import walk_kinds as walk  # noqa: E402
from frames import Scene, compare_frame  # noqa: E402
from helpers import POISON, band_rows, bits  # noqa: E402

gpu = pytest.mark.gpu

W, H = 100, 70
TILES_X, TILES_Y = (W + 15) // 16, (H + 15) // 16
WAVE, ITEM, BLOCK = 64, 256, 1024
SH_NONE, SH_SINGLE = walk.SH_NONE, walk.SH_SINGLE
# the three covariance layouts of records without SH (k_preprocess), one layout with SH (k_preprocess_banded)
LAYOUTS = [(SH_NONE, 0), (SH_NONE, 1), (SH_NONE, 2), (SH_SINGLE, 0)]
LAYOUT_IDS = ["sh%d-cov%d" % lc for lc in LAYOUTS]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
BAND = (1, 3)

# mirror slots [64 w, 64 w + 64) in index order; the last wave is partial
WAVES = ["visible_a", "left", "visible_b", "right", "above", "below", "opacity0", "det", "near", "only_lane0", "only_lane63",
         "visible_c", "left_b", "visible_d", "clipped_away", "visible_e", "below_b", "tail"]
TAIL = 17
N = (len(WAVES) - 1) * WAVE + TAIL
VISIBLE = {"visible_a", "visible_b", "visible_c", "visible_d", "visible_e"}
CLIPPED_LANE = 5                                   # of visible_c: one Gaussian of the clipped_away kind among visible ones


def wave(name):
    w = WAVES.index(name)
    return slice(w * WAVE, min((w + 1) * WAVE, N))


def _place(g, idx, px, py, z, cam):
    """centres at pixel (px, py), depth z, for the default camera (eye at the origin, looking down -z)"""
    g["pos"][idx, 0] = (px - cam.cx) / cam.fx * z
    g["pos"][idx, 1] = -(py - cam.cy) / cam.fy * z
    g["pos"][idx, 2] = -z


def _clip_away(g, idx, cam):
    """radius rect non-empty, clipped rect empty: opacity byte 1 reaches alpha 1/255 only within
    power >= -0.1, a quarter of a pixel for a splat of the dilation's size, and the centre sits on a tile CORNER, half a
    pixel from the nearest pixel centre"""
    k = np.arange(len(idx))
    _place(g, idx, 16.0 * (1 + k % 5), 16.0 * (1 + (k // 5) % 3), 3.0 + (k % 7) * 0.5, cam)
    g["scale"][idx] = 1e-4
    g["color"][idx, 3] = 1


_cache = {}


def constructed(ob):
    """the Gaussians of WAVES, and the hide and tint masks of their selection frame"""
    if _cache:
        return _cache
    cam = helpers.default_camera(ob, W, H)
    rng = np.random.default_rng(64)
    g = synth.scene(N, first=5)                                   # rotations, colours, SH
    # everything on the screen first: opaque enough and large enough to reach a pixel centre wherever it lies
    _place(g, np.arange(N), rng.uniform(4, W - 4, N), rng.uniform(4, H - 4, N), rng.uniform(3.0, 8.0, N), cam)
    g["scale"] = np.exp(rng.uniform(-4.0, -1.0, (N, 3))).astype(np.float32)        # some rects of 2 .. 3 tiles: the corner test
    g["color"][:, 3] = rng.integers(128, 256, N)
    z = -g["pos"][:, 2]

    def off(name, px=None, py=None):
        idx = np.arange(N)[wave(name)]
        _place(g, idx, rng.uniform(4, W - 4, len(idx)) if px is None else px, rng.uniform(4, H - 4, len(idx)) if py is None else py,
               z[idx], cam)
    for name in ("left", "left_b", "tail"):
        off(name, px=-300.0)
    off("right", px=W + 300.0)
    off("above", py=-300.0)
    off("below", py=H + 300.0)
    off("below_b", py=H + 300.0)
    g["color"][wave("opacity0"), 3] = 0
    g["scale"][wave("det")] = 1e20                                # the 2-D covariance overflows: det is no positive number
    idx = np.arange(N)[wave("near")]
    g["pos"][idx[::2], 2] = -0.05                                 # between the eye and the near plane (0.1)
    g["pos"][idx[1::2], 2] = 1.0                                  # behind the eye
    for name, lane in (("only_lane0", 0), ("only_lane63", WAVE - 1)):
        idx = np.delete(np.arange(N)[wave(name)], lane)
        _place(g, idx, -300.0, rng.uniform(4, H - 4, len(idx)), z[idx], cam)
    _clip_away(g, np.arange(N)[wave("clipped_away")], cam)
    _clip_away(g, np.arange(N)[wave("visible_c")][CLIPPED_LANE:CLIPPED_LANE + 1], cam)
    _cache.update(g=g, hidden=rng.random(N) < 0.4, tinted=rng.random(N) < 0.2)
    return _cache


def frames_of(sh):
    """(label, band, selection frame?): the second plain frame is the shape's first frame that is no sizing frame"""
    return [("plain (sizing)", None, False), ("plain", None, False), ("hide + tint", None, True), ("band", BAND, False),
            ("band, hide + tint", BAND, True)]


def oracle_frame(ob, sh, cov, order, band, sel):
    sc = constructed(ob)
    pods = ob.pack(sh, cov, sc["g"])
    if sel:
        pods = Scene.twin_pods(types.SimpleNamespace(pods=pods, n=N), sc["hidden"])
    ogt, omt = ob.gaussian_transform(sh_deg=3 if sh != SH_NONE else 0), ob.model_transform()
    ocam = helpers.default_camera(ob, W, H)
    proj, tiles = ob.preprocess(sh, cov, pods, ogt, omt, ocam, band=band)
    if sel:
        walk.recolour(proj, sc["tinted"])
    keys, idx = ob.build_keys(proj, tiles, TILES_X, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, TILES_X * TILES_Y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=ogt)
    tl = np.asarray(tiles)
    return dict(proj=proj, tiles=tl, keys=skeys, idx=sidx, ranges=ranges, rgba=rgba, V=int((tl > 0).sum()),
                D=int(tl.astype(np.uint64).sum()), ogt=ogt, omt=omt, ocam=ocam)


# ------------------------------------------------------------------------------------------------
# the construction, from the oracle alone (no GPU)
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", LAYOUTS, ids=LAYOUT_IDS)
def test_the_waves_are_what_they_are_named(ob, sh, cov):
    sc = constructed(ob)
    g = sc["g"]
    assert N > BLOCK and N % WAVE == TAIL and len(g) == N           # two blocks; a partial last wave, culled
    ogt, omt, ocam = ob.gaussian_transform(sh_deg=3 if sh != SH_NONE else 0), ob.model_transform(), helpers.default_camera(ob, W, H)

    def tiles_of(gg, band=None):
        return np.asarray(ob.preprocess(sh, cov, ob.pack(sh, cov, gg), ogt, omt, ocam, band=band)[1])
    tl = tiles_of(g)
    clipped = np.zeros(N, bool)
    clipped[wave("clipped_away")] = True
    clipped[wave("visible_c").start + CLIPPED_LANE] = True
    for name in WAVES:
        t = tl[wave(name)]
        if name in VISIBLE:
            assert (t[~clipped[wave(name)]] > 0).all(), name
        elif name == "only_lane0":
            assert t[0] > 0 and not t[1:].any()
        elif name == "only_lane63":
            assert t[-1] > 0 and not t[:-1].any()
        else:
            assert not t.any(), name
    assert not tl[clipped].any()
    assert ((tl >= 4) & (tl <= 9)).sum() >= 20                      # rects of 2 .. 3 tiles a side: rect version 4's corner test runs
    # each culled wave is culled for its own reason: undo the reason and all of it is visible
    for name, field, value in (("opacity0", "color", 255), ("clipped_away", "color", 255), ("det", "scale", 0.05)):
        g2 = g.copy()
        if field == "color":
            g2["color"][wave(name), 3] = value
        else:
            g2[field][wave(name)] = value
        assert (tiles_of(g2)[wave(name)] > 0).all(), name
    g2 = g.copy()
    g2["pos"][wave("near"), 2] = -4.0
    g2["pos"][wave("near"), :2] = 0.0
    assert (tiles_of(g2)[wave("near")] > 0).all()
    # the band culls whole waves' worth of Gaussians that the full frame keeps, and keeps others
    tb = tiles_of(g, BAND)
    assert 0 < (tb > 0).sum() < (tl > 0).sum()
    # the selection frame hides some Gaussians of every visible wave and leaves some
    for name in VISIBLE:
        assert 0 < sc["hidden"][wave(name)].sum() < WAVE


# ------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------

def check_frame(r, fr, band, o, rgba, ctx):
    assert fr.flags == 0 and fr.visible == o["V"], "%s: flags %#x, %d visible, the oracle %d" % (ctx, fr.flags, fr.visible, o["V"])
    assert fr.pairs == o["D"], "%s: %d pairs, the oracle %d" % (ctx, fr.pairs, o["D"])
    proj, tiles = r.download_projected(N)
    assert np.array_equal(tiles, o["tiles"]), "%s: tiles touched differ at %s" % (ctx, np.nonzero(tiles != o["tiles"])[0][:8])
    keep = o["tiles"] > 0
    assert proj[keep].tobytes() == o["proj"][keep].tobytes(), "%s: projected records of visible Gaussians differ" % ctx
    keys, idx = r.download_sorted()
    assert np.array_equal(keys, o["keys"]), "%s: sorted keys differ" % ctx
    assert np.array_equal(idx, o["idx"]), "%s: sorted indices differ" % ctx
    assert np.array_equal(r.download_ranges(TILES_X * TILES_Y), o["ranges"]), "%s: tile ranges differ" % ctx
    y0, y1 = band_rows(band, H)
    bad = bits(rgba[y0:y1]) != bits(o["rgba"][y0:y1])
    assert not bad.any(), "%s: %d words of the image differ from the oracle's frame" % (ctx, bad.sum())
    assert (rgba[:y0] == POISON).all() and (rgba[y1:] == POISON).all(), "%s: rows outside the band were written" % ctx


@gpu
@pytest.mark.parametrize("spatial", [False, True], ids=["index-order", "spatial-order"])
@pytest.mark.parametrize("sh,cov", LAYOUTS, ids=LAYOUT_IDS)
def test_constructed_waves(gs, ob, device, stream, sh, cov, spatial):
    sc = constructed(ob)
    pod = gs.GaussianPod(sh, cov)
    pods = pod.from_gaussian(sc["g"])
    assert np.array_equal(np.asarray(pods, dtype=np.uint8).reshape(-1), ob.pack(sh, cov, sc["g"])), "product pack != oracle pack"
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    if not spatial:
        buf.set_spatial_order(False)
    order = buf.download_order(stream)
    expected = ob.spatial_order(sh, cov, ob.pack(sh, cov, sc["g"])) if spatial else np.arange(N, dtype=np.uint32)
    assert np.array_equal(order, expected), "the mirror order is not the one the waves were built for"
    img = gs.Buffer(device, data=np.full(H * W * 4, POISON))
    hide, tint = gs.Selection(device, N), gs.Selection(device, N)
    hide.upload(stream, sc["hidden"])
    tint.upload(stream, sc["tinted"])
    r = gs.Renderer(device)
    cache = {}
    for label, band, sel in frames_of(sh):
        ctx = "layout (%d, %d), %s, frame %s" % (sh, cov, "spatial order" if spatial else "index order", label)
        o = cache.get((band, sel)) or oracle_frame(ob, sh, cov, order, band, sel)
        cache[(band, sel)] = o
        gt = gs.GaussianTransformPod.from_buffer_copy(bytes(o["ogt"]))
        mt = gs.ModelTransformPod.from_buffer_copy(bytes(o["omt"]))
        cam = helpers.copy_camera(o["ocam"], gs.Camera)
        img.write(stream, 0, np.full(H * W * 4, POISON))
        stream.synchronize()
        kw = dict(hide=hide, tint=tint, tint_rgba=walk.TINT_RGBA) if sel else {}
        fr = r.render(stream, buf, gt, mt, cam, img.device_ptr(), band=band, check=True, **kw)
        stream.synchronize()
        rgba = img.download(stream, np.float32).reshape(H, W, 4).copy()
        print("%s: V %d, D %d" % (ctx, fr.visible, fr.pairs))
        check_frame(r, fr, band, o, rgba, ctx)
        if not spatial and band is None and not sel:
            # the culled wave between two visible ones: its slots read "culled", its neighbours' do not
            _, tiles = r.download_projected(N)
            assert not tiles[wave("left")].any() and tiles[wave("visible_a")].any() and tiles[wave("visible_b")].any()
    r.destroy(); hide.destroy(); tint.destroy(); img.release(); buf.destroy()


@gpu
@pytest.mark.parametrize("sh,cov", [(SH_NONE, 0), (SH_SINGLE, 0)], ids=["sh3-cov0", "sh0-cov0"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(gs, ob, device, stream, n, sh, cov):
    """every item boundary of a thread, the partial last block and its partial waves, `inext >= n` of the banded kernel"""
    st = compare_frame(gs, ob, device, stream, sh, cov, synth.scene(n, first=n), W, H,
                       gt_kw=dict(sh_deg=3 if sh != SH_NONE else 0))
    print("n %d: V %d, D %d" % (n, st.visible, st.pairs))


@gpu
@pytest.mark.parametrize("env", [{"GS3D_MASK_REC": "0"}, {"GS3D_MASK_REC": "1"}, {"GS3D_BLOCK_LIST": "1"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_constructed_waves_under_switch(env):
    """GS3D_MASK_REC: culled lanes of k_preprocess_banded do (0) or do not (1) store their records, whatever the mirror
    order; GS3D_BLOCK_LIST=1: every frame of a layout with SH takes k_block_cull's list, its outputs in list space"""
    if any(os.environ.get(k) == v for k, v in env.items()):
        pytest.skip("already running under this switch")
    res = gpu_child.run(["-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_constructed_waves and not switch",
                         "-p", "no:cacheprovider"], env=env, timeout=300, label=",".join("%s=%s" % kv for kv in env.items()))
    assert "%d passed" % (2 * len(LAYOUTS)) in res.stdout and "deselected" in res.stdout, res.stdout[-1000:]
