"""Every record layout through every preprocess path of a frame.  The preprocess stage is compiled once
per record layout (4 SH encodings x 3 covariance encodings) and exists in more path variants than any other stage:
k_tbl_preprocess[nt][sh][cov], k_tbl_preprocess_banded[nt][pipelined][sh][cov], both again with a SelIO argument, and
k_tbl_block_bounds[sh][cov], whose output decides which 1024-Gaussian blocks a frame never reads.  Here ONE renderer per
layout renders one sequence of frames that takes every path — the block test inside the kernel, the block list with the
partial last block on it, a band, a selection frame on each of them, a wholly hidden block, the SH degrees below 3, block
bounds recomputed after a partial update — and every frame is compared with the ORACLE's frame of the same layout: V, D,
tiles touched, the projected records of the visible Gaussians byte for byte, the sorted keys and indices, the tile ranges
and the image bit for bit.

The scene is the renderer walk's buffer P (tests/walk_kinds.py) with the layout swapped: 20 000 Gaussians in
spatial order, 20 mirror blocks, a partial last block of 544, an image of 7 x 5 tiles with partial tiles on both edges and
the walk's corner view, which culls 18 of the 20 blocks.  The figures the paths depend on are the oracle's and are asserted
below without a GPU, for all 12 layouts.

A second, short sequence (enlarged_frames) is there for the covariance bound of k_block_bounds alone, which decides
nothing in the first one; block_test_model says without a GPU what a bound that is too small would lose in each frame.

The same cases run in a child process under GS3D_NT_LOADS=1 (the non-temporal halves of the four tables, which the
renderer picks by itself only above 512 MB of records) and in one under GS3D_PRE_PIPELINE=0 (the serial two-phase
kernels); the switches are read once per process."""
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
import walk_kinds as walk  # noqa: E402
from frames import Scene  # noqa: E402
from helpers import POISON, band_rows, bits  # noqa: E402

gpu = pytest.mark.gpu

N, W, H = walk.N, 100, 70
TILES_X, TILES_Y = (W + 15) // 16, (H + 15) // 16
BLOCK = 1024
NBLOCKS = (N + BLOCK - 1) // BLOCK
CORNER = walk.KINDS["corner"]["cam"]                 # target (13, 7, -3), vfov 25 degrees
BAND = walk.KINDS["band"]["band"]                    # (2, 4)
HIDDEN_BLOCK = 18
MOVED = (5000, 300)                                  # caller indices [5000, 5300): update_range
SH_NONE = walk.SH_NONE
LAYOUTS = [(sh, cov) for sh in range(4) for cov in range(3)]
LAYOUT_IDS = ["sh%d-cov%d" % lc for lc in LAYOUTS]

# the oracle's figures of the scene: (V, D, blocks holding a visible Gaussian)
FIGURES = {"plain": (13993, 18523, 20), "corner": (347, 484, 2), "band": (7620, 9549, 19)}
CORNER_BLOCKS = {18: 120, 19: 227}                   # visible Gaussians per surviving block of the corner view
V_CORNER_HIDDEN, V_PLAIN_HIDDEN, PLAIN_BLOCK_18 = 139, 8116, 342
V_CORNER_MOVED = 636


def _frame(view, band=None, sel=False, deg=None, no_sh0=False, moved=False, size=1.0):
    """every field of a frame; deg None: 3 for layouts with SH, 0 for SH-none; size: GaussianTransform::size"""
    return dict(view=view, band=band, sel=sel, deg=deg, no_sh0=no_sh0, moved=moved, size=size)


def frames_of(sh):
    """the sequence of one layout: (label, frame); the moved range is rewritten ahead of the first `moved` frame"""
    if sh != SH_NONE:
        degrees = [(0, False), (1, True), (2, False), (3, True)]
    else:
        degrees = [(0, False), (0, True)]
    seq = [("1 plain (sizing)", _frame("plain")),
           ("2 corner", _frame("corner")),
           ("3 corner", _frame("corner")),
           ("4 corner + hide + tint", _frame("corner", sel=True)),
           ("5 plain", _frame("plain")),
           ("6 plain + hide + tint", _frame("plain", sel=True)),
           ("7 band", _frame("plain", band=BAND)),
           ("8 band + hide + tint", _frame("plain", band=BAND, sel=True))]
    seq += [("9 plain, degree %d, no_sh0 %s" % (d, z), _frame("plain", deg=d, no_sh0=z)) for d, z in degrees]
    seq += [("10 corner after update_range", _frame("corner", moved=True)),
            ("11 corner after update_range", _frame("corner", moved=True))]
    return seq


SIZE_BIG = 40.0
BAND_TOP, BAND_BOTTOM = (0, 1), (4, 5)


def enlarged_frames():
    """A second, short sequence on a renderer and a buffer of its own.  In the eleven frames above the covariance bound L
    of k_block_bounds decides nothing: the box of every block that holds a visible Gaussian reaches into the view by its
    corners alone (block_test_model below says so with L = 0), so bounds that are wrong for one covariance encoding go
    unnoticed.  With the Gaussians enlarged 40 x (GaussianTransform::size) and a band of one or two tile rows, blocks whose
    boxes lie wholly outside the band hold visible Gaussians, which reach in by their radius alone: only L keeps those blocks."""
    return [("E1 band, enlarged (sizing)", _frame("plain", band=BAND, size=SIZE_BIG)),
            ("E2 band, enlarged", _frame("plain", band=BAND, size=SIZE_BIG)),
            ("E3 bottom tile row, enlarged", _frame("plain", band=BAND_BOTTOM, size=SIZE_BIG)),
            ("E4 top tile row, enlarged", _frame("plain", band=BAND_TOP, size=SIZE_BIG))]


def frame_paths(frames, visible):
    """gsp::plan_use_list, restated: which frames take k_block_cull's list.  A frame of another shape (here: another band)
    than the one before it is a sizing frame and takes the list only when it is a band; every other frame takes it when the
    frame before it saw less than half of the Gaussians.  visible[k]: the oracle's V of frame k."""
    out, shape = [], None
    for k, f in enumerate(frames):
        sizing = f["band"] != shape or k == 0
        out.append(f["band"] is not None if sizing else visible[k - 1] < N // 2)
        shape = f["band"]
    return out


# the paths the sequence is there for (True: the block list); frame 9 is 4 frames for layouts with SH, 2 for SH-none
EXPECTED_PATHS = [False, False, True, True, True, False, True, True]          # frames 1 .. 8


# ------------------------------------------------------------------------------------------------
# the scene and the oracle's frames (no GPU)
# ------------------------------------------------------------------------------------------------

_scene_cache, _pods_cache = {}, {}


def scene(ob):
    """what all 12 layouts share: the Gaussians before and after the update, the mirror order, the masks"""
    if _scene_cache:
        return _scene_cache
    hb = walk.host_buffer(ob, "P")
    g, order = hb["g"], hb["order"]
    hidden, tinted = walk.selection_masks()
    hidden = hidden.copy()
    hidden[order[HIDDEN_BLOCK * BLOCK:(HIDDEN_BLOCK + 1) * BLOCK]] = True         # mirror block 18: sel_block_hidden
    # the moved range: positions copied from Gaussians the corner view sees (buffer P's own layout names them), so that
    # blocks the corner view culled before hold visible Gaussians afterwards
    ocam = helpers.default_camera(ob, W, H, **CORNER)
    _, tiles = ob.preprocess(walk.SH_SINGLE, walk.ROT_SCALE, hb["pods"], ob.gaussian_transform(sh_deg=3), ob.model_transform(), ocam)
    corner_visible = np.nonzero(np.asarray(tiles) > 0)[0]
    rng = np.random.default_rng(3)
    start, count = MOVED
    src = rng.choice(corner_visible, count)
    offsets = rng.normal(0, 0.05, (count, 3)).astype(np.float32)
    g2 = g.copy()
    g2["pos"][start:start + count] = g["pos"][src] + offsets
    _scene_cache.update(g=g, g2=g2, order=order, hidden=hidden, tinted=tinted)
    return _scene_cache


def layout_pods(ob, sh, cov, moved=False):
    key = (sh, cov, moved)
    if key not in _pods_cache:
        sc = scene(ob)
        _pods_cache[key] = ob.pack(sh, cov, sc["g2"] if moved else sc["g"])
    return _pods_cache[key]


def frame_transforms(ob, sh, f):
    deg = f["deg"] if f["deg"] is not None else (3 if sh != SH_NONE else 0)
    ogt = ob.gaussian_transform(size=f["size"], sh_deg=deg, no_sh0=f["no_sh0"])
    ocam = helpers.default_camera(ob, W, H, **(CORNER if f["view"] == "corner" else {}))
    return ogt, ob.model_transform(), ocam


def oracle_preprocess(ob, sh, cov, f):
    """(proj, tiles) of a frame: a selection frame through its twin records (hidden: opacity byte 0) and the tint
    recolouring, as tests/test_gpu_selection.py and the walk build them"""
    sc = scene(ob)
    pods = layout_pods(ob, sh, cov, f["moved"])
    if f["sel"]:
        pods = Scene.twin_pods(types.SimpleNamespace(pods=pods, n=N), sc["hidden"])
    ogt, omt, ocam = frame_transforms(ob, sh, f)
    proj, tiles = ob.preprocess(sh, cov, pods, ogt, omt, ocam, band=f["band"])
    if f["sel"]:
        walk.recolour(proj, sc["tinted"])
    return proj, tiles, (ogt, omt, ocam)


def oracle_frame(ob, sh, cov, f, cache):
    """cache: the caller's, for the frames a sequence repeats (a layout's frames serve one test only)"""
    key = tuple(sorted(f.items(), key=lambda kv: kv[0]))
    if key in cache:
        return cache[key]
    proj, tiles, (ogt, omt, ocam) = oracle_preprocess(ob, sh, cov, f)
    keys, idx = ob.build_keys(proj, tiles, TILES_X, order=scene(ob)["order"])
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, TILES_X * TILES_Y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=f["band"], gt=ogt)
    tl = np.asarray(tiles)
    o = dict(proj=proj, tiles=tl, keys=skeys, idx=sidx, ranges=ranges, rgba=rgba, V=int((tl > 0).sum()),
             D=int(tl.astype(np.uint64).sum()), ogt=ogt, omt=omt, ocam=ocam)
    cache[key] = o
    return o


def visible_per_block(ob, tiles):
    """visible Gaussians of every mirror block (the last one is partial)"""
    slots = np.zeros(NBLOCKS * BLOCK, dtype=np.int64)
    slots[:N] = np.asarray(tiles)[scene(ob)["order"]] > 0
    return slots.reshape(NBLOCKS, BLOCK).sum(axis=1)


def _counts(ob, sh, cov, f):
    _, tiles, _ = oracle_preprocess(ob, sh, cov, f)
    tl = np.asarray(tiles)
    return int((tl > 0).sum()), int(tl.astype(np.uint64).sum()), visible_per_block(ob, tl), tl


def test_the_scene_is_the_walks():
    assert (N, NBLOCKS, N - (NBLOCKS - 1) * BLOCK) == (20000, 20, 544)
    assert (TILES_X, TILES_Y, W % 16, H % 16) == (7, 5, 4, 6)
    assert walk.KINDS["plain"]["W"] == W and walk.KINDS["plain"]["H"] == H
    assert CORNER == dict(target=(13, 7, -3), vfov_deg=25.0) and BAND == (2, 4)
    assert MOVED[1] <= N // 4                 # a partial update this small keeps the mirror order


@pytest.mark.parametrize("sh,cov", LAYOUTS, ids=LAYOUT_IDS)
def test_oracle_figures_of_every_layout(ob, sh, cov):
    """every condition the GPU sequence relies on, from the oracle alone.  The figures hold for all 12 layouts (the mirror
    order depends on positions only, and no count sits within an f16 covariance's rounding of a threshold)."""
    sc = scene(ob)
    order, hidden = sc["order"], sc["hidden"]
    assert np.array_equal(ob.spatial_order(sh, cov, layout_pods(ob, sh, cov)), order), "the order depends on the layout"
    # V, D and the survivor blocks of the three views
    per_block = {}
    for name, f in (("plain", _frame("plain")), ("corner", _frame("corner")), ("band", _frame("plain", band=BAND))):
        V, D, blocks, _ = _counts(ob, sh, cov, f)
        per_block[name] = blocks
        print("%s: V %d, D %d, %d of %d blocks" % (name, V, D, (blocks > 0).sum(), NBLOCKS))
        assert (V, D, int((blocks > 0).sum())) == FIGURES[name], name
    assert per_block["plain"].min() > 0
    # the corner's survivors: block 18 and the partial last block
    corner = per_block["corner"]
    assert {int(b): int(corner[b]) for b in np.nonzero(corner)[0]} == CORNER_BLOCKS
    assert NBLOCKS - 1 in CORNER_BLOCKS and N % BLOCK != 0
    assert int(per_block["band"].min()) == 0 and (per_block["band"] > 0).sum() < NBLOCKS
    # the hide mask: block 18 is wholly hidden, and it holds visible Gaussians in both views before hiding
    assert hidden[order[HIDDEN_BLOCK * BLOCK:(HIDDEN_BLOCK + 1) * BLOCK]].all()
    for b in range(NBLOCKS):
        if b != HIDDEN_BLOCK:
            assert not hidden[order[b * BLOCK:(b + 1) * BLOCK]].all(), "only block %d may be wholly hidden" % HIDDEN_BLOCK
    assert per_block["plain"][HIDDEN_BLOCK] == PLAIN_BLOCK_18 and corner[HIDDEN_BLOCK] > 0
    V, _, blocks, tl = _counts(ob, sh, cov, _frame("corner", sel=True))
    assert V == V_CORNER_HIDDEN and blocks[NBLOCKS - 1] == V and not tl[hidden].any()
    V, _, blocks, tl = _counts(ob, sh, cov, _frame("plain", sel=True))
    assert V == V_PLAIN_HIDDEN and blocks[HIDDEN_BLOCK] == 0 and not tl[hidden].any()
    # the moved range: visible afterwards, most of it in blocks the corner view culled before
    start, count = MOVED
    moved = np.arange(start, start + count)
    _, _, _, tl0 = _counts(ob, sh, cov, _frame("corner"))
    V, _, blocks, tl1 = _counts(ob, sh, cov, _frame("corner", moved=True))
    slot_of = np.empty(N, dtype=np.int64)
    slot_of[order] = np.arange(N)
    in_culled = (tl1[moved] > 0) & (corner[slot_of[moved] // BLOCK] == 0)
    print("moved: %d visible before, %d after, %d of them in blocks culled before; V %d" %
          ((tl0[moved] > 0).sum(), (tl1[moved] > 0).sum(), in_culled.sum(), V))
    assert ((tl0[moved] > 0).sum(), (tl1[moved] > 0).sum(), int(in_culled.sum())) == (7, 296, 271)
    assert in_culled.sum() >= 200, "stale bounds would not change V"
    assert V == V_CORNER_MOVED and V < N // 2
    # the list / in-kernel decision of every frame
    seq = [f for _, f in frames_of(sh)]
    visible = [_counts(ob, sh, cov, f)[0] for f in seq]
    paths = frame_paths(seq, visible)
    nine = len(seq) - 10
    assert nine == (4 if sh != SH_NONE else 2)
    assert paths == EXPECTED_PATHS + [False] * nine + [False, True], paths
    assert visible[8:8 + nine] == [FIGURES["plain"][0]] * nine       # the SH degree moves no count


_model_cache = {}


def block_test_model(ob, f, shrink):
    """block_is_culled (gs_render_kernels.h) restated in float64 without its slack for f32 rounding, for the identity
    model transform: which blocks the test drops in frame f when every block's L is divided by `shrink` (inf: L = 0).
    L here is the largest Frobenius norm of a block's covariances, diag(scale^2) rotated — an upper bound of what
    k_block_bounds stores (it keeps the smaller of that and the largest row sum), so a block this model drops, the kernel
    with the same shrunken bound drops too."""
    key = (f["view"], f["band"], f["moved"], f["size"], shrink)         # (the model knows no layout)
    if key in _model_cache:
        return _model_cache[key]
    sc = scene(ob)
    g, order = sc["g2"] if f["moved"] else sc["g"], sc["order"]
    _, _, ocam = frame_transforms(ob, 0, f)
    view = np.array(list(ocam.view), dtype=np.float64).reshape(4, 4).T          # (column-major)
    frob = np.sqrt((g["scale"].astype(np.float64) ** 4).sum(axis=1))
    ty0, ty1 = f["band"] if f["band"] is not None else (0, TILES_Y)
    culled = np.zeros(NBLOCKS, bool)
    for b in range(NBLOCKS):
        idx = order[b * BLOCK:(b + 1) * BLOCK]
        lo, hi = g["pos"][idx].min(axis=0).astype(np.float64), g["pos"][idx].max(axis=0).astype(np.float64)
        corners = np.array([[(hi if c >> a & 1 else lo)[a] for a in range(3)] + [1.0] for c in range(8)]) @ view.T
        xv, yv, zv = corners[:, 0], -corners[:, 1], -corners[:, 2]
        if zv.max() <= ocam.near_plane or zv.min() >= ocam.far_plane:
            culled[b] = True
            continue
        if zv.min() <= 0.0:
            continue
        zl = max(zv.min(), ocam.near_plane)
        u, v = xv / zv, yv / zv
        ub = min(np.abs(u).max(), 1.3 * 0.5 * ocam.width / ocam.fx)
        vb = min(np.abs(v).max(), 1.3 * 0.5 * ocam.height / ocam.fy)
        ja, jc, jb = ocam.fx ** 2 * (1.0 + ub * ub), ocam.fy ** 2 * (1.0 + vb * vb), abs(ocam.fx * ocam.fy) * ub * vb
        jn = 0.5 * (ja + jc) + np.sqrt(0.25 * (ja - jc) ** 2 + jb * jb)
        lam = f["size"] ** 2 * jn * (frob[idx].max() / shrink) / (zl * zl) + 0.7
        r = 3.0 * np.sqrt(lam) * 1.001 + 1.01 + 0.05
        mx, my = ocam.fx * u + ocam.cx, ocam.fy * v + ocam.cy
        culled[b] = (mx.max() + r < 0.0 or mx.min() - r >= 16.0 * TILES_X or my.max() + r < 16.0 * ty0 or
                     my.min() - r >= 16.0 * ty1)
    _model_cache[key] = culled
    return culled


@pytest.mark.parametrize("sh,cov", LAYOUTS, ids=LAYOUT_IDS)
def test_oracle_conditions_of_the_enlarged_frames(ob, sh, cov):
    """what a covariance bound that is too small would lose, by block_test_model: nothing in the eleven frames, whatever
    the bound (the bound of a block is its largest Gaussian's, a hundred times the median's: even where a block lies
    outside the view, a bound 4 x too small keeps it).  Of the enlarged frames, a vanishing bound loses Gaussians in E1 / E2,
    E3 and E4, one 64 x too small in E3 and E4, one 16 x too small in E3."""
    def lost(f, shrinks):
        """{shrink: (visible Gaussians, blocks holding some) in the blocks the model drops}"""
        _, tiles, _ = oracle_preprocess(ob, sh, cov, f)
        vis = visible_per_block(ob, np.asarray(tiles))
        return {k: (int(vis[c].sum()), int((c & (vis > 0)).sum())) for k in shrinks for c in [block_test_model(ob, f, k)]}
    for _, f in frames_of(sh):
        if not f["sel"]:        # (a hidden Gaussian only takes away)
            assert lost(f, (1.0, np.inf)) == {1.0: (0, 0), np.inf: (0, 0)}, f
    seq = enlarged_frames()
    found = {label[:2]: lost(f, (1.0, 4.0, 16.0, 64.0, np.inf)) for label, f in seq}
    print("enlarged frames, {bound divided by: (visible Gaussians, blocks) lost} = %s" % found)
    for e in found.values():
        assert e[1.0] == (0, 0)
    assert found["E1"] == found["E2"] and found["E1"][np.inf][0] >= 100
    assert found["E3"][16.0][0] >= 5 and found["E3"][64.0][0] >= 10 and found["E3"][np.inf] >= (500, 8)
    assert found["E4"][64.0][0] >= 40 and found["E4"][np.inf] >= (500, 6)
    # E1 sizes the pair buffers and, a band, takes the list; E2 follows a frame that saw more than half; E3 and E4 are new shapes
    visible = [int((np.asarray(oracle_preprocess(ob, sh, cov, f)[1]) > 0).sum()) for _, f in seq]
    assert frame_paths([f for _, f in seq], visible) == [True, False, True, True]


# ------------------------------------------------------------------------------------------------
# the sequence on the device
# ------------------------------------------------------------------------------------------------

def _list_rule_is_the_renderers_own():
    return not (os.environ.get("GS3D_BLOCK_LIST") or os.environ.get("GS3D_BLOCK_CULL") == "0" or
                os.environ.get("GS3D_FORCE_BANDED"))


def check_frame(r, fr, f, o, rgba, ctx):
    assert fr.flags == 0 and fr.visible == o["V"], "%s: flags %#x, %d visible, the oracle %d" % (ctx, fr.flags, fr.visible, o["V"])
    assert fr.pairs == o["D"], "%s: %d pairs, the oracle %d" % (ctx, fr.pairs, o["D"])
    proj, tiles = r.download_projected(N)
    assert np.array_equal(tiles, o["tiles"]), "%s: tiles touched differ at %d Gaussians" % (ctx, (tiles != o["tiles"]).sum())
    keep = o["tiles"] > 0
    assert proj[keep].tobytes() == o["proj"][keep].tobytes(), "%s: projected records of visible Gaussians differ" % ctx
    keys, idx = r.download_sorted()
    assert np.array_equal(keys, o["keys"]), "%s: sorted keys differ" % ctx
    assert np.array_equal(idx, o["idx"]), "%s: sorted indices differ" % ctx
    assert np.array_equal(r.download_ranges(TILES_X * TILES_Y), o["ranges"]), "%s: tile ranges differ" % ctx
    y0, y1 = band_rows(f["band"], H)
    bad = bits(rgba[y0:y1]) != bits(o["rgba"][y0:y1])
    assert not bad.any(), "%s: %d words of the image differ from the oracle's frame" % (ctx, bad.sum())
    assert (rgba[:y0] == POISON).all() and (rgba[y1:] == POISON).all(), "%s: rows outside the band were written" % ctx


def run_sequence(gs, ob, device, stream, sh, cov, seq):
    """one buffer, one renderer, one image poisoned before every frame; returns (took the list?, launches) per frame"""
    sc = scene(ob)
    cache = {}
    oracle = [oracle_frame(ob, sh, cov, f, cache) for _, f in seq]
    paths = frame_paths([f for _, f in seq], [o["V"] for o in oracle])
    pod = gs.GaussianPod(sh, cov)
    pods = pod.from_gaussian(sc["g"])
    assert np.array_equal(np.asarray(pods, dtype=np.uint8).reshape(-1), layout_pods(ob, sh, cov)), "product pack != oracle pack"
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    assert np.array_equal(buf.download_order(stream), sc["order"]), "the mirror order is not the oracle's spatial order"
    img = gs.Buffer(device, data=np.full(H * W * 4, POISON))
    hide, tint = gs.Selection(device, N), gs.Selection(device, N)
    hide.upload(stream, sc["hidden"])
    tint.upload(stream, sc["tinted"])
    r = gs.Renderer(device)
    launches = []
    for k, (label, f) in enumerate(seq):
        path = "no block test" if sh == SH_NONE else "block list" if paths[k] else "block test in the kernel"
        ctx = "layout (%d, %d), frame %s [%s]" % (sh, cov, label, path)
        if f["moved"] and not seq[k - 1][1]["moved"]:
            start, count = MOVED
            buf.update_range(stream, start, sc["g2"][start:start + count])
            assert np.array_equal(buf.download_order(stream), sc["order"]), "a partial update must keep the mirror order"
        ogt, omt, ocam = oracle[k]["ogt"], oracle[k]["omt"], oracle[k]["ocam"]
        gt = gs.GaussianTransformPod.from_buffer_copy(bytes(ogt))
        mt = gs.ModelTransformPod.from_buffer_copy(bytes(omt))
        cam = helpers.copy_camera(ocam, gs.Camera)
        img.write(stream, 0, np.full(H * W * 4, POISON))
        stream.synchronize()
        kw = dict(hide=hide, tint=tint, tint_rgba=walk.TINT_RGBA) if f["sel"] else {}
        fr = r.render(stream, buf, gt, mt, cam, img.device_ptr(), band=f["band"], check=True, **kw)
        stream.synchronize()
        rgba = img.download(stream, np.float32).reshape(H, W, 4).copy()
        launches.append(fr.launches)
        print("%s: V %d, D %d, %d launches" % (ctx, fr.visible, fr.pairs, fr.launches))
        check_frame(r, fr, f, oracle[k], rgba, ctx)
    r.destroy(); hide.destroy(); tint.destroy(); img.release(); buf.destroy()
    return paths, launches


def check_list_launch(sh, paths, launches, k, what):
    """frames k - 1 and k are the same frame, the first with the block test in the kernel, the second on the list: the
    list is one launch (k_block_cull) ahead of the preprocess kernel.  SH-none layouts have no block test."""
    assert paths[k - 1] is False and paths[k] is True, paths
    if _list_rule_is_the_renderers_own():
        assert launches[k] == launches[k - 1] + (1 if sh != SH_NONE else 0), "%s: %s" % (what, launches)


@gpu
@pytest.mark.parametrize("sh,cov", LAYOUTS, ids=LAYOUT_IDS)
def test_every_path_of_a_layout(gs, ob, device, stream, sh, cov):
    """the eleven frames of the module docstring: which table and which path each takes is DESIGN.md §4.4's table"""
    paths, launches = run_sequence(gs, ob, device, stream, sh, cov, frames_of(sh))
    check_list_launch(sh, paths, launches, 2, "frame 3 against frame 2")
    check_list_launch(sh, paths, launches, len(paths) - 1, "frame 11 against frame 10")


@gpu
@pytest.mark.parametrize("sh,cov", LAYOUTS, ids=LAYOUT_IDS)
def test_enlarged_gaussians_reach_in_from_blocks_outside_the_view(gs, ob, device, stream, sh, cov):
    """enlarged_frames(): the frames in which k_block_bounds' covariance bound of this layout decides what is visible"""
    paths, _ = run_sequence(gs, ob, device, stream, sh, cov, enlarged_frames())
    assert paths == [True, False, True, True]


# ------------------------------------------------------------------------------------------------
# the same cases under GS3D_NT_LOADS=1 and under GS3D_PRE_PIPELINE=0: one child process per switch, one at a time
# ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("env", [{"GS3D_NT_LOADS": "1"}, {"GS3D_PRE_PIPELINE": "0"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_every_path_of_every_layout_under_switch(env):
    """GS3D_NT_LOADS=1: k_preprocess<.., true>, k_preprocess_banded<.., true, true>, with and without SelIO — what the
    renderer picks by itself for every scene above 512 MB of records.  GS3D_PRE_PIPELINE=0: k_preprocess_banded<.., false,
    false>, with and without SelIO."""
    if any(os.environ.get(k) == v for k, v in env.items()):
        pytest.skip("already running under this switch")
    res = gpu_child.run(["-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu",
                         "-k", "test_every_path_of_a_layout or test_enlarged_gaussians", "-p", "no:cacheprovider"],
                        env=env, timeout=300, label=",".join("%s=%s" % kv for kv in env.items()))
    assert "%d passed" % (2 * len(LAYOUTS)) in res.stdout and "deselected" in res.stdout, res.stdout[-1000:]
