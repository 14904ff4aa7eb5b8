"""The frame kinds of the renderer walk (tests/test_gpu_renderer_walk.py; tests/test_gpu_layout_paths.py swaps the layout of
its buffer P): the buffers, the kinds, and the oracle's frame of every kind, computed once per process and without a GPU."""
import types

import numpy as np

import helpers
import rounds_np
import synth
from frames import Scene, tint32
from planes import oracle_depth, pick_witness

ROUND1 = 2048
N = 20000
TINT_RGBA = (1.0, 0.25, 0.0, 0.5)
SH_SINGLE, SH_NONE, ROT_SCALE, COV_HALF = 0, 3, 0, 2      # gs.SH_* / gs.COV3D_*

# buffers, created once per walk.  P' holds P's Gaussians in index order; E is new_empty(device, pod, 0)
BUFFERS = {
    "P": dict(sh=SH_SINGLE, cov=ROT_SCALE, n=N, first=0),
    "P'": dict(sh=SH_SINGLE, cov=ROT_SCALE, n=N, first=0, spatial=False),
    "Q": dict(sh=SH_NONE, cov=COV_HALF, n=N, first=777, scale=40.0),
    "R": dict(sh=SH_NONE, cov=ROT_SCALE, n=N, first=31, opacity=250, scale=10.0),
    "S": dict(sh=SH_NONE, cov=COV_HALF, n=3000, first=0),
    "E": dict(sh=SH_NONE, cov=ROT_SCALE, n=0),
}


def _kind(buf, W=100, H=70, band=None, cam=None, mode=0, std=3.0, aux=False, sel=False, sort=(-1, -1), rounds=(0, 0),
          masks=1, background=None):
    """every field of a frame: nothing is inherited from the frame before (sort = set_sort_mode, rounds = set_rounds,
    masks = set_tile_masks)"""
    return dict(buf=buf, W=W, H=H, band=band, cam=cam or {}, mode=mode, std=std, aux=aux, sel=sel, sort=sort, rounds=rounds,
                masks=masks, background=background, sh_deg=3 if BUFFERS[buf]["sh"] != SH_NONE else 0)


KINDS = {
    # V 13 993, D 18 523, longest list 1 060: banded preprocess, the block test inside the kernel, G = 8 blend; partial tiles on
    # both edges, a last tile row of 6 pixel rows
    "plain": _kind("P"),
    # V 7 620, D 9 549: a band's shape; block list on a shape's first frame; rows outside the band keep the poison
    "band": _kind("P", band=(2, 4)),
    # V 347, D 484: V < n / 2, so the next frame, whatever its kind, starts from use_list = true (History::newest_any)
    "corner": _kind("P", cam=dict(target=(13, 7, -3), vfov_deg=25.0)),
    # index order: last_order null, culled records written, LSD depth sort
    "index": _kind("P'", sort=(0, -1)),
    # V 18 161, D 154 605, longest list 6 968: plain's shape; k_preprocess; lists of many staging batches; 8 x the pairs
    "fat": _kind("Q", sort=(1, -1)),
    # no rect clipping in this mode; rect version 3 pinned (the oracle follows: ob.set_rect_version)
    "ellipse": _kind("Q", mode=1, std=1.5, masks=0),
    "point": _kind("P", mode=2),
    # the AUX instantiations: depth + pick planes
    "aux": _kind("P", aux=True),
    # the slot-mask cache: 40 % hidden, 20 % tinted
    "hide": _kind("P", sel=True),
    # ... and THE SAME two Selection objects on another buffer of the same length: a mask gathered through P's mirror order
    # must not serve Q (SlotMaskKey::buffer)
    "hide_q": _kind("Q", sel=True),
    # V 15 209, D 35 140: two rounds; unpartitioned after a kind of another shape (a sizing frame), partitioned after any
    # kind of 20 000 Gaussians on the full 100 x 70 image, single-round ones included
    "rounds": _kind("R", rounds=(1, ROUND1)),
    # V 2 027, D 2 451, 6 tiles: another n and size — a sizing frame on entry and on exit; a tile sort of one pass leaves the
    # pairs on the other side
    "small": _kind("S", W=48, H=32),
    # stage_empty_frame: both sorted sides := 0, image = background
    "empty": _kind("E", background=(0.25, 0.5, 0.75)),
}
NAMES = list(KINDS)
FIGURES = {      # kind: (V, D, longest tile list or None)
    "plain": (13993, 18523, 1060), "band": (7620, 9549, None), "corner": (347, 484, None),
    "fat": (18161, 154605, 6968), "rounds": (15209, 35140, None), "small": (2027, 2451, None), "empty": (0, 0, 0),
}
SAME_SHAPE_AS_ROUNDS = [k for k, v in KINDS.items() if BUFFERS[v["buf"]]["n"] == N and (v["W"], v["H"], v["band"]) == (100, 70, None)]


def walk_sequence():
    return [NAMES[i] for i in helpers.pair_walk(len(NAMES))]


def selection_masks():
    rng = np.random.default_rng(40)
    return rng.random(N) < 0.4, rng.random(N) < 0.2          # hidden, tinted


# ------------------------------------------------------------------------------------------------
# the oracle's frame of every kind (no GPU)
# ------------------------------------------------------------------------------------------------

_host_cache, _oracle_cache = {}, {}


def host_buffer(ob, b):
    """Gaussians, records and the mirror order of a freshly created buffer (the walk asserts that the
    device's order IS this one before it renders anything)"""
    if b not in _host_cache:
        spec = BUFFERS[b]
        n = spec["n"]
        if n:
            g = synth.scene(n, first=spec["first"])
            if "opacity" in spec:
                g["color"][:, 3] = spec["opacity"]
            if "scale" in spec:
                g["scale"] *= np.float32(spec["scale"])
            pods = ob.pack(spec["sh"], spec["cov"], g)
        else:
            g, pods = np.zeros(0, dtype=ob.GAUSSIAN_DTYPE), np.zeros(0, dtype=np.uint8)
        spatial = spec.get("spatial", True) and n > 1
        order = ob.spatial_order(spec["sh"], spec["cov"], pods) if spatial else np.arange(n, dtype=np.uint32)
        _host_cache[b] = dict(g=g, pods=pods, order=order)
    return _host_cache[b]


def recolour(proj, tinted):
    for ch, t in zip("rgb", TINT_RGBA[:3]):
        proj[ch][tinted] = tint32(proj[ch][tinted], TINT_RGBA[3], t)


def kind_transforms(ob, name):
    k = KINDS[name]
    ogt = ob.gaussian_transform(mode=k["mode"], sh_deg=k["sh_deg"], max_std_dev=k["std"])
    omt = ob.model_transform()
    ocam = helpers.default_camera(ob, k["W"], k["H"], **k["cam"])
    if k["background"] is not None:
        ocam.background[:] = list(k["background"])
    return ogt, omt, ocam


def oracle_frame(ob, name):
    """built as tests/frames.py's oracle_stages is, order = the buffer's mirror order; a selection kind through its
    twin (hidden: opacity byte 0) and test_tint's recolouring; the aux kind with its depth plane and the float64 pick walk"""
    if name in _oracle_cache:
        return _oracle_cache[name]
    k = KINDS[name]
    spec, hb = BUFFERS[k["buf"]], host_buffer(ob, k["buf"])
    sh, cov, n, W, H = spec["sh"], spec["cov"], spec["n"], k["W"], k["H"]
    pods = hb["pods"]
    hidden, tinted = selection_masks()
    if k["sel"]:
        pods = Scene.twin_pods(types.SimpleNamespace(pods=pods, n=n), hidden)
    ogt, omt, ocam = kind_transforms(ob, name)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    version = ob.rect_version()
    try:
        ob.set_rect_version(4 if k["masks"] else 3)
        proj, tiles = ob.preprocess(sh, cov, pods, ogt, omt, ocam, band=k["band"])
        if k["sel"]:
            recolour(proj, tinted)
        keys, idx = ob.build_keys(proj, tiles, tiles_x, order=hb["order"])
    finally:
        ob.set_rect_version(version)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=k["band"], gt=ogt)
    tl = np.asarray(tiles)
    o = dict(proj=proj, tiles=tl, rows=tiles.rows, keys=skeys, idx=sidx, ranges=ranges, rgba=rgba, V=int((tl > 0).sum()),
             D=int(tl.astype(np.uint64).sum()), longest=int((ranges[:, 1] - ranges[:, 0]).max()), tiles_x=tiles_x,
             num_tiles=tiles_x * tiles_y, ogt=ogt, omt=omt, ocam=ocam)
    if k["aux"]:
        o["depth"] = oracle_depth(ob, proj, sidx, ranges, ocam, ogt, k["band"])
        o["pick"], o["pick_ambiguous"] = pick_witness(proj, sidx, ranges, W, H, tiles_x, float(np.float32(1.0) - np.float32(0.5)))
    if k["rounds"][0] == 1:
        o["finished"], o["open"] = round1_coverage(o, hb["order"], W, H, k["rounds"][1])
        # the exact counts of the frame, unpartitioned and partitioned (tests/rounds_np.py)
        with_rows = tl.view(ob.TilesTouched)
        with_rows.rows = tiles.rows
        o["model"] = [rounds_np.frame(ob, proj, with_rows, hb["order"], ocam, ogt, k["band"], k["rounds"][1], part, n=n)
                      for part in (0, 1)]
    _oracle_cache[name] = o
    return o


def round1_coverage(o, order, W, H, round1):
    """the numbers of certainly finished and of certainly open tiles (round1_coverage_masks)"""
    finished, opened = round1_coverage_masks(o, order, W, H, round1)
    return int(finished.sum()), int(opened.sum())


def round1_coverage_masks(o, order, W, H, round1):
    """(certainly finished, certainly open) tiles, one bool per tile, after a round 1 of the nearest `round1` visible
    Gaussians (an unpartitioned frame's): a float64 walk of the oracle's lists restricted to them.  A pixel that meets a
    step with T (1 - alpha) < 0.999e-4 has certainly stopped; one that never meets a step below 1.001e-4 is certainly still
    open (f32 rounding does not cross 0.1 %); a step in between is taken as not stopping, and leaves the pixel undecided
    unless a later step stops it for certain — which the next active step does, whichever way the kernel decided: it
    multiplies a T of ~1e-4 by at most 1 - 1/255.  A tile is finished when every in-image pixel has stopped, open when one
    is open; a tile with an undecided pixel and no open one is neither."""
    proj, sidx, ranges = o["proj"], o["idx"], o["ranges"]
    vis = order[o["tiles"][order] > 0]
    near = vis[np.argsort(proj["depth"][vis], kind="stable")][:round1]
    member = np.zeros(len(proj), bool)
    member[near] = True
    p = {f: proj[f].astype(np.float64) for f in ("mx", "my", "ca", "cb", "cc", "opacity")}
    finished, opened = np.zeros(ranges.shape[0], bool), np.zeros(ranges.shape[0], bool)
    for t in range(ranges.shape[0]):
        tx, ty = t % o["tiles_x"], t // o["tiles_x"]
        xs, ys = np.arange(tx * 16, min(tx * 16 + 16, W)), np.arange(ty * 16, min(ty * 16 + 16, H))
        px, py = [a.ravel() for a in np.meshgrid(xs + 0.5, ys + 0.5)]
        T = np.ones(px.shape)
        stopped = np.zeros(px.shape, bool)
        maybe = np.zeros(px.shape, bool)
        for j in range(int(ranges[t, 0]), int(ranges[t, 1])):
            g = int(sidx[j])
            if not member[g]:
                continue
            dx, dy = p["mx"][g] - px, p["my"][g] - py
            power = p["ca"][g] * dx * dx + p["cb"][g] * dx * dy + p["cc"][g] * dy * dy
            alpha = np.minimum(0.99, p["opacity"][g] * np.exp(power))
            act = ~stopped & (power <= 0.0) & (alpha >= 1.0 / 255.0)
            Tn = T * (1.0 - alpha)
            maybe |= act & (Tn < 1.001e-4)
            sure = act & (Tn < 0.999e-4)
            stopped |= sure
            T = np.where(act & ~sure, Tn, T)
        finished[t] = stopped.all()
        opened[t] = (~maybe).any()
    return finished, opened
