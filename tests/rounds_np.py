"""numpy restatement of DESIGN.md §4.2 "rounds" (the count rules of a two-round frame), written from the text over the
oracle's stage outputs: which Gaussians round 1 renders, which tiles its blend finishes and leaves open, which of the
other Gaussians round 2 still emits, and what the frame then reports (gs_frame_result.visible / .pairs,
gs_sort_info.rounds / .round1 / .partitioned / .tiles_done).  The only arithmetic is the oracle's own blend
(binding.blend(..., stopped=True)); everything else is integer bookkeeping.  Shares no code with the library."""
import numpy as np

TOP_BITS = 10            # the depth key's top digit a partitioned frame cuts at
STEP = 2048              # round 1's length is a multiple of it


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def depth_key_bits(near, far):
    """(bits(max(near, 0)), width of the depth keys bits(depth) - bits(max(near, 0)) of depths in (near, far))"""
    nb = f32_bits(max(float(near), 0.0))
    fb = f32_bits(far) if far > 0 else 0
    return nb, ((fb - nb).bit_length() if fb > nb else 0)


def round1_length(K, n):
    """K' = K rounded up to a multiple of 2 048; 0 (a single round) when that leaves nothing of the buffer's n Gaussians
    for a second round"""
    k = (int(K) + STEP - 1) // STEP * STEP
    return k if k < n else 0


def is_partitioned(near, far, requested):
    """a frame asked to be partitioned is, when the depth keys have more bits than the top digit"""
    return bool(requested) and depth_key_bits(near, far)[1] > TOP_BITS


def visible_in_order(tiles, order):
    """the visible Gaussians in mirror order"""
    order = np.asarray(order)
    return order[np.asarray(tiles)[order] > 0]


def round1_members(proj, tiles, order, near, far, K, partitioned):
    """mask of the Gaussians round 1 renders; K = round1_length(...) > 0.  Unpartitioned: the nearest K visible ones, ties in
    the mirror's order (the depth sort is stable).  Partitioned: the keys bits(depth) - bits(max(near, 0)) below
    (d + 1) << low_bits, low_bits = key bits - 10, d the smallest value of the key's top 10 bits with at least K visible
    Gaussians at or below it; all of them when fewer than K are visible."""
    vis = visible_in_order(tiles, order)
    depth = np.ascontiguousarray(proj["depth"][vis])
    m = np.zeros(len(proj), bool)
    if not partitioned:
        m[vis[np.argsort(depth, kind="stable")][:K]] = True
        return m
    near_bits, dbits = depth_key_bits(near, far)
    assert dbits > TOP_BITS
    low_bits = dbits - TOP_BITS
    dkey = depth.view(np.uint32).astype(np.int64) - near_bits
    assert (dkey >= 0).all() and (dkey >> low_bits < 1 << TOP_BITS).all(), "a visible depth outside (near, far)"
    upto = np.cumsum(np.bincount(dkey >> low_bits, minlength=1 << TOP_BITS))
    tau = (int(np.searchsorted(upto, K)) + 1) << low_bits if upto[-1] >= K else 1 << 32
    m[vis[dkey < tau]] = True
    return m


def blend_lists(ob, proj, tiles, order, camera, gt, band, stopped=False):
    """the oracle's blend of the lists that `tiles` describes (build, sort, ranges, blend): (ranges, blend's result)"""
    tiles_x, tiles_y = (camera.width + 15) // 16, (camera.height + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    return ranges, ob.blend(proj, sidx, ranges, camera, band=band, gt=gt, stopped=stopped)


def tile_all(plane, W, H):
    """[tiles_y, tiles_x]: every in-image pixel of the tile is set"""
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    full = np.ones((tiles_y * 16, tiles_x * 16), bool)
    full[:H, :W] = plane != 0
    return full.reshape(tiles_y, 16, tiles_x, 16).all(axis=(1, 3))


def touched_tiles(proj, rows, i):
    """the tiles Gaussian i emits pairs for: its box, or what the row code of a masked (version-4) rect keeps of it — 4 bits
    per tile row: (first kept column) | (kept columns) << 2"""
    tx0, ty0, tx1, ty1 = (int(proj[f][i]) for f in ("tx0", "ty0", "tx1", "ty1"))
    code = int(rows[i]) if rows is not None else 0
    if not code & 0x8000:
        return [(ty, tx) for ty in range(ty0, ty1) for tx in range(tx0, tx1)]
    out = []
    for j in range(ty1 - ty0):
        nib = (code >> (4 * j)) & 15
        out += [(ty0 + j, tx0 + (nib & 3) + c) for c in range(nib >> 2)]
    return out


def frame(ob, proj, tiles, order, camera, gt, band, K, partitioned, n=None):
    """The model of one frame rendered with set_rounds(1, K): a dict of
      rounds, round1, partitioned, visible, pairs, tiles_done      what the device reports
      D, D1, pairs_undropped                                      the oracle's pairs, round 1's, and D1 + the others'
      member, done, open [tiles_y, tiles_x], gated, band_tiles
      rest, dropped, survivors (index arrays), small, masked (masks over all Gaussians)
    `tiles` carries .rows where rect version 4 is on; n: the buffer's length (default: len(proj))."""
    W, H = camera.width, camera.height
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    tl = np.asarray(tiles).astype(np.int64)
    rows = getattr(tiles, "rows", None)
    n = len(proj) if n is None else n
    b0, b1 = band if band is not None else (0, tiles_y)
    b1 = min(b1, tiles_y)
    out = dict(visible=int((tl > 0).sum()), D=int(tl.sum()), band_tiles=(b1 - b0) * tiles_x)
    k = round1_length(K, n)
    out["round1"] = k
    if k == 0:
        out.update(rounds=1, partitioned=0, pairs=out["D"], tiles_done=0)
        return out
    part = is_partitioned(camera.near_plane, camera.far_plane, partitioned)
    member = round1_members(proj, tiles, order, camera.near_plane, camera.far_plane, k, part)
    # round 1's lists: the frame's without the others (the row codes stay)
    t1 = tiles.copy()
    t1[~member] = 0
    ranges, (_, stopped) = blend_lists(ob, proj, t1, order, camera, gt, band, stopped=True)
    has_pairs = (ranges[:, 1] > ranges[:, 0]).reshape(tiles_y, tiles_x)
    in_band = np.zeros((tiles_y, tiles_x), bool)
    in_band[b0:b1] = True
    done = tile_all(stopped, W, H) & has_pairs & in_band
    opened = has_pairs & ~done & in_band
    gated = int(done.sum()) == out["band_tiles"]
    # round 2: a visible Gaussian outside round 1 is dropped when its box is at most 3 x 3 tiles and every tile of the
    # WHOLE box is done (a masked rect too); sums over boxes by an integral image of `done`
    rest = np.flatnonzero((tl > 0) & ~member)
    ii = np.zeros((tiles_y + 1, tiles_x + 1), np.int64)
    ii[1:, 1:] = done.cumsum(0).cumsum(1)
    x0, y0, x1, y1 = (proj[f].astype(np.int64) for f in ("tx0", "ty0", "tx1", "ty1"))
    w, h = x1 - x0, y1 - y0
    box_done = ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]
    small = (w >= 1) & (h >= 1) & (w <= 3) & (h <= 3)
    drop = small & (box_done == w * h)
    dropped, survivors = rest[drop[rest]], rest[~drop[rest]]
    d1 = int(tl[member].sum())
    d2 = 0 if gated else int(tl[survivors].sum())
    out.update(rounds=2, partitioned=int(part), member=member, done=done, open=opened, gated=gated, rest=rest,
               dropped=dropped, survivors=survivors, small=small,
               masked=(np.asarray(rows) & 0x8000) != 0 if rows is not None else np.zeros(len(proj), bool),
               D1=d1, pairs_undropped=d1 + int(tl[rest].sum()), pairs=d1 + d2, tiles_done=int(done.sum()))
    return out


def kept_by_whole_box_only(m, proj, tiles):
    """the survivors with a small masked rect every tile of which (of those they touch) is done: only the whole-box rule
    keeps them"""
    rows = getattr(tiles, "rows", None)
    out = []
    for i in m["survivors"]:
        if m["small"][i] and m["masked"][i] and all(m["done"][t] for t in touched_tiles(proj, rows, i)):
            out.append(int(i))
    return out
