"""The exact expectation of the contribution records (gs_contribution), from the frozen oracle.

The oracle's blend with background 0 and every projected colour 0 except r = 1 for Gaussian i0, g = 1 for i1 and b = 1 for i2
returns, in its three colour channels, exactly the weight planes of those three Gaussians: a Gaussian meets a pixel at most
once, fma(1, w, 0) = w, fma(0, w, C) = C, and the background term is T * 0.  From a plane W_i:
hits = count_nonzero, wmax = max, sum = sum of (uint64)(W_i * 2^24) with the product exact in float64."""
import hashlib

import numpy as np

import synth

CONTRIBUTION_DTYPE = np.dtype([("sum", "<u8"), ("hits", "<u4"), ("wmax", "<f4")])
assert CONTRIBUTION_DTYPE.itemsize == 16

_cache = {}


def zero_records(n):
    return np.zeros(n, dtype=CONTRIBUTION_DTYPE)


def combine(a, b):
    """a (+) b: add, add (mod 2^32), max"""
    out = zero_records(len(a))
    out["sum"] = a["sum"] + b["sum"]
    out["hits"] = a["hits"] + b["hits"]      # uint32: wraps
    out["wmax"] = np.maximum(a["wmax"], b["wmax"])
    return out


def raw(records):
    """the records as rows of 16 bytes: what "bit for bit" compares"""
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1, 16)


def sorted_frame(ob, sh, cov, pods, ogt, omt, ocam, order, band=None, hidden=None):
    """the oracle's frame up to the tile ranges; hidden: indices whose tile counts are zeroed before build_keys"""
    proj, tiles = ob.preprocess(sh, cov, pods, ogt, omt, ocam, band=band)
    if hidden is not None:
        tiles[hidden] = 0
    tiles_x, tiles_y = (ocam.width + 15) // 16, (ocam.height + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    return proj, tiles, skeys, sidx, ranges


def expectation(ob, proj, tiles, skeys, sidx, ranges, ocam, ogt, band=None):
    """n records: the contributions of one frame (band: its tile rows).  Cached on everything the weights depend on: two
    layouts with the same geometry and opacity share one computation."""
    n = len(proj)
    tiles_x = (ocam.width + 15) // 16
    geom = np.ascontiguousarray(proj).copy()
    for name in ("r", "g", "b"):
        geom[name] = 0.0
    key = hashlib.sha256(geom.tobytes() + np.ascontiguousarray(sidx).tobytes() + np.ascontiguousarray(ranges).tobytes() +
                         bytes(ocam) + bytes(ogt) + repr(band).encode()).hexdigest()
    if key in _cache:
        return _cache[key].copy()
    cam0 = ob.Camera.from_buffer_copy(bytes(ocam))
    cam0.background[:] = [0.0, 0.0, 0.0]
    out = zero_records(n)
    # the tile rows every Gaussian has pairs in: a blend call covers only the rows of its three Gaussians
    trow = ((skeys >> np.uint64(32)).astype(np.int64) // tiles_x) if len(skeys) else np.zeros(0, np.int64)
    lo = np.full(n, 1 << 30, np.int64)
    hi = np.full(n, -1, np.int64)
    np.minimum.at(lo, sidx, trow)
    np.maximum.at(hi, sidx, trow)
    vis = np.flatnonzero(hi >= 0)
    vis = vis[np.argsort(lo[vis], kind="stable")]
    for k in range(0, len(vis), 3):
        trio = vis[k:k + 3]
        p = geom.copy()
        for name, i in zip(("r", "g", "b"), trio):
            p[name][i] = 1.0
        rows = (int(lo[trio].min()), int(hi[trio].max()) + 1)
        if band is not None:
            rows = (max(rows[0], band[0]), min(rows[1], band[1]))
        planes = ob.blend(p, sidx, ranges, cam0, band=rows, gt=ogt)
        for c, i in enumerate(trio):
            w = planes[..., c]
            assert (w >= 0.0).all()
            out["hits"][i] = np.count_nonzero(w)
            out["wmax"][i] = w.max()
            out["sum"][i] = (w.astype(np.float64) * 16777216.0).astype(np.uint64).sum(dtype=np.uint64)
    _cache[key] = out
    return out.copy()


def scene_a():
    """2500 large opaque splats at 90 x 58: lists of more than one staging batch, thousands of pixels stopped at T < 1e-4,
    visible Gaussians that no pixel blends, partial tiles on both edges"""
    g = synth.scene(2500, first=4242)
    g["color"][:, 3] = 255
    g["scale"] *= np.float32(12)
    return g


SCENE_A_SIZE = (90, 58)


def assert_scene_a_conditions(ob, tiles, skeys, sidx, ranges, ocam, ogt, proj, order, exp):
    """what makes scene A a test of the accumulation: asserted on the oracle's output before anything is compared"""
    W, H = ocam.width, ocam.height
    assert int((ranges[:, 1] - ranges[:, 0]).max()) > 256, "no tile list of more than one staging batch"
    _, stopped = ob.blend(proj, sidx, ranges, ocam, gt=ogt, stopped=True)
    assert int(stopped.sum()) >= 1000, "too few pixels stop at T < 1e-4"
    visible = np.asarray(tiles) > 0
    assert (visible & (exp["hits"] == 0)).any(), "every visible Gaussian is blended somewhere"
    assert not np.array_equal(order, np.arange(len(order))), "the spatial order is the identity"
    assert W % 16 and H % 16, "no partial tile column / row"
    assert (exp["hits"][~visible] == 0).all()
