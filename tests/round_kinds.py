"""The frame kinds of the round-bound sequences (tests/test_gpu_round_bounds.py) and the oracle's side of them, computed once
per process and without a GPU: the frame of a kind in stages, the Gaussians of its round 1 and the pairs of each round."""
import numpy as np

import helpers
import rounds_np

N, W, H, BAND = 60000, 640, 360, (5, 14)          # the one shape of every sequence: 40 x 23 tiles, a band of 360
TILES_X, TILES_Y = (W + 15) // 16, (H + 15) // 16
BAND_TILES = (BAND[1] - BAND[0]) * TILES_X
SH_NONE, ROT_SCALE = 3, 0                          # gs.SH_NONE / gs.COV3D_ROT_SCALE
NEAR, FAR = 0.1, 100.0                             # helpers.default_camera's planes: 27 depth-key bits

# T: translucent (opacity byte 5); A: opaque splats eight times the size, which cover the view
BUFFERS = {"T": dict(first=4242, opacity=5, scale=4.0), "A": dict(first=31, opacity=255, scale=8.0)}
# kind: (buffer, size of the Gaussian transform).  The oracle's figures in the band (V visible, D pairs; D1 + D2 with the
# nearest 2 048 / 16 384 in round 1, unpartitioned): small 23 501, 55 345 (10 613 + 44 732 / 42 774 + 12 571); big 28 468,
# 309 085 (76 478 + 232 607 / 237 078 + 72 007); cover 27 773, 258 918 (round 1 of 2 048: 63 555 pairs, finishes all 360 tiles)
KINDS = {"small": ("T", 1.0), "big": ("T", 4.0), "cover": ("A", 1.0)}
_host_cache, _kind_cache, _members_cache, _round1_cache = {}, {}, {}, {}


def host_buffer(ob, b):
    if b not in _host_cache:
        g = helpers.deep_scene(N, **BUFFERS[b])
        pods = ob.pack(SH_NONE, ROT_SCALE, g)
        _host_cache[b] = dict(g=g, pods=pods, order=ob.spatial_order(SH_NONE, ROT_SCALE, pods))
    return _host_cache[b]


def kind_transforms(ob, kind):
    ogt = ob.gaussian_transform(size=KINDS[kind][1], sh_deg=0)
    ocam = helpers.default_camera(ob, W, H, near=NEAR, far=FAR)
    ocam.background[:] = [0.0, 0.0, 0.0]
    return ogt, ob.model_transform(), ocam


def _oracle_blend(ob, o, tiles):
    keys, idx = ob.build_keys(o["proj"], tiles, TILES_X, order=o["order"])
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, TILES_X * TILES_Y)
    return sidx, ranges, ob.blend(o["proj"], sidx, ranges, o["ocam"], band=BAND, gt=o["ogt"])


def oracle_kind(ob, kind):
    """the oracle's frame of a kind, in stages (as tests/test_gpu_renderer_walk.py builds its frames), once per module"""
    if kind not in _kind_cache:
        hb = host_buffer(ob, KINDS[kind][0])
        ogt, omt, ocam = kind_transforms(ob, kind)
        proj, tiles = ob.preprocess(SH_NONE, ROT_SCALE, hb["pods"], ogt, omt, ocam, band=BAND)
        o = dict(proj=proj, tiles=tiles, order=hb["order"], ogt=ogt, omt=omt, ocam=ocam)
        o["idx"], o["ranges"], o["rgba"] = _oracle_blend(ob, o, tiles)
        tl = np.asarray(tiles)
        o["V"], o["D"] = int((tl > 0).sum()), int(tl.astype(np.uint64).sum())
        _kind_cache[kind] = o
    return _kind_cache[kind]


def round1_members(ob, kind, K, partitioned):
    """mask of the Gaussians round 1 renders (tests/rounds_np.py's round1_members, at this file's planes): the nearest K
    visible ones of an unpartitioned frame, everything in front of the cut of a partitioned one"""
    key = (kind, K, bool(partitioned))
    if key not in _members_cache:
        o = oracle_kind(ob, kind)
        _members_cache[key] = rounds_np.round1_members(o["proj"], o["tiles"], o["order"], NEAR, FAR, K, partitioned)
    return _members_cache[key]


def round_counts(ob, kind, K, partitioned):
    """(D1, D - D1): the tile counts of round 1's Gaussians and of the others"""
    o = oracle_kind(ob, kind)
    d1 = int(np.asarray(o["tiles"])[round1_members(ob, kind, K, partitioned)].astype(np.uint64).sum())
    return d1, o["D"] - d1


def round1_frame(ob, kind, K, partitioned):
    """the oracle's frame of round 1's Gaussians alone, in their relative order, on background 0"""
    key = (kind, K, bool(partitioned))
    if key not in _round1_cache:
        o = oracle_kind(ob, kind)
        tiles = o["tiles"].copy()              # (keeps the tile row codes of rect version 4)
        tiles[~round1_members(ob, kind, K, partitioned)] = 0
        _round1_cache[key] = _oracle_blend(ob, o, tiles)[2]
    return _round1_cache[key]
