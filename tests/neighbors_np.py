"""numpy restatement of DESIGN.md §3.11 (neighbour counts, select by neighbourhood), written from the text: a brute-force
count over all pairs of points, every operation one rounded float32 operation in the written order.  No grid, no sort:
the count does not depend on either.  Shares no code with the library; the transformed positions are those of
stats_np.world_positions, the arithmetic tests/test_stats_api.py pins against a plain loop."""
import numpy as np

import stats_np

f32 = np.float32
UINT32_MAX = 0xFFFFFFFF
CHUNK = 256      # queries per block: 256 x n x 3 float32 at a time


def positions(rows, pos=stats_np.IDENTITY["pos"], rot=stats_np.IDENTITY["rot"], scale=stats_np.IDENTITY["scale"]):
    """pw of every record (n rows of bytes, the position is the first 12 bytes of every layout)"""
    rows = np.ascontiguousarray(rows)
    x = rows[:, :12].copy().view(f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return stats_np.world_positions(x, pos, rot, scale)


def points(pw, among=None):
    """i is a point iff it belongs to `among` (None: all) and the three components of pw_i are finite"""
    p = np.isfinite(pw).all(axis=1)
    return p if among is None else p & np.asarray(among, bool)


def counts(pw, radius, among=None):
    """c_i: the points j != i with (d.x d.x + d.y d.y) + d.z d.z <= fl(r r), d = pw_i - pw_j; 0 where i is no point.
    np.int64, uncapped."""
    pw = np.asarray(pw, f32)
    n = len(pw)
    pt = points(pw, among)
    idx = np.flatnonzero(pt)
    q = pw[idx]
    rr = f32(radius) * f32(radius)
    out = np.zeros(n, np.int64)
    for a in range(0, len(idx), CHUNK):
        d = q[a:a + CHUNK, None, :] - q[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = d2 <= rr
        k = np.arange(a, min(a + CHUNK, len(idx)))
        near[k - a, k] = False      # i != j
        out[idx[a:a + CHUNK]] = near.sum(axis=1)
    return out


def capped(c, cap):
    return np.minimum(c, cap).astype(np.uint32)


def in_count_range(c, pt, min_count, max_count):
    """T = {i : i is a point and min_count <= c_i <= max_count}"""
    return pt & (c >= min_count) & (c <= max_count)
