"""numpy restatement of DESIGN.md §3.18 (k nearest neighbours, their statistics, select and summary), written from the
text: a brute-force search over all pairs of points, every operation one rounded float32 operation in the written order.
No grid, no sort of cells: the row does not depend on either.  Shares no code with the library; the transformed positions
are those of neighbors_np.positions."""
import numpy as np

f32 = np.float32
NONE = 0xFFFFFFFF
KTH_DIST2, MEAN_DIST = 0, 1
CHUNK = 256      # queries per block: 256 x n x 3 float32 at a time


def points(pw, among=None):
    """i is a point iff it belongs to `among` (None: all) and the three components of pw_i are finite"""
    p = np.isfinite(np.asarray(pw, f32)).all(axis=1)
    return p if among is None else p & np.asarray(among, bool)


def rows(pw, k, radius, among=None):
    """(d2, idx): float32[n, k] and uint32[n, k].  Row i = the first min(k, candidates) candidates j != i, points with
    d2(i, j) <= fl(r r), in the order (bits of d2, caller index j); padded with +inf / NONE; all NaN / NONE where i is no
    point."""
    pw = np.asarray(pw, f32)
    n = len(pw)
    pt = points(pw, among)
    idx = np.flatnonzero(pt)
    q = pw[idx]
    rr = f32(radius) * f32(radius)
    d2_out = np.full((n, k), np.nan, f32)
    ix_out = np.full((n, k), NONE, np.uint32)
    for a in range(0, len(idx), CHUNK):
        with np.errstate(over="ignore"):
            d = q[a:a + CHUNK, None, :] - q[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == f32
        for b in range(d2.shape[0]):
            i = idx[a + b]
            cand = d2[b] <= rr
            cand[a + b] = False      # j != i
            j = idx[cand]
            bits = d2[b][cand].view(np.uint32)
            order = np.lexsort((j, bits))[:k]      # the last key is the primary one: d2 bits, then the caller index
            m = len(order)
            d2_out[i] = np.inf
            d2_out[i, :m] = bits[order].view(f32)
            ix_out[i, :m] = j[order]
    return d2_out, ix_out


def row_kinds(d2):
    """(point, complete) of every row of a distance plane: its first value is not NaN; it is a point's and its last value
    is not the padding"""
    d2 = np.asarray(d2, f32)
    point = ~np.isnan(d2[:, 0])
    return point, point & (d2[:, -1].view(np.uint32) != f32(np.inf).view(np.uint32))


def statistic(d2, kind):
    """v of every row (float32[n]): KTH_DIST2 the last value; MEAN_DIST ((sqrt d2_0 + sqrt d2_1) + ...) / (float) k, each
    operation rounded to float32; +inf for an incomplete row, NaN for a row that is no point's"""
    d2 = np.asarray(d2, f32)
    k = d2.shape[1]
    point, complete = row_kinds(d2)
    v = np.full(len(d2), np.nan, f32)
    v[point] = np.inf
    if kind == KTH_DIST2:
        v[complete] = d2[complete, -1]
    else:
        c = d2[complete]
        s = np.sqrt(c[:, 0])
        for t in range(1, k):
            s = s + np.sqrt(c[:, t])
        assert s.dtype == f32
        v[complete] = s / f32(k)
    return v


def in_range(d2, kind, lo, hi):
    """{i : row i is a point's and lo <= v_i <= hi}"""
    v = statistic(d2, kind)
    point, _ = row_kinds(d2)
    with np.errstate(invalid="ignore"):
        return point & (v >= f32(lo)) & (v <= f32(hi))


def summary(d2, kind):
    """points, complete, min, max (float32, by bit order over the complete rows' v; +inf / -inf without one) and the
    binary64 sums of v and v v with the sums of their magnitudes (the scale of the tolerance)"""
    v = statistic(d2, kind)
    point, complete = row_kinds(d2)
    c = v[complete]
    bits = c.view(np.uint32)
    w = c.astype(np.float64)
    return dict(points=int(point.sum()), complete=int(complete.sum()),
                min=bits.min().view(f32) if len(c) else f32(np.inf), max=bits.max().view(f32) if len(c) else f32(-np.inf),
                sum=float(np.sum(w)), sum_sq=float(np.sum(w * w)), abs_sum=float(np.sum(np.abs(w))))
