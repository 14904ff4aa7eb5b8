"""numpy restatement of DESIGN.md §3.16 (connected components of the neighbour graph), written from the text: the
brute-force adjacency over all pairs of points — the exact binary32 expression of neighbors_np.counts, every operation one
rounded float32 operation in the written order — then min-labels propagated until nothing changes.  No grid, no sort, no
union-find: the components depend on none of them.  Shares no code with the library."""
import numpy as np

import neighbors_np

f32 = np.float32
NONE = 0xFFFFFFFF
UINT32_MAX = 0xFFFFFFFF
CHUNK = 256      # rows of the adjacency built at a time

INFO_FIELDS = ("points", "components", "largest", "largest_label")


def adjacency(pw, radius, among=None):
    """(idx, near): the caller indices of the points and the boolean matrix of the neighbour pairs among them (the
    diagonal is False)"""
    pw = np.asarray(pw, f32)
    idx = np.flatnonzero(neighbors_np.points(pw, among))
    q = pw[idx]
    rr = f32(radius) * f32(radius)
    near = np.zeros((len(idx), len(idx)), bool)
    for a in range(0, len(idx), CHUNK):
        d = q[a:a + CHUNK, None, :] - q[None, :, :]
        near[a:a + CHUNK] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= rr
    np.fill_diagonal(near, False)
    return idx, near


def _edge_list(near):
    """(src, dst) of every directed edge, sorted by src, and the rows that have one"""
    src, dst = np.nonzero(near)
    has = np.zeros(len(near), bool)
    has[src] = True
    starts = np.flatnonzero(np.r_[True, src[1:] != src[:-1]]) if len(src) else np.zeros(0, np.int64)
    return src, dst, has, starts


def components(pw, radius, among=None):
    """(L, S, info): L_i = the smallest caller index of a point in i's component (NONE where i is no point), S_i = the
    number of points in it (0 where i is no point), info = dict of INFO_FIELDS.  L and S are np.uint32."""
    pw = np.asarray(pw, f32)
    n = len(pw)
    idx, near = adjacency(pw, radius, among)
    src, dst, has, starts = _edge_list(near)
    label = idx.astype(np.int64)
    while len(src):
        # every point takes the smallest label among itself and its neighbours, then follows its label's label
        best = label.copy()
        best[has] = np.minimum(label[has], np.minimum.reduceat(label[dst], starts))
        pos = np.searchsorted(idx, best)          # a label is the caller index of a point
        best = np.minimum(best, best[pos])
        if np.array_equal(best, label):
            break
        label = best
    L = np.full(n, NONE, np.uint32)
    S = np.zeros(n, np.uint32)
    L[idx] = label
    if len(idx):
        labels, inverse, count = np.unique(label, return_inverse=True, return_counts=True)
        S[idx] = count[inverse]
        largest = int(count.max())
        info = dict(points=len(idx), components=int((L[idx] == idx).sum()), largest=largest,
                    largest_label=int(labels[count == largest].min()))
    else:
        info = dict(points=0, components=0, largest=0, largest_label=NONE)
    return L, S, info


def info_tuple(info):
    return tuple(int(info[k]) for k in INFO_FIELDS)


def in_size_range(S, min_size, max_size):
    """T = {i : i is a point and min_size <= S_i <= max_size}"""
    S = S.astype(np.int64)
    return (S > 0) & (S >= min_size) & (S <= max_size)


def connected(L, seeds):
    """T = {i : i is a point and its component contains a point j with seeds[j]}"""
    seeds = np.asarray(seeds, bool)
    pt = L != NONE
    hit = np.unique(L[pt & seeds])
    return pt & np.isin(L, hit)
