"""numpy restatement of DESIGN.md §3.19 (nearest neighbours between two buffers, the sums over their pairs, the rigid fit
and the composition of two transforms), written from the text.  rows_between is a brute-force search over all (query,
target point) pairs, every operation one rounded float32 operation in the written order: no grid, no sort of cells.
pair_sums is binary64 with math.fsum for the reference value.  rigid_fit is independent of the library's Jacobi: the
largest eigenvector of Horn's matrix by numpy.linalg.eigh, and the SVD form beside it.  Shares no code with the library;
the transformed positions are those of neighbors_np.positions."""
import math

import numpy as np

f32 = np.float32
NONE = 0xFFFFFFFF
CHUNK = 256      # queries per block: 256 x n_t x 3 float32 at a time


def rows_between(pq, pt, k, radius, queries=None, among=None):
    """(d2, idx, written): float32[n_q, k], uint32[n_q, k] and the bool mask of the rows the call writes (`queries`; None:
    all).  Row i of a query whose pq_i is finite = the first min(k, candidates) target points j (in `among`, pt_j finite)
    with d2(i, j) <= fl(r r), in the order (bits of d2, target index j), padded with +inf / NONE; all NaN / NONE where pq_i
    is not finite.  A row outside `queries` is not defined by the call — it keeps its bytes — and comes back NaN / NONE."""
    pq, pt = np.asarray(pq, f32).reshape(-1, 3), np.asarray(pt, f32).reshape(-1, 3)
    nq = len(pq)
    written = np.ones(nq, bool) if queries is None else np.asarray(queries, bool)
    tpoint = np.isfinite(pt).all(axis=1)
    if among is not None:
        tpoint = tpoint & np.asarray(among, bool)
    tidx = np.flatnonzero(tpoint)
    t = pt[tidx]
    qidx = np.flatnonzero(np.isfinite(pq).all(axis=1) & written)
    q = pq[qidx]
    rr = f32(radius) * f32(radius)
    d2_out = np.full((nq, k), np.nan, f32)
    ix_out = np.full((nq, k), NONE, np.uint32)
    for a in range(0, len(qidx), CHUNK):
        with np.errstate(over="ignore"):
            d = q[a:a + CHUNK, None, :] - t[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == f32
        for b in range(d2.shape[0]):
            i = qidx[a + b]
            cand = d2[b] <= rr
            j = tidx[cand]
            bits = d2[b][cand].view(np.uint32)
            order = np.lexsort((j, bits))[:k]      # the last key is the primary one: d2 bits, then the target index
            m = len(order)
            d2_out[i] = np.inf
            d2_out[i, :m] = bits[order].view(f32)
            ix_out[i, :m] = j[order]
    return d2_out, ix_out, written


def pair_terms(pq, pt, first_index, queries=None):
    """(mask of the queries that form a pair, the 18 per-pair values in the order of gs_pair_sums behind its count): pair i
    iff i is in `queries`, j = first_index[i] < n_t and pq_i, pt_j are finite; binary64 from the float32 positions"""
    pq, pt = np.asarray(pq, f32).reshape(-1, 3), np.asarray(pt, f32).reshape(-1, 3)
    j = np.asarray(first_index, np.uint32).astype(np.int64)
    ok = j < len(pt)
    if queries is not None:
        ok &= np.asarray(queries, bool)
    ok &= np.isfinite(pq).all(axis=1)
    ok[ok] = np.isfinite(pt[j[ok]]).all(axis=1)
    p, q = pq[ok].astype(np.float64), pt[j[ok]].astype(np.float64)
    d = p - q
    terms = np.concatenate([p, q, (p[:, :, None] * q[:, None, :]).reshape(-1, 9),
                            ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])[:, None],
                            ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])[:, None],
                            ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]], axis=1)
    return ok, terms


def pair_sums(pq, pt, first_index, queries=None):
    """dict(pairs, sums: the 18 values by math.fsum — correctly rounded —, abs: the sums of their magnitudes, the scale of
    the tolerance)"""
    ok, terms = pair_terms(pq, pt, first_index, queries)
    return dict(pairs=int(ok.sum()), sums=np.array([math.fsum(terms[:, f]) for f in range(18)]),
                abs=np.array([math.fsum(np.abs(terms[:, f])) for f in range(18)]))


def horn_matrix(pairs, sums):
    """(N, H, mean p, mean q, spread of p) from the count and the 18 sums"""
    sums = np.asarray(sums, np.float64)
    sp, sq, spq, spp = sums[0:3], sums[3:6], sums[6:15].reshape(3, 3), sums[15]
    n = float(pairs)
    H = spq - np.outer(sp, sq) / n
    N = np.array([[H[0, 0] + H[1, 1] + H[2, 2], H[1, 2] - H[2, 1], H[2, 0] - H[0, 2], H[0, 1] - H[1, 0]],
                  [H[1, 2] - H[2, 1], H[0, 0] - H[1, 1] - H[2, 2], H[0, 1] + H[1, 0], H[2, 0] + H[0, 2]],
                  [H[2, 0] - H[0, 2], H[0, 1] + H[1, 0], H[1, 1] - H[0, 0] - H[2, 2], H[1, 2] + H[2, 1]],
                  [H[0, 1] - H[1, 0], H[2, 0] + H[0, 2], H[1, 2] + H[2, 1], H[2, 2] - H[0, 0] - H[1, 1]]])
    return N, H, sp / n, sq / n, spp - float(sp @ sp) / n


def quat_matrix(q):
    """the rotation matrix of the unit quaternion (w, x, y, z)"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rigid_fit(pairs, sums, with_scale=False):
    """dict(quat (w, x, y, z; w >= 0), scale, t, R, rms, eig: the eigenvalues of N ascending, fro: its Frobenius norm)"""
    N, H, pm, qm, spread = horn_matrix(pairs, sums)
    vals, vecs = np.linalg.eigh(N)
    q = vecs[:, -1]
    q = q / np.linalg.norm(q)
    first = q[np.flatnonzero(q)[0]]
    if first < 0:
        q = -q
    R = quat_matrix(q)
    s = float(np.sum(R * H.T) / spread) if with_scale else 1.0
    return dict(quat=q, scale=s, t=qm - s * (R @ pm), R=R, rms=math.sqrt(np.asarray(sums)[17] / pairs), eig=vals,
                fro=float(np.linalg.norm(N)))


def rigid_fit_svd(p, q):
    """the rotation of the classic SVD solution (Arun / Kabsch) from the pairs themselves: R with q ~ R p + t"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    pc, qc = p - p.mean(axis=0), q - q.mean(axis=0)
    U, _, Vt = np.linalg.svd(pc.T @ qc)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    return Vt.T @ D @ U.T


def pod_matrix(pos, rot, scale):
    """the 4 x 4 matrix of a pos / rot (x, y, z, w) / scale pod in binary64: R diag(scale), then the translation"""
    x, y, z, w = [float(v) for v in rot]
    M = np.eye(4)
    M[:3, :3] = quat_matrix((w, x, y, z)) @ np.diag([float(v) for v in scale])
    M[:3, 3] = [float(v) for v in pos]
    return M


def compose(delta, m):
    """(pos, rot xyzw, scale) of delta o m in binary64, delta of uniform scale delta[2][0]"""
    (dp, dr, ds), (mp, mr, ms) = delta, m
    dw, dx, dy, dz = float(dr[3]), float(dr[0]), float(dr[1]), float(dr[2])
    mw, mx, my, mz = float(mr[3]), float(mr[0]), float(mr[1]), float(mr[2])
    w = dw * mw - dx * mx - dy * my - dz * mz
    x = dw * mx + dx * mw + dy * mz - dz * my
    y = dw * my - dx * mz + dy * mw + dz * mx
    z = dw * mz + dx * my - dy * mx + dz * mw
    s = float(ds[0])
    pos = s * (quat_matrix((dw, dx, dy, dz)) @ np.asarray(mp, np.float64)) + np.asarray(dp, np.float64)
    return pos, np.array([x, y, z, w]), s * np.asarray(ms, np.float64)


def icp_case(side=9, jitter=0.1, part=0.4, degrees=2.0, shift=(0.03, -0.02, 0.04), seed=19):
    """The ICP input of the tests: dict(target float32[side^3, 3]: a unit lattice jittered by +-jitter per axis; query
    float32[n_q, 3]: `part` of the target moved so that R (q - c) + c + shift is its mate, R = `degrees` about an oblique
    axis through the centroid c; mate int64[n_q]; R; t: the translation of x -> R x + t)"""
    rng = np.random.default_rng(seed)
    k = np.arange(side, dtype=np.float64)
    target = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-jitter, jitter, (side ** 3, 3))
    target = target.astype(f32)
    mate = np.sort(rng.permutation(len(target))[:int(part * len(target))])
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    half = math.radians(degrees) / 2
    R = quat_matrix(np.r_[math.cos(half), math.sin(half) * axis])
    c = target.astype(np.float64).mean(axis=0)
    query = ((target[mate].astype(np.float64) - c - np.asarray(shift)) @ R + c).astype(f32)      # R^T (.) as a row product
    return dict(target=target, query=query, mate=mate, R=R, t=c + np.asarray(shift) - R @ c)
