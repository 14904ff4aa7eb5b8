"""float64 witness of DESIGN.md §3.17 (merge the Gaussians of each grid cell), written from the text.  The cells are a numpy
restatement of the grid of §3.11 (bounding box, h, the 21-bit cell per axis, all in binary64 as the kernels compute them):
they are exact, so no case is excluded.  The merged values are evaluated in float64 from the binary32 values of the records
(decoded by convert_np, which shares no code with the library), and every compared value comes with the bound

    (m + 16) 2^-24 sum w_i |t_i| / W        (+ (m + 16) 2^-24 |delta_a delta_b| for a covariance term)

which holds for ANY summation shape of m binary32 terms t_i — the shape is not part of the definition.  t_i is the summed term:
d_i for a position, Sigma_i + d_i d_i^T for a covariance term, the coefficient for SH.  A position gets 2^-24 |p| on top: the
bound above covers delta, but the compared value is p = c + delta rounded to binary32, and in a small cell far from the
origin half an ulp of p (up to 2^-24 |p|) exceeds it — no binary32 result could meet the bound without that term; for the
other values |value| <= sum w_i |t_i| / W, so the 16 already covers their last rounding.  Colour and opacity bytes may differ
from the witness's by 1."""
import numpy as np

import convert_np
from edit_np import pod_bytes

f32, f64 = np.float32, np.float64
CELL_BITS = 21
CELL_MAX = (1 << CELL_BITS) - 1
NOT_A_POINT = 0xFFFFFFFF
COV_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # (a, b) of the six covariance words


# ---- the set ---------------------------------------------------------------------------------------------------------

def unit_cube_gaussians(n, seed=31):
    """decompose_np.set_gaussians-style Gaussians (random rotations, scales log-uniform in [1e-4, 1e2], degenerate kinds)
    with positions uniform in the unit cube"""
    import decompose_np
    g = decompose_np.set_gaussians(n, seed=seed)
    g["pos"] = np.random.default_rng(seed + 1).random((n, 3)).astype(f32)
    return g


# ---- cells -----------------------------------------------------------------------------------------------------------

def points(pos, among=None):
    p = np.isfinite(pos).all(axis=1)
    return p if among is None else p & np.asarray(among, bool)


def grid(pos, pt, cell_size):
    """(lo float64[3], h float64): nb_grid over the points"""
    if pt.any():
        lo, hi = pos[pt].min(axis=0).astype(f64), pos[pt].max(axis=0).astype(f64)
        lo = lo + 0.0      # (-0 as +0, as the identity transform of the kernels leaves it; the value is the same)
        ext = float((hi - lo).max())
    else:
        lo, ext = np.zeros(3), 0.0
    margin = 1.0 + 2.0 ** -10
    h = max(float(f32(cell_size)) * margin, ext * 2.0 ** -21 * margin, 2.0 ** -62)
    return lo, h


def cells(pos, cell_size, among=None):
    """dict(pt bool[n], key uint64[n] (points only meaningful), q int64[n, 3], lo, h, K, cell_of uint32[n], order: the point
    indices in output order (key, then caller index), first[k] / count[k]: the run of cell k in `order`, keys[k])"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    pt = points(pos, among)
    lo, h = grid(pos, pt, cell_size)
    inv_h = 1.0 / h
    with np.errstate(all="ignore"):
        u = (pos.astype(f64) - lo) * inv_h
        q = np.where(u >= float(CELL_MAX), CELL_MAX, np.where(u > 0.0, np.trunc(u), 0.0))
    q = np.where(pt[:, None], q, 0).astype(np.int64)
    key = (q[:, 2].astype(np.uint64) << np.uint64(2 * CELL_BITS)) | (q[:, 1].astype(np.uint64) << np.uint64(CELL_BITS)) | q[:, 0].astype(np.uint64)
    idx = np.flatnonzero(pt)
    order = idx[np.argsort(key[idx], kind="stable")]
    ks = key[order]
    head = np.ones(len(order), bool)
    head[1:] = ks[1:] != ks[:-1]
    first = np.flatnonzero(head)
    K = len(first)
    count = np.diff(np.append(first, len(order)))
    cell_of = np.full(n, NOT_A_POINT, np.uint32)
    cell_of[order] = (np.cumsum(head) - 1).astype(np.uint32)
    return dict(pt=pt, key=key, q=q, lo=lo, h=h, K=K, cell_of=cell_of, order=order, first=first, count=count, keys=ks[first])


def centres(c):
    """float32[K, 3]: lo + (cell + 0.5) h per axis, rounded to binary32"""
    q = c["q"][c["order"][c["first"]]]
    return (c["lo"] + (q.astype(f64) + 0.5) * c["h"]).astype(f32)


# ---- decoding --------------------------------------------------------------------------------------------------------

def decode(sh, cov, pods):
    """the binary32 values of packed records: dict(pos [n, 3], rgba [n, 4] bytes, sh [n, 45], cov [n, 6])"""
    wide = convert_np.convert(sh, cov, 0, 1, pods).reshape(-1, pod_bytes(0, 1))
    return dict(pos=np.ascontiguousarray(wide[:, :12]).view(f32), rgba=wide[:, 12:16].copy(),
                sh=np.ascontiguousarray(wide[:, 16:196]).view(f32), cov=np.ascontiguousarray(wide[:, 196:220]).view(f32))


# ---- the merge -------------------------------------------------------------------------------------------------------

def _seg(x, first):
    return np.add.reduceat(x, first, axis=0)


def merge(d, c):
    """The merged cells of the decoded records d over the cells c, float64: dict(m int[K], unit bool[K], pos [K, 3],
    cov [K, 6], sh [K, 45], rgb [K, 3], alpha [K] (before the byte), and *_tol: the bound of every compared value).  Cells
    with m == 1 are in the arrays too (the merge of one Gaussian); the tests compare those bit for bit with the conversion."""
    o, first, m = c["order"], c["first"], c["count"]
    K = c["K"]
    if K == 0:
        return dict(m=m, K=0)
    rep = np.repeat(np.arange(K), m)
    with np.errstate(all="ignore"):
        pos, cov, sh = d["pos"][o].astype(f64), d["cov"][o].astype(f64), d["sh"][o].astype(f64)
        rgb, alpha = d["rgba"][o, :3].astype(f64) / 255.0, d["rgba"][o, 3].astype(f64) / 255.0
        size = (cov[:, 0] + cov[:, 3]) + cov[:, 5]
        w = alpha * size
        W = _seg(w, first)
        # binary32 decides: a weight that overflows binary32 is not finite there
        bad = ~np.isfinite((alpha.astype(f32) * ((d["cov"][o, 0] + d["cov"][o, 3]) + d["cov"][o, 5])).astype(f32))
        unit = ~(W > 0) | (_seg(bad.astype(np.int64), first) > 0)
        w = np.where(unit[rep], 1.0, w)
        W = _seg(w, first)
        cen = centres(c).astype(f64)
        dd = pos - cen[rep]
        eps = ((m + 16) * 2.0 ** -24)[:, None]

        def mean(t):
            t = t.reshape(len(t), -1)
            return _seg(w[:, None] * t, first) / W[:, None], eps * _seg(w[:, None] * np.abs(t), first) / W[:, None]
        delta, p_tol = mean(dd)
        p = cen + delta
        p_tol = p_tol + 2.0 ** -24 * np.abs(p)      # the rounding of c + delta to binary32: see the head of the file
        S, S_tol = mean(np.stack([cov[:, k] + dd[:, a] * dd[:, b] for k, (a, b) in enumerate(COV_PAIRS)], axis=1))
        for k, (a, b) in enumerate(COV_PAIRS):
            S[:, k] -= delta[:, a] * delta[:, b]
            S_tol[:, k] += eps[:, 0] * np.abs(delta[:, a] * delta[:, b])
        for k in (0, 3, 5):
            S[:, k] = np.where(S[:, k] < 0, 0.0, S[:, k])
        shm, sh_tol = mean(sh)
        col, _ = mean(rgb)
        trace = (S[:, 0] + S[:, 3]) + S[:, 5]
        a_w = np.where(trace > 0, W / np.where(trace > 0, trace, 1.0), 0.0)
        a_u = _seg(alpha, first) / m
        a = np.clip(np.where(unit, a_u, a_w), 0.0, 1.0)
        a = np.where(np.isnan(a), 0.0, a)
    return dict(m=m, K=K, unit=unit, pos=p, pos_tol=p_tol, cov=S, cov_tol=S_tol, sh=shm, sh_tol=sh_tol, rgb=col, alpha=a)


def color_bytes(x):
    """trunc(255 x + 0.5), saturated, NaN -> 0"""
    with np.errstate(all="ignore"):
        v = 255.0 * np.asarray(x, f64) + 0.5
        return np.where(v > 0, np.minimum(np.floor(v), 255.0), 0.0).astype(np.int64)


def check_merged(got_wide, w, only=None):
    """got_wide: the (SH f32, cov f32) records of the device, K x 224 bytes; w: merge(...).  Every cell with m >= 2 (and in
    `only`, a bool mask over the cells) is compared value by value against the witness within its bound, colour and opacity
    bytes within 1.  Returns the number of cells compared."""
    rows = np.asarray(got_wide, np.uint8).reshape(-1, pod_bytes(0, 1))
    assert len(rows) == w["K"], (len(rows), w["K"])
    pick = w["m"] >= 2
    if only is not None:
        pick &= only
    g = dict(pos=np.ascontiguousarray(rows[:, :12]).view(f32).astype(f64), rgba=rows[:, 12:16].astype(np.int64),
             sh=np.ascontiguousarray(rows[:, 16:196]).view(f32).astype(f64), cov=np.ascontiguousarray(rows[:, 196:220]).view(f32).astype(f64))
    with np.errstate(all="ignore"):
        for name in ("pos", "cov", "sh"):
            want, tol, have = w[name][pick], w[name + "_tol"][pick], g[name][pick]
            fin = np.isfinite(want) & np.isfinite(tol)
            err = np.abs(have - want)
            worst = np.where(fin, err - tol, -1.0)
            assert (worst <= 0).all(), (name, float(worst.max()), np.argwhere(worst > 0)[:4].tolist(),
                                        float((err / np.where(tol > 0, tol, 1.0))[fin].max()))
    assert (np.abs(g["rgba"][pick, :3] - color_bytes(w["rgb"][pick])) <= 1).all(), "colour bytes"
    assert (np.abs(g["rgba"][pick, 3] - color_bytes(w["alpha"][pick])) <= 1).all(), "opacity bytes"
    return int(pick.sum())


def expected_singletons(gs, spod, dpod, pods, c):
    """(cell indices with one member, their expected records [k, dpod.size]): the source rows converted by the HOST functions
    (gs_convert_pods; gs_decompose_pods for a covariance source and a rotation + scale destination)"""
    one = np.flatnonzero(c["count"] == 1)
    src = np.ascontiguousarray(np.asarray(pods, np.uint8).reshape(-1, spod.size)[c["order"][c["first"][one]]]).reshape(-1)
    if dpod.cov == 0 and spod.cov != 0:
        out = spod.decompose(src, dpod.sh)
    else:
        out = spod.convert(src, dpod)
    return one, np.asarray(out, np.uint8).reshape(-1, dpod.size)
