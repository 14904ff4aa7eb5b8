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
from records import selection_from_mask

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


def check_merged(got_wide, w, only=None, require_finite=False):
    """got_wide: the (SH f32, cov f32) records of the device, K x 224 bytes; w: merge(...).  Every cell with m >= 2 (and in
    `only`, a bool mask over the cells) is compared value by value against the witness within its bound, colour and opacity
    bytes within 1.  A value whose witness or bound is not finite is left out of the comparison; with require_finite there
    must be none: every value of every picked cell is compared.  Returns the number of cells compared."""
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
            if require_finite:
                assert fin.all(), (name, "left out of the comparison", int((~fin).sum()), np.argwhere(~fin)[:4].tolist())
            err = np.abs(have - want)
            worst = np.where(fin, err - tol, -1.0)
            assert (worst <= 0).all(), (name, float(worst.max()), np.argwhere(worst > 0)[:4].tolist(),
                                        float((err / np.where(tol > 0, tol, 1.0))[fin].max()))
    if require_finite:
        assert np.isfinite(w["rgb"][pick]).all() and np.isfinite(w["alpha"][pick]).all(), "colour or opacity left to the NaN rule"
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


# ---- records from decoded values -------------------------------------------------------------------------------------

def pack_wide(d):
    """decode()'s dict -> (SH f32, cov f32) records, flat bytes: pos | rgba | sh | cov | pad, 224 bytes each.  The inverse of
    decode(0, 1, .): a test sets covariance words (or any other value) in the dict and packs it"""
    n = len(d["pos"])
    rows = np.zeros((n, pod_bytes(0, 1)), np.uint8)
    rows[:, :12] = np.ascontiguousarray(d["pos"], f32).reshape(n, 3).view(np.uint8)
    rows[:, 12:16] = np.asarray(d["rgba"], np.uint8).reshape(n, 4)
    rows[:, 16:196] = np.ascontiguousarray(d["sh"], f32).reshape(n, 45).view(np.uint8)
    rows[:, 196:220] = np.ascontiguousarray(d["cov"], f32).reshape(n, 6).view(np.uint8)
    return rows.reshape(-1)


# ---- constructed runs ------------------------------------------------------------------------------------------------
# The kernels see the Gaussians sorted by cell key, 64 sorted slots per wave, 256 per block, the slots without a point behind
# the points.  line_scene puts a known number of points into each cell of one row of cells, so which run a sorted slot
# belongs to is known by design; wave_partials says from the definition alone what each wave of slots has to hand on.

def line_scene(counts, cell_size, rng, among_tail=0):
    """(pos float32[n, 3], among bool[n] or None): counts[j] points in cell j of one row of cells along x, for which
    cells(pos, cell_size, among)["count"] is exactly `counts`.  h = float32(cell_size) (1 + 2^-10) is the cell side (the
    extent of a few cells is far from the second regime); x = x0 + (j + f) h with f uniform in [0.2, 0.8]: far from a cell
    face against the binary32 rounding of x; y and z within a tenth of a cell; the first member of cell 0 sits exactly on
    the low corner of the box, so the grid starts where the design says.  among_tail more Gaussians, in and around the
    row, are excluded by `among`: they sort behind the points.  The caller order is a random permutation."""
    counts = np.asarray(counts, np.int64)
    assert counts.ndim == 1 and (counts > 0).all()
    P, n = int(counts.sum()), int(counts.sum()) + among_tail
    h = float(f32(cell_size)) * (1.0 + 2.0 ** -10)
    lo = np.array([-0.375, 0.5, 0.25])      # exact in binary32
    j = np.repeat(np.arange(len(counts)), counts).astype(f64)
    pos = np.empty((n, 3), f64)
    pos[:P, 0] = lo[0] + (j + rng.uniform(0.2, 0.8, P)) * h
    pos[:P, 1:] = lo[1:] + rng.uniform(0.0, 0.1, (P, 2)) * h
    pos[0] = lo
    pos[P:, 0] = lo[0] + rng.uniform(-1.0, len(counts) + 1.0, among_tail) * h      # beyond both ends of the row too
    pos[P:, 1:] = lo[1:] + rng.uniform(-0.5, 0.5, (among_tail, 2)) * h
    among = np.arange(n) < P
    perm = rng.permutation(n)
    return pos[perm].astype(f32), (among[perm] if among_tail else None)


W_NONE, W_OPEN, W_MIDDLE, W_LAST = "none", "open", "middle", "last"


def wave_partials(c):
    """From cells(): what every wave of 64 sorted slots hands on, by the definition of a run (not by the kernel's flags).
    dict(incoming[g]: the run that holds the wave's first slot also holds the slot before it — W_MIDDLE if it also holds
    the first slot of the next wave, W_LAST if it ends here, else W_NONE; outgoing[g]: W_OPEN if the run that holds the
    wave's last slot starts in this wave and holds the next wave's first slot, else W_NONE; partials[k]: the waves run k
    touches — a run that crosses a wave edge leaves that many partials).  The slots behind the points hold no run."""
    n, P, K = len(c["pt"]), len(c["order"]), c["K"]
    nwaves = (n + 63) // 64
    first = np.asarray(c["first"], np.int64)
    end = first + np.asarray(c["count"], np.int64)      # one past the run
    run = np.full(64 * (nwaves + 1), -1, np.int64)
    run[:P] = np.repeat(np.arange(K), c["count"])
    incoming, outgoing = [], []
    for g in range(nwaves):
        a, b = 64 * g, 64 * g + 64
        r = run[a]
        came_in = g > 0 and r >= 0 and run[a - 1] == r
        incoming.append(W_NONE if not came_in else W_MIDDLE if run[b] == r else W_LAST)
        r = run[b - 1]
        outgoing.append(W_OPEN if r >= 0 and run[b] == r and first[r] >= a else W_NONE)
    return dict(incoming=incoming, outgoing=outgoing, partials=(end - 1) // 64 - first // 64 + 1)


# The run shapes of the tests: name -> (points per cell, Gaussians excluded by `among`, what the shape is for).  Cell size
# RUN_CELL.  tests/test_simplify_api.py proves what the table covers; tests/test_gpu_simplify_runs.py runs it.
RUN_CELL = 0.25
RUN_SHAPES = {
    "a": ([40, 24, 5, 59], 0, "a run ends in lane 63, the next heads lane 0"),
    "b": ([64, 64, 3], 0, "runs that are exactly one wave"),
    "c": ([63, 2, 63], 0, "a run of two over a wave edge: two partials of one member each"),
    "d": ([255, 2, 30], 0, "a run of two over a block edge"),
    "e": ([63, 1, 1, 10], 0, "singletons in lane 63 and in lane 0"),
    "f": ([64, 192, 5], 0, "open from lane 0, middle waves, last in lane 63"),
    "g": ([10, 200, 7], 0, "open, middle and last, none aligned"),
    "h": ([1, 64 * 63 + 2, 9], 0, "a long run of 64 partials: the last one ends the first chunk of the walk"),
    "i": ([1, 64 * 64 + 2, 9], 0, "a long run of 65 partials: the last one heads the second chunk"),
    "j": ([63, 64 * 64 + 2, 9], 0, "a long run of 66 partials, open in lane 63"),
    "k": ([30, 100, 100, 3], 0, "a wave that closes one crossing run and opens the next"),
    "l": ([5, 187], 0, "the last run ends at slot n - 1, n a multiple of 64"),
    "m": ([6, 250], 0, "the last run ends at slot n - 1, n a multiple of 256"),
    "n": ([5, 187], 70, "non-points fill a whole wave behind the points"),
    "o": ([10, 200, 7], 70, "non-points directly behind a run that ends inside a wave"),
}


def run_shape(name):
    """(pos, among, counts) of a shape of RUN_SHAPES; the same every time"""
    counts, tail, _ = RUN_SHAPES[name]
    pos, among = line_scene(counts, RUN_CELL, np.random.default_rng(1000 + ord(name)), tail)
    return pos, among, np.asarray(counts, np.int64)


# ---- a device call against the witness -------------------------------------------------------------------------------

WIDE = (0, 1)                       # SH f32, cov f32: what the merged values are read from


def witness(sh, cov, pods, cell_size, among=None):
    d = decode(sh, cov, pods)
    c = cells(d["pos"], cell_size, among)
    return d, c, merge(d, c)


def simplify(gs, device, stream, src, pods, cell_size, dst=None, among=None):
    """-> (bytes of the result, the cell plane uint32[n], K)"""
    spod = gs.GaussianPod(*src)
    n = len(pods) // spod.size
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods) if n else gs.GaussiansBuffer.new_empty(device, spod, 0)
    sel = selection_from_mask(gs, device, stream, among)
    out, plane = buf.simplify(stream, cell_size, None if dst is None else gs.GaussianPod(*dst), sel, cell_of_out=True)
    assert out.pod == (spod if dst is None else gs.GaussianPod(*dst))
    got, cell_of, K = out.download(stream), plane.download(stream, np.uint32)[:n].copy(), out.len()
    assert np.array_equal(buf.download(stream), pods), "the source is untouched"
    out.destroy(); plane.release(); buf.destroy()
    if sel is not None:
        sel.destroy()
    return got, cell_of, K


def check_against_witness(gs, device, stream, src, pods, cell_size, among=None, require_finite=False):
    """simplify into (SH f32, cov f32) and compare everything: K and the cell plane exactly, the merged cells within the
    witness's bound (check_merged), the cells of one member bit for bit with the host's conversion; returns (cells, merged
    witness, device bytes)"""
    d, c, w = witness(*src, pods, cell_size, among)
    got, cell_of, K = simplify(gs, device, stream, src, pods, cell_size, WIDE, among)
    assert K == c["K"] and np.array_equal(cell_of, c["cell_of"]), (K, c["K"], int((cell_of != c["cell_of"]).sum()))
    if K:
        check_merged(got, w, require_finite=require_finite)
        one, want = expected_singletons(gs, gs.GaussianPod(*src), gs.GaussianPod(*WIDE), pods, c)
        have = np.asarray(got).reshape(-1, pod_bytes(*WIDE))[one]
        assert np.array_equal(have, want), (len(one), int((have != want).any(axis=1).sum()))
    else:
        assert got.size == 0
    return c, w, got
