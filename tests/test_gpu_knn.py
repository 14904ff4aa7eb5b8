"""k nearest neighbours, select by them and their summary on the device against the brute-force numpy
restatement of tests/knn_np.py: rows, indices, statistics, min / max, counts and selection words bit for bit; the two
binary64 sums inside complete 2^-52 sum |v| (sum v v), the bound of tests/test_gpu_stats.py.  The row is defined without a
grid, so the restatement has none; the lattice, the duplicates and the far outlier are the inputs a grid gets wrong."""
import ctypes as C

import numpy as np
import pytest

import knn_np
import neighbors_np
import stats_np
from records import SELECT_OPS, buffer_rows, edited_pods, np_op, sample_edit, selection_from_mask
from scenes import FOUR_LAYOUTS, N, pod_rows

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
INF = float("inf")
KS = (1, 3, 8, 16)
# rotation + translation + non-uniform scale
Q = np.array([0.3, -0.5, 0.2, 0.7])
MT = dict(pos=(0.5, -0.25, 1.5), rot=tuple((Q / np.linalg.norm(Q)).astype(f32)), scale=(1.25, 0.75, 2.0))

_REF = {}


def _kth_distance(pw, k):
    """median over the points of the distance to the k-th nearest other point (binary64; only used to PICK radii, as
    tests/test_gpu_neighbors.py picks them)"""
    q = pw[np.isfinite(pw).all(axis=1)].astype(np.float64)
    out = []
    for a in range(0, len(q), 512):
        d2 = ((q[a:a + 512, None, :] - q[None, :, :]) ** 2).sum(axis=2)
        out.append(np.sqrt(np.partition(d2, k, axis=1)[:, k]))        # column 0 is the point itself
    return float(np.median(np.concatenate(out)))


def _scene_ref(gs):
    """pw of the N-scene under MT, three radii (median count 0, about 8, more than half of n) and the restatement's rows of
    16 for each (the row of k is its first k entries: tests/test_knn_api.py); computed once, never written to"""
    if not _REF:
        pw = neighbors_np.positions(pod_rows(gs, 3, 0), **MT)
        radii = [0.5 * _kth_distance(pw, 1), _kth_distance(pw, 8), _kth_distance(pw, (6 * N) // 10)]
        rows = [knn_np.rows(pw, 16, r) for r in radii]
        counts = [neighbors_np.counts(pw, r) for r in radii]
        med = [float(np.median(c[neighbors_np.points(pw)])) for c in counts]
        assert med[0] == 0 and 4 <= med[1] <= 16 and med[2] > N / 2, med
        for k in (8, 16):      # incomplete and complete rows both occur at the middle radius
            pt, complete = knn_np.row_kinds(rows[1][0][:, :k])
            assert complete.any() and (pt & ~complete).any(), k
        for a in [pw] + [x for pair in rows for x in pair]:
            a.setflags(write=False)
        _REF.update(pw=pw, radii=radii, rows=rows)
    return _REF


def _knn(buf, stream, k, r, among=None, queries=None, mt=None):
    """(d2 float32[n, k], index uint32[n, k]) of one knn call into new planes"""
    d, ix = buf.knn(stream, k, r, among=among, queries=queries, model_transform=mt, indices=True)
    n = buf.len()
    got = (np.asarray(d.download(stream, f32))[:n * k].reshape(n, k).copy(), np.asarray(ix.download(stream, u32))[:n * k].reshape(n, k).copy())
    d.release(); ix.release()
    return got


def _same(got, want, what=""):
    assert got[0].dtype == f32 and got[1].dtype == u32
    assert np.array_equal(got[0].view(u32), want[0].view(u32)), ("d2", what)
    assert np.array_equal(got[1], want[1]), ("index", what)


def _buffer_at(gs, device, positions):
    """a (no SH, rot + scale) buffer with the given positions"""
    import synth
    g = synth.scene(len(positions), first=3)
    g["pos"] = np.asarray(positions, f32)
    pod = gs.GaussianPod(3, 0)
    rows = np.asarray(pod.from_gaussian(g)).reshape(len(positions), pod.size)
    return gs.GaussiansBuffer.new_with_pods(device, pod, rows), rows


def _check_positions(gs, device, stream, p, radii, ks, what):
    buf, _ = _buffer_at(gs, device, p)
    for r in radii:
        for k in ks:
            _same(_knn(buf, stream, k, r), knn_np.rows(p, k, r), (what, r, k))
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 1. four layouts, three radii, four values of k, under a transform
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_rows_equal_the_restatement(gs, device, stream, sh, cov):
    ref = _scene_ref(gs)
    rows = pod_rows(gs, sh, cov)
    assert np.array_equal(neighbors_np.positions(rows, **MT).view(u32), ref["pw"].view(u32))
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    mt = gs.model_transform_pod(**MT)
    for r, (wd, wi) in zip(ref["radii"], ref["rows"]):
        for k in KS:
            got = _knn(buf, stream, k, r, mt=mt)
            _same(got, (wd[:, :k], wi[:, :k]), (r, k))
            assert np.isnan(got[0][5:8]).all() and (got[1][5:8] == knn_np.NONE).all()      # the planted NaN / inf rows
    # without the index plane: the same distances
    d = buf.knn(stream, 8, ref["radii"][1], model_transform=mt)
    assert isinstance(d, gs.Buffer)
    assert np.array_equal(np.asarray(d.download(stream, u32))[:8 * N], ref["rows"][1][0][:, :8].reshape(-1).view(u32))
    d.release()
    assert np.array_equal(buffer_rows(buf, stream), rows)
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 2. small buffers
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1025])
def test_small_buffers(gs, device, stream, n):
    sh, cov = 1, 2
    pod = gs.GaussianPod(sh, cov)
    rows = pod_rows(gs, sh, cov, n) if n else np.zeros((0, pod.size), np.uint8)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, rows)
    pw = neighbors_np.positions(rows) if n else np.zeros((0, 3), f32)
    r = 2.0 * _kth_distance(pw, 1) if n > 12 else 1.0
    for k in (3, 16):
        want = knn_np.rows(pw, k, r)
        _same(_knn(buf, stream, k, r), want, (n, k))
        if n > 12:
            pt, complete = knn_np.row_kinds(want[0])
            assert (pt & ~complete).any() and (complete.any() or k == 16)
    # k = 16 > n - 1 at a radius that holds everything: every point's row is incomplete
    if 0 < n <= 16:
        want = knn_np.rows(pw, 16, 1e3)
        assert not knn_np.row_kinds(want[0])[1].any()
        _same(_knn(buf, stream, 16, 1e3), want, n)
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 3. a lattice: every neighbour sits on a cell boundary and most distances tie
# ------------------------------------------------------------------------------------------------

def _lattice():
    k = np.arange(9, dtype=f32) * f32(0.25)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("shuffled", [False, True])
def test_lattice_ties_go_to_the_smaller_index(gs, device, stream, shuffled):
    p = _lattice()
    if shuffled:      # sorted order != caller order
        p = p[np.random.default_rng(8).permutation(len(p))]
    interior = ((p > 0) & (p < 2)).all(axis=1)
    buf, _ = _buffer_at(gs, device, p)
    for r in (0.25, 0.5):
        for k in (6, 7):
            want = knn_np.rows(p, k, r)
            got = _knn(buf, stream, k, r)
            _same(got, want, (r, k))
            # six neighbours at the spacing, in ascending caller index; the seventh only inside the larger radius
            d, ix = got[0][interior], got[1][interior]
            assert (d[:, :6] == f32(0.0625)).all() and (np.diff(ix[:, :6].astype(np.int64), axis=1) > 0).all()
            if k == 7:
                assert (d[:, 6] == (f32(0.125) if r == 0.5 else f32(INF))).all()
                assert ((ix[:, 6] == knn_np.NONE) == (r == 0.25)).all()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 4. duplicates: r = 0, every distance +0, the indices are the k smallest other copies
# ------------------------------------------------------------------------------------------------

def test_duplicates(gs, device, stream):
    rng = np.random.default_rng(12)
    p = rng.uniform(-2, 2, (130, 3)).astype(f32)
    copies = np.sort(rng.permutation(130)[:100])
    p[copies] = f32([0.3, -1.7, 2.9])
    buf, _ = _buffer_at(gs, device, p)
    for k in (3, 16):
        want = knn_np.rows(p, k, 0.0)
        got = _knn(buf, stream, k, 0.0)
        _same(got, want, k)
        assert (got[0][copies].view(u32) == 0).all()
        for i in copies[[0, 1, 50, 99]]:
            assert np.array_equal(got[1][i], copies[copies != i][:k])
        others = np.setdiff1d(np.arange(130), copies)
        assert np.isinf(got[0][others]).all() and (got[1][others] == knn_np.NONE).all()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 5. a far outlier changes nobody's row and has an incomplete one
# ------------------------------------------------------------------------------------------------

def test_far_outlier(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 3, 0
    rows = pod_rows(gs, sh, cov)
    pts = ref["pw"][np.isfinite(ref["pw"]).all(axis=1)]
    far = rows[11:12].copy()
    far[0, :12] = (f32(1000.0) * (pts.max(axis=0) - pts.min(axis=0)).max() * np.ones(3, f32)).view(np.uint8)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), np.concatenate([rows, far]))
    mt = gs.model_transform_pod(**MT)
    for r, (wd, wi) in zip(ref["radii"][:2], ref["rows"][:2]):
        d, ix = _knn(buf, stream, 8, r, mt=mt)
        _same((d[:N], ix[:N]), (wd[:, :8], wi[:, :8]), r)
        assert np.isinf(d[N]).all() and (ix[N] == knn_np.NONE).all()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 6. a dense cell, a long row of cells, the first and last cell of every axis
# ------------------------------------------------------------------------------------------------

def test_dense_cell_and_long_row(gs, device, stream):
    rng = np.random.default_rng(21)
    r = 1.0
    # 300 points inside one cell (cells of side about r from the box's corner at 0): a run of more than four batches of 64
    dense = (f32([5.5, 5.5, 5.5]) + rng.uniform(-0.2, 0.2, (300, 3))).astype(f32)
    # 64 points in the first row of cells, 0.2 apart: consecutive in the sorted order, spread over 13 cells (NB_SPAN + 1 = 7)
    line = np.stack([0.2 * np.arange(64), np.full(64, 0.5), np.full(64, 0.5)], axis=1).astype(f32)
    hi = 12.8
    corners = np.array([[x, y, z] for x in (0.0, hi) for y in (0.0, hi) for z in (0.0, hi)], f32)
    near_corners = (corners + np.where(corners > 0, -0.3, 0.3)).astype(f32)
    p = np.concatenate([dense, line, corners, near_corners, rng.uniform(0, hi, (400, 3)).astype(f32)])
    p = p[rng.permutation(len(p))]
    buf, _ = _buffer_at(gs, device, p)
    for k in (1, 8, 16):
        want = knn_np.rows(p, k, r)
        _same(_knn(buf, stream, k, r), want, k)
    assert knn_np.row_kinds(want[0])[1].sum() >= 300
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 7. among and queries: what is written and what is not
# ------------------------------------------------------------------------------------------------

def test_among_and_queries(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 0, 0
    rows = pod_rows(gs, sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    mt = gs.model_transform_pod(**MT)
    rng = np.random.default_rng(5)
    among_mask, query_mask = rng.random(N) < 0.6, rng.random(N) < 0.4
    query_mask[4992:] = True
    assert (query_mask & ~among_mask).any() and (~query_mask & among_mask).any()
    among, queries = selection_from_mask(gs, device, stream, among_mask), selection_from_mask(gs, device, stream, query_mask)
    k, r, extra = 5, ref["radii"][1], 7
    wd, wi = knn_np.rows(ref["pw"], k, r, among_mask)
    fill = np.full(N * k + extra, 0xA5A5A5A5, u32)
    for q_sel, q_mask in ((queries, query_mask), (None, np.ones(N, bool))):
        d, ix = gs.Buffer(device, data=fill), gs.Buffer(device, data=fill)
        out = buf.knn(stream, k, r, among=among, queries=q_sel, model_transform=mt, dist2_out=d, index_out=ix)
        assert out[0] is d and out[1] is ix
        gd, gi = np.asarray(d.download(stream, u32)), np.asarray(ix.download(stream, u32))
        assert (gd[N * k:] == 0xA5A5A5A5).all() and (gi[N * k:] == 0xA5A5A5A5).all()       # bytes behind 4 k n
        gd, gi = gd[:N * k].reshape(N, k), gi[:N * k].reshape(N, k)
        assert (gd[~q_mask] == 0xA5A5A5A5).all() and (gi[~q_mask] == 0xA5A5A5A5).all()     # rows outside the queries
        assert np.array_equal(gd[q_mask], wd.view(u32)[q_mask]) and np.array_equal(gi[q_mask], wi[q_mask])
        outside = q_mask & ~among_mask                                                    # a query outside among
        assert np.isnan(gd.view(f32)[outside]).all() and (gi[outside] == knn_np.NONE).all()
        d.release(); ix.release()
    # nobody's neighbour: the rows among a subset are those of the subset alone, indices renumbered
    sub = knn_np.rows(ref["pw"][among_mask], k, r)
    assert np.array_equal(wd[among_mask].view(u32), sub[0].view(u32))
    # queries that select nothing write nothing
    none = selection_from_mask(gs, device, stream, np.zeros(N, bool))
    d = gs.Buffer(device, data=fill)
    buf.knn(stream, k, r, among=among, queries=none, model_transform=mt, dist2_out=d)
    assert (np.asarray(d.download(stream, u32)) == 0xA5A5A5A5).all()
    d.release()
    assert np.array_equal(buffer_rows(buf, stream), rows)
    for o in (among, queries, none):
        o.destroy()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 8. knn_auto: the rows without a radius guess
# ------------------------------------------------------------------------------------------------

def test_knn_auto_equals_one_call_at_its_radius(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 2, 1
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    # the default first radius, and one with a median count of 0: several passes over the incomplete rows
    for k, radius0 in ((3, None), (8, ref["radii"][0])):
        d, ix, radius, passes = buf.knn_auto(stream, k, model_transform=mt, radius0=radius0)
        got = (np.asarray(d.download(stream, f32))[:N * k].reshape(N, k), np.asarray(ix.download(stream, u32))[:N * k].reshape(N, k))
        assert radius > 0 and 1 <= passes <= 24 and (radius0 is None or (passes >= 3 and radius == float(f32(radius0)) * 2 ** (passes - 1)))
        _same(got, _knn(buf, stream, k, radius, mt=mt), k)
        _same(got, knn_np.rows(ref["pw"], k, radius), k)
        pt, complete = knn_np.row_kinds(got[0])
        assert complete[pt].all() and not pt[5:8].any()
        d.release(); ix.release()
    buf.destroy()


def test_knn_auto_ends(gs, device, stream):
    rng = np.random.default_rng(3)
    # points <= k: no row can be complete, the search ends at the box's diagonal
    p = rng.uniform(-1, 1, (5, 3)).astype(f32)
    buf, _ = _buffer_at(gs, device, p)
    d, ix, radius, passes = buf.knn_auto(stream, 8)
    got = (np.asarray(d.download(stream, f32))[:40].reshape(5, 8), np.asarray(ix.download(stream, u32))[:40].reshape(5, 8))
    _same(got, knn_np.rows(p, 8, radius))
    assert passes < 24 and np.isfinite(got[0][:, :4]).all() and np.isinf(got[0][:, 4:]).all()
    d.release(); ix.release(); buf.destroy()
    # all duplicates: the box has no extent, one pass at radius 0
    p = np.tile(f32([[0.3, -1.7, 2.9]]), (50, 1))
    buf, _ = _buffer_at(gs, device, p)
    for k in (3, 16):
        d, ix, radius, passes = buf.knn_auto(stream, k)
        got = (np.asarray(d.download(stream, f32))[:50 * k].reshape(50, k), np.asarray(ix.download(stream, u32))[:50 * k].reshape(50, k))
        assert radius == 0.0 and passes == 1
        _same(got, knn_np.rows(p, k, 0.0))
        assert (got[0].view(u32) == 0).all()
        d.release(); ix.release()
    buf.destroy()
    p = np.tile(f32([[0.3, -1.7, 2.9]]), (10, 1))      # ... and with fewer copies than k it still ends, incomplete
    buf, _ = _buffer_at(gs, device, p)
    d, ix, radius, passes = buf.knn_auto(stream, 16)
    got = np.asarray(d.download(stream, f32))[:160].reshape(10, 16)
    assert radius == 0.0 and passes == 1 and (got[:, :9] == 0).all() and np.isinf(got[:, 9:]).all()
    d.release(); ix.release(); buf.destroy()
    # no Gaussian at all
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(3, 0), np.zeros((0, gs.GaussianPod(3, 0).size), np.uint8))
    d, ix, radius, passes = buf.knn_auto(stream, 4)
    assert passes == 1
    d.release(); ix.release(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 9. select_knn: both statistics, the five ops, the ends of the range
# ------------------------------------------------------------------------------------------------

def _plane_of(gs, device, d2):
    return gs.Buffer(device, data=np.ascontiguousarray(d2, f32).reshape(-1)) if d2.size else gs.Buffer(device, size=4)


def test_select_knn(gs, device, stream):
    ref = _scene_ref(gs)
    k = 8
    d2 = ref["rows"][1][0][:, :k]
    plane = _plane_of(gs, device, d2)
    pt, complete = knn_np.row_kinds(d2)
    prior = np.random.default_rng(7).random(N) < 0.5
    sel = gs.Selection(device, N)
    for kind in (knn_np.KTH_DIST2, knn_np.MEAN_DIST):
        v = knn_np.statistic(d2, kind)
        q1, q2 = np.quantile(v[complete].astype(np.float64), [0.25, 0.75])
        exact = float(v[complete][17])      # a bound that is a value of the plane: the range is closed
        ranges = ((0.0, q1), (q1, q2), (q2, INF), (exact, exact), (-INF, INF), (INF, INF), (q2, q1), (-1.0, -0.5))
        for op in SELECT_OPS:
            for lo, hi in ranges:
                sel.upload(stream, prior)
                sel.select_knn(stream, plane, k, kind, lo, hi, op)
                want = np_op(prior, knn_np.in_range(d2, kind, lo, hi), op)
                assert np.array_equal(sel.download_words(stream), stats_np.pack_bits(want)), (kind, op, lo, hi)
        assert knn_np.in_range(d2, kind, exact, exact).any() and 0 < knn_np.in_range(d2, kind, 0.0, q1).sum() < N
        assert not knn_np.in_range(d2, kind, q2, q1).any()
        # lo = hi = +inf: exactly the incomplete rows; a NaN row never
        assert np.array_equal(knn_np.in_range(d2, kind, INF, INF), pt & ~complete)
        assert np.array_equal(knn_np.in_range(d2, kind, -INF, INF), pt) and not pt[5:8].any()
    # the statistic by name, and a tail that stays clear
    n = 65
    small = gs.Selection(device, n)
    for op in SELECT_OPS:
        small.fill(stream)
        small.select_knn(stream, plane, k, "mean_dist", -INF, INF, op)
        words = small.download_words(stream)
        assert len(words) == 3 and words[2] >> 1 == 0
        assert np.array_equal(words, stats_np.pack_bits(np_op(np.ones(n, bool), pt[:n], op)))
    small.destroy(); sel.destroy(); plane.release()


# ------------------------------------------------------------------------------------------------
# 10. knn_summary
# ------------------------------------------------------------------------------------------------

def _check_summary(gs, stream, plane, d2, k, kind):
    n = len(d2)
    want = knn_np.summary(d2, kind)
    a, b = gs.knn_summary(stream, plane, n, k, kind), gs.knn_summary(stream, plane, n, k, kind)
    assert (a.points, a.complete) == (want["points"], want["complete"])
    assert f32(a.min).view(u32) == f32(want["min"]).view(u32) and f32(a.max).view(u32) == f32(want["max"]).view(u32)
    eps = want["complete"] * 2.0 ** -52
    assert abs(a.sum - want["sum"]) <= eps * want["abs_sum"], (a.sum, want["sum"])
    assert abs(a.sum_sq - want["sum_sq"]) <= eps * want["sum_sq"], (a.sum_sq, want["sum_sq"])
    # the same bits from run to run
    assert np.float64(a.sum).view(np.uint64) == np.float64(b.sum).view(np.uint64)
    assert np.float64(a.sum_sq).view(np.uint64) == np.float64(b.sum_sq).view(np.uint64)
    return a


@pytest.mark.parametrize("kind", [knn_np.KTH_DIST2, knn_np.MEAN_DIST])
def test_knn_summary(gs, device, stream, kind):
    ref = _scene_ref(gs)
    for k, which in ((8, 1), (3, 1), (16, 2), (1, 1)):
        d2 = ref["rows"][which][0][:, :k]
        plane = _plane_of(gs, device, d2)
        s = _check_summary(gs, stream, plane, d2, k, kind)
        assert 0 < s.complete <= s.points == N - 3 and 0 <= s.min <= s.max < INF and s.std > 0
        plane.release()
    # an all-incomplete plane, and no row at all
    d2 = ref["rows"][0][0][:257, :16]
    assert not knn_np.row_kinds(d2)[1].any()
    plane = _plane_of(gs, device, d2)
    s = _check_summary(gs, stream, plane, d2, 16, kind)
    assert s.complete == 0 and s.points == 254 and s.min == INF and s.max == -INF and s.sum == 0 and s.sum_sq == 0
    s = gs.knn_summary(stream, plane, 0, 16, kind)
    assert (s.points, s.complete, s.sum, s.sum_sq) == (0, 0, 0.0, 0.0) and s.min == INF and s.max == -INF
    plane.release()


# ------------------------------------------------------------------------------------------------
# 11. argument errors
# ------------------------------------------------------------------------------------------------

def test_argument_errors_change_nothing(gs, device, stream):
    sh, cov = 0, 0
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mask = np.random.default_rng(9).random(N) < 0.3
    sel, short = selection_from_mask(gs, device, stream, mask), gs.Selection(device, N - 1)
    other = gs.Device(0)          # a second device object: its objects belong to another device
    k = 4
    foreign, foreign_plane = gs.Selection(other, N), gs.Buffer(other, size=4 * k * N)
    words = sel.download_words(stream)
    fill = np.full(N * k, 0x5A5A5A5A, u32)
    plane, index, small = gs.Buffer(device, data=fill), gs.Buffer(device, data=fill), gs.Buffer(device, size=4 * k * N - 4)
    L, bad = gs._L, gs.InvalidArgumentError.code
    mt = C.byref(gs.model_transform_pod(**MT))
    nan, inf = float("nan"), INF

    def knn(g=buf._h, among=sel._h, queries=None, k=k, r=0.5, d=plane._h, ix=index._h):
        return L.gs_gaussians_buffer_knn(g, stream._h, among, queries, mt, k, r, d, ix)

    assert knn(g=None) == bad and knn(d=None) == bad
    for r in (-1.0, nan, inf, -inf, 1e20):
        assert knn(r=r) == bad, r
    assert knn(k=0) == bad and knn(k=17) == bad
    assert knn(d=small._h) == bad and knn(ix=small._h) == bad      # a short plane
    assert knn(k=5) == bad                                          # ... and one that is short for this k
    assert knn(d=foreign_plane._h) == bad and knn(ix=foreign_plane._h) == bad
    assert knn(among=short._h) == bad and knn(among=foreign._h) == bad
    assert knn(queries=short._h) == bad and knn(queries=foreign._h) == bad
    for b in (plane, index):
        assert np.array_equal(np.asarray(b.download(stream, u32)), fill)

    def select(s=sel._h, p=plane._h, k=k, kind=0, lo=0.0, hi=1.0, op=0):
        return L.gs_select_knn(s, stream._h, p, k, kind, lo, hi, op)

    assert select(s=None) == bad and select(p=None) == bad
    assert select(op=5) == bad and select(op=-1) == bad and select(kind=2) == bad
    assert select(k=0) == bad and select(k=17) == bad and select(k=5) == bad
    assert select(lo=nan) == bad and select(hi=nan) == bad
    assert select(p=small._h) == bad and select(p=foreign_plane._h) == bad and select(s=foreign._h) == bad
    assert np.array_equal(sel.download_words(stream), words)

    out = gs._capi.KnnSummaryRecord()
    out.points = 77

    def summary(p=plane._h, n=N, k=k, kind=0, o=C.byref(out)):
        return L.gs_knn_summary(stream._h, p, n, k, kind, o)

    assert summary(p=None) == bad and summary(o=None) == bad
    assert summary(k=0) == bad and summary(k=17) == bad and summary(kind=2) == bad
    assert summary(n=N + 1) == bad and summary(p=small._h) == bad and summary(n=1 << 32) == bad
    assert summary(p=foreign_plane._h) == bad      # the stream belongs to another device
    assert out.points == 77
    # and the valid calls next to them
    assert knn(r=0.0, k=1) == 0 and knn(ix=None, queries=sel._h) == 0 and select(lo=2.0, hi=1.0, op=1) == 0 and summary(n=N - 1) == 0
    stream.synchronize()
    for o in (sel, short, foreign):
        o.destroy()
    for o in (plane, index, small, foreign_plane):
        o.release()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 12. ordering behind an edit on another stream
# ------------------------------------------------------------------------------------------------

def test_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    orig = pod_rows(gs, sh, cov)
    mask = np.random.default_rng(4).random(N) < 0.3
    s1, s2 = stream, device.create_stream()
    sel = selection_from_mask(gs, device, s1, mask)
    s1.synchronize()
    edited = edited_pods(gs, sh, cov, orig.reshape(-1), mask, 15).reshape(N, pod.size)
    pw, before = neighbors_np.positions(edited), neighbors_np.positions(orig)
    k, r = 4, _kth_distance(before, 8)
    want, unedited = knn_np.rows(pw, k, r), knn_np.rows(before, k, r)
    assert not np.array_equal(want[1], unedited[1]), "the edit changes the rows"
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
    buf.edit(s1, sel, sample_edit(gs, 15))
    # on stream 2 right behind the edit on stream 1, no host synchronisation in between
    _same(_knn(buf, s2, k, r), want)
    s1.synchronize()
    assert np.array_equal(buffer_rows(buf, s1), edited)
    # ... and a call on stream 1 behind the one on stream 2 reuses the scratch
    _same(_knn(buf, s1, k, r), want)
    s2.synchronize()
    buf.destroy(); sel.destroy()
    s2.close()


# ------------------------------------------------------------------------------------------------
# 13. statistical outlier removal
# ------------------------------------------------------------------------------------------------

def test_statistical_outliers(gs, device, stream):
    rng = np.random.default_rng(17)
    nb, k, sigma = 1500, 8, 2.0
    blob = rng.standard_normal((nb, 3)).astype(f32)
    u = rng.standard_normal((20, 3))
    planted = (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(8, 12, (20, 1))).astype(f32)
    where = np.sort(rng.permutation(nb + 20)[:20])
    is_planted = np.zeros(nb + 20, bool)
    is_planted[where] = True
    p = np.empty((nb + 20, 3), f32)
    p[is_planted], p[~is_planted] = planted, blob
    buf, _ = _buffer_at(gs, device, p)
    sel = gs.Selection(device, len(p))
    sel.fill(stream)
    threshold, radius = sel.select_statistical_outliers(stream, buf, k=k, sigma=sigma)
    got = sel.download(stream)
    # the restatement: the rows at the radius the search ended with, mean + sigma std in binary64
    d2 = knn_np.rows(p, k, radius)[0]
    v = knn_np.statistic(d2, knn_np.MEAN_DIST)
    pt, complete = knn_np.row_kinds(d2)
    w = v[complete].astype(np.float64)
    mine = w.mean() + sigma * w.std()
    assert abs(threshold - mine) <= 1e-12 * mine
    for t in (mine, threshold):      # the condition, on the restatement: all 20, fewer than 5 % of the blob
        want = pt & (v.astype(np.float64) > t)
        assert want[is_planted].all() and want[~is_planted].sum() < 0.05 * nb
    assert np.array_equal(got, want)
    sel.destroy(); buf.destroy()
