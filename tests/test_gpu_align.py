"""Nearest neighbours between two buffers, overlap select, Chamfer distance, pair sums and ICP on the device (DESIGN.md
§3.19) against the brute-force numpy restatement of tests/align_np.py: rows, indices, selection words and counts bit for
bit; every binary64 sum inside count 2^-52 sum |v|, the bound of tests/test_gpu_stats.py (the first-order bound of any
summation order, doubled).  The row is defined without a grid, so the restatement has none; the small targets, the
duplicates, the queries outside the target's box and the far outlier are the inputs a grid gets wrong."""
import ctypes as C
import math

import numpy as np
import pytest

import align_np
import neighbors_np
from records import SELECT_OPS, buffer_rows, np_op, selection_from_mask
from scenes import FOUR_LAYOUTS, pod_rows

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
KS = (1, 3, 8, 16)
NQ, NT = 1500, 2003      # n_q is no multiple of 64 or 256
POISON = 0xA5A5A5A5
# two different transforms: rotation + translation + non-uniform scale each
QQ, QT = np.array([0.3, -0.5, 0.2, 0.7]), np.array([-0.2, 0.4, 0.1, 0.8])
MTQ = dict(pos=(0.5, -0.25, 1.5), rot=tuple((QQ / np.linalg.norm(QQ)).astype(f32)), scale=(1.25, 0.75, 2.0))
MTT = dict(pos=(0.25, 0.0, 1.25), rot=tuple((QT / np.linalg.norm(QT)).astype(f32)), scale=(1.5, 1.0, 1.75))

_REF = {}


def _cross_counts(pq, pt, r):
    """per finite query the number of finite targets within r (binary64; only used to PICK and describe radii)"""
    q, t = pq[np.isfinite(pq).all(axis=1)].astype(np.float64), pt[np.isfinite(pt).all(axis=1)].astype(np.float64)
    return np.concatenate([(((q[a:a + 512, None, :] - t[None, :, :]) ** 2).sum(axis=2) <= r * r).sum(axis=1) for a in range(0, len(q), 512)])


def _kth_cross_distance(pq, pt, k):
    """median over the finite queries of the distance to the k-th nearest finite target (k = 1: the nearest)"""
    q, t = pq[np.isfinite(pq).all(axis=1)].astype(np.float64), pt[np.isfinite(pt).all(axis=1)].astype(np.float64)
    out = [np.sqrt(np.partition(((q[a:a + 512, None, :] - t[None, :, :]) ** 2).sum(axis=2), k - 1, axis=1)[:, k - 1]) for a in range(0, len(q), 512)]
    return float(np.median(np.concatenate(out)))


def _scene_ref(gs):
    """pw of both sides under their transforms, three radii (median count 0, about 8, more than half of the target) and the
    restatement's rows of 16 for each (the row of k is its first k entries: tests/test_align_api.py); computed once, never
    written to"""
    if not _REF:
        pq = neighbors_np.positions(pod_rows(gs, 3, 0, NQ, 3), **MTQ)
        pt = neighbors_np.positions(pod_rows(gs, 3, 0, NT, 5), **MTT)
        radii = [0.5 * _kth_cross_distance(pq, pt, 1), _kth_cross_distance(pq, pt, 8), _kth_cross_distance(pq, pt, (6 * NT) // 10)]
        med = [float(np.median(_cross_counts(pq, pt, r))) for r in radii]
        assert med[0] == 0 and 4 <= med[1] <= 16 and med[2] > NT / 2, med
        rows = [align_np.rows_between(pq, pt, 16, r)[:2] for r in radii]
        for k in (8, 16):      # incomplete and complete rows both occur at the middle radius
            d = rows[1][0][:, k - 1]
            assert np.isfinite(d).any() and np.isinf(d).any(), k
        for a in [pq, pt] + [x for pair in rows for x in pair]:
            a.setflags(write=False)
        _REF.update(pq=pq, pt=pt, radii=radii, rows=rows)
    return _REF


def _knn_to(qbuf, tbuf, stream, k, r, **kw):
    """(d2 float32[n_q, k], index uint32[n_q, k]) of one knn_to call into new planes"""
    d, ix = qbuf.knn_to(stream, tbuf, k, r, indices=True, **kw)
    n = qbuf.len()
    got = (np.asarray(d.download(stream, f32))[:n * k].reshape(n, k).copy(), np.asarray(ix.download(stream, u32))[:n * k].reshape(n, k).copy())
    d.release(); ix.release()
    return got


def _same(got, want, what=""):
    assert got[0].dtype == f32 and got[1].dtype == u32
    assert np.array_equal(got[0].view(u32), want[0].view(u32)), ("d2", what)
    assert np.array_equal(got[1], want[1]), ("index", what)


def _buffer_at(gs, device, positions, sh=3, cov=0):
    """a buffer of one layout with the given positions"""
    import synth
    positions = np.asarray(positions, f32).reshape(-1, 3)
    pod = gs.GaussianPod(sh, cov)
    if not len(positions):
        return gs.GaussiansBuffer.new_with_pods(device, pod, np.zeros((0, pod.size), np.uint8))
    g = synth.scene(len(positions), first=3)
    g["pos"] = positions
    return gs.GaussiansBuffer.new_with_pods(device, pod, np.asarray(pod.from_gaussian(g)).reshape(len(positions), pod.size))


def _check_positions(gs, device, stream, pq, pt, radii, ks, what):
    pq, pt = np.asarray(pq, f32).reshape(-1, 3), np.asarray(pt, f32).reshape(-1, 3)
    qb, tb = _buffer_at(gs, device, pq), _buffer_at(gs, device, pt, 1, 2)
    for r in radii:
        for k in ks:
            _same(_knn_to(qb, tb, stream, k, r), align_np.rows_between(pq, pt, k, r)[:2], (what, r, k))
    qb.destroy(); tb.destroy()


# ------------------------------------------------------------------------------------------------
# 1. four layouts, three radii, four values of k, each side under its own transform
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_rows_equal_the_restatement(gs, device, stream, sh, cov):
    ref = _scene_ref(gs)
    tsh, tcov = FOUR_LAYOUTS[(FOUR_LAYOUTS.index((sh, cov)) + 1) % 4]      # the two sides differ in layout too
    qrows, trows = pod_rows(gs, sh, cov, NQ, 3), pod_rows(gs, tsh, tcov, NT, 5)
    assert np.array_equal(neighbors_np.positions(qrows, **MTQ).view(u32), ref["pq"].view(u32))
    assert np.array_equal(neighbors_np.positions(trows, **MTT).view(u32), ref["pt"].view(u32))
    qb = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), qrows)
    tb = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(tsh, tcov), trows)
    mq, mt = gs.model_transform_pod(**MTQ), gs.model_transform_pod(**MTT)
    for r, (wd, wi) in zip(ref["radii"], ref["rows"]):
        for k in KS:
            got = _knn_to(qb, tb, stream, k, r, model_transform=mq, target_transform=mt)
            _same(got, (wd[:, :k], wi[:, :k]), (r, k))
            assert np.isnan(got[0][5:8]).all() and (got[1][5:8] == align_np.NONE).all()      # the planted NaN / inf queries
            assert not np.isin(got[1], [5, 6, 7]).any()                                      # ... and targets
    # without the index plane: the same distances
    d = qb.knn_to(stream, tb, 8, ref["radii"][1], model_transform=mq, target_transform=mt)
    assert isinstance(d, gs.Buffer)
    assert np.array_equal(np.asarray(d.download(stream, u32))[:8 * NQ], ref["rows"][1][0][:, :8].reshape(-1).view(u32))
    d.release()
    assert np.array_equal(buffer_rows(qb, stream), qrows) and np.array_equal(buffer_rows(tb, stream), trows)
    qb.destroy(); tb.destroy()


# ------------------------------------------------------------------------------------------------
# 2. the shapes a grid gets wrong
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,nt", [(0, 40), (1, 1), (65, 1), (257, 37), (1025, 63), (100, 0), (64, 65)])
def test_small_buffers(gs, device, stream, nq, nt):
    rng = np.random.default_rng(100 * nq + nt)
    pq, pt = rng.uniform(-1, 1, (nq, 3)).astype(f32), rng.uniform(-1, 1, (nt, 3)).astype(f32)
    if nq > 3:
        pq[2, 1] = np.nan
    _check_positions(gs, device, stream, pq, pt, (0.0, 0.3, 4.0), (1, 3, 16), (nq, nt))


def test_a_target_without_points_gives_incomplete_rows(gs, device, stream):
    rng = np.random.default_rng(5)
    pq = rng.uniform(-1, 1, (70, 3)).astype(f32)
    pq[9, 0] = np.inf
    pt = np.full((90, 3), np.nan, f32)
    pt[::2, 1] = 1.0
    qb, tb = _buffer_at(gs, device, pq), _buffer_at(gs, device, pt)
    got = _knn_to(qb, tb, stream, 3, 1.0)
    _same(got, align_np.rows_between(pq, pt, 3, 1.0)[:2])
    point = np.arange(70) != 9
    assert np.isinf(got[0][point]).all() and np.isnan(got[0][9]).all() and (got[1] == align_np.NONE).all()
    # ... and so does an empty `among` over a target that has points
    tb2 = _buffer_at(gs, device, rng.uniform(-1, 1, (90, 3)).astype(f32))
    none = selection_from_mask(gs, device, stream, np.zeros(90, bool))
    _same(_knn_to(qb, tb2, stream, 3, 1.0, among=none), got)
    stream.synchronize()
    none.destroy(); qb.destroy(); tb.destroy(); tb2.destroy()


def test_target_duplicates_are_streamed_in_two_batches(gs, device, stream):
    """150 copies of one target point in one cell: a run longer than 64; r = 0 finds exactly them, smallest indices first"""
    rng = np.random.default_rng(12)
    pt = rng.uniform(-2, 2, (200, 3)).astype(f32)
    copies = np.sort(rng.permutation(200)[:150])
    pt[copies] = f32([0.3, -1.7, 1.9])
    pq = rng.uniform(-2, 2, (77, 3)).astype(f32)
    pq[[4, 40, 76]] = f32([0.3, -1.7, 1.9])            # cross-buffer duplicates: distance +0
    pq[10] = f32([0.3, -1.7, 1.9]) + f32(0.01)
    qb, tb = _buffer_at(gs, device, pq), _buffer_at(gs, device, pt)
    for r in (0.0, 0.05, 1.0):
        for k in (1, 3, 16):
            want = align_np.rows_between(pq, pt, k, r)[:2]
            got = _knn_to(qb, tb, stream, k, r)
            _same(got, want, (r, k))
            for i in (4, 40, 76):
                assert (got[0][i].view(u32) == 0).all() and np.array_equal(got[1][i], copies[:k])
    assert np.isinf(_knn_to(qb, tb, stream, 1, 0.0)[0][[0, 10]]).all()
    qb.destroy(); tb.destroy()


def test_queries_on_a_line_and_outside_the_box(gs, device, stream):
    """the target is a lattice of spacing 0.25 in [0, 2]^3: with r = 0.25 the cells are about one spacing wide.  Queries on a
    line of adjacent cells search in NB_SPAN groups; queries outside the box on each axis and side, within r of it and
    well beyond, get the cells at the border or none"""
    k = np.arange(9, dtype=f32) * f32(0.25)
    pt = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    line = np.stack([np.linspace(-0.3, 2.3, 131, dtype=f32), np.full(131, 1.01, f32), np.full(131, 0.74, f32)], axis=1)
    outside = []
    for axis in range(3):
        for side, far in ((-1, False), (-1, True), (1, False), (1, True)):
            for _ in range(6):
                p = np.random.default_rng(len(outside)).uniform(0, 2, 3)
                off = (0.6 + 5 * len(outside) if far else np.random.default_rng(len(outside)).uniform(0.0, 0.26))
                p[axis] = -off if side < 0 else 2 + off
                outside.append(p)
    pq = np.concatenate([line, np.array(outside, f32), f32([[-0.25, -0.25, -0.25], [2.25, 2.25, 2.25], [1e6, 1, 1], [-3e9, 1, 1]])])
    rng = np.random.default_rng(8)
    pq = pq[rng.permutation(len(pq))]                  # sorted order != caller order
    assert len(pq) % 64
    _check_positions(gs, device, stream, pq, pt, (0.25, 0.26, 0.5), (1, 7, 16), "line")
    want = align_np.rows_between(pq, pt, 1, 0.5)[0][:, 0]
    assert np.isfinite(want).sum() > 140 and np.isinf(want).sum() > 30


def test_far_target_outlier_gives_a_coarse_grid(gs, device, stream):
    """one target 10^8 away: extent 2^-21 = 95 is above the radius, so a cell is wider than r and holds many points"""
    ref = _scene_ref(gs)
    pt = np.array(ref["pt"][:300])
    pt[50] = f32([1e8, -1e8, 1e8])
    pq = np.array(ref["pq"][:333])
    pq[60] = f32([1e8, -1e8, 1e8]) + f32(1e-3)          # rounds onto the outlier: the spacing of binary32 is 8 there
    r = ref["radii"][1]
    assert r < 90
    _check_positions(gs, device, stream, pq, pt, (r, 0.0), (1, 8), "outlier")
    d2, ix, _ = align_np.rows_between(pq, pt, 1, r)
    assert ix[60, 0] == 50 and d2[60, 0] == 0 and 30 < np.isfinite(d2[:, 0]).sum() < 333


# ------------------------------------------------------------------------------------------------
# 3. subsets, poison, NULL index plane, twice the radius, errors
# ------------------------------------------------------------------------------------------------

def _scene_buffers(gs, device):
    qb = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(1, 2), pod_rows(gs, 1, 2, NQ, 3))
    tb = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(2, 1), pod_rows(gs, 2, 1, NT, 5))
    return qb, tb, gs.model_transform_pod(**MTQ), gs.model_transform_pod(**MTT)


def test_subsets_leave_other_rows_and_the_tail_untouched(gs, device, stream):
    ref = _scene_ref(gs)
    qb, tb, mq, mt = _scene_buffers(gs, device)
    rng = np.random.default_rng(21)
    q_mask, a_mask = rng.random(NQ) < 0.4, rng.random(NT) < 0.7
    q_mask[[5, 6]] = True
    qsel, asel = selection_from_mask(gs, device, stream, q_mask), selection_from_mask(gs, device, stream, a_mask)
    r, extra = ref["radii"][1], 37
    for k in (3, 16):
        fill = np.full(NQ * k + extra, POISON, u32)
        d, ix = gs.Buffer(device, data=fill), gs.Buffer(device, data=fill)
        qb.knn_to(stream, tb, k, r, queries=qsel, among=asel, model_transform=mq, target_transform=mt, dist2_out=d, index_out=ix)
        gd, gi = np.asarray(d.download(stream, u32)), np.asarray(ix.download(stream, u32))
        assert (gd[NQ * k:] == POISON).all() and (gi[NQ * k:] == POISON).all()                 # bytes behind 4 k n_q
        gd, gi = gd[:NQ * k].reshape(NQ, k), gi[:NQ * k].reshape(NQ, k)
        assert (gd[~q_mask] == POISON).all() and (gi[~q_mask] == POISON).all()                 # rows outside the queries
        wd, wi, written = align_np.rows_between(ref["pq"], ref["pt"], k, r, q_mask, a_mask)
        assert np.array_equal(written, q_mask)
        assert np.array_equal(gd[q_mask], wd[q_mask].view(u32)) and np.array_equal(gi[q_mask], wi[q_mask])
        assert a_mask[gi[q_mask][gi[q_mask] != align_np.NONE]].all()
        d.release(); ix.release()
    stream.synchronize()
    qsel.destroy(); asel.destroy(); qb.destroy(); tb.destroy()


def test_a_complete_row_is_unchanged_at_twice_the_radius(gs, device, stream):
    ref = _scene_ref(gs)
    qb, tb, mq, mt = _scene_buffers(gs, device)
    r = ref["radii"][1]
    for k in (1, 8):
        a = _knn_to(qb, tb, stream, k, r, model_transform=mq, target_transform=mt)
        b = _knn_to(qb, tb, stream, k, 2 * r, model_transform=mq, target_transform=mt)
        complete = np.isfinite(a[0][:, -1])
        assert complete.any() and not complete.all()
        assert np.array_equal(a[0][complete].view(u32), b[0][complete].view(u32)) and np.array_equal(a[1][complete], b[1][complete])
        held = np.isfinite(a[0])      # an incomplete row only grows: its entries stay a prefix
        assert np.array_equal(a[0][held].view(u32), b[0][held].view(u32)) and np.array_equal(a[1][held], b[1][held])
    qb.destroy(); tb.destroy()


def test_errors_leave_the_planes_untouched(gs, device, stream):
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    qb, tb, mq, mt = _scene_buffers(gs, device)
    k = 3
    fill = np.full(NQ * k, POISON, u32)
    d, ix, small = gs.Buffer(device, data=fill), gs.Buffer(device, data=fill), gs.Buffer(device, size=4 * k * NQ - 4)
    wrong_q, wrong_t = gs.Selection(device, NQ + 1), gs.Selection(device, NT - 1)
    right_q = gs.Selection(device, NQ)
    sums = gs._capi.PairSumsRecord()
    sums.pairs = 7

    def call(q=qb, t=tb, queries=None, among=None, kk=k, r=1.0, dist=d, index=ix):
        return lib.gs_gaussians_buffer_knn_between(q._h if q else None, t._h if t else None, stream._h, queries._h if queries else None,
                                                   among._h if among else None, C.byref(mq), C.byref(mt), kk, r, dist._h if dist else None,
                                                   index._h if index else None)
    for kw in (dict(q=None), dict(t=None), dict(dist=None), dict(t=qb), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")),
               dict(r=1e20), dict(kk=0), dict(kk=17), dict(dist=small), dict(index=small), dict(queries=wrong_q), dict(among=wrong_t),
               dict(queries=wrong_t), dict(among=right_q)):
        assert call(**kw) == bad, kw
    for kw in (dict(kk=0), dict(kk=17), dict(plane=small), dict(queries=wrong_q), dict(plane=None)):
        plane = kw.get("plane", ix)
        rc = lib.gs_gaussians_buffer_pair_sums(qb._h, tb._h, stream._h, kw["queries"]._h if "queries" in kw else None, None, None,
                                               plane._h if plane else None, kw.get("kk", k), C.byref(sums))
        assert rc == bad and sums.pairs == 7, kw
    stream.synchronize()
    assert (np.asarray(d.download(stream, u32)) == POISON).all() and (np.asarray(ix.download(stream, u32)) == POISON).all()
    # ... and the call still works afterwards
    assert call() == 0
    stream.synchronize()
    assert not (np.asarray(d.download(stream, u32)) == POISON).any()
    for o in (wrong_q, wrong_t, right_q, qb, tb):
        o.destroy()
    for b in (d, ix, small):
        b.release()


# ------------------------------------------------------------------------------------------------
# 4. the overlap select and the Chamfer distance
# ------------------------------------------------------------------------------------------------

def test_select_near_words_equal_the_restatement(gs, device, stream):
    ref = _scene_ref(gs)
    qb, tb, mq, mt = _scene_buffers(gs, device)
    rng = np.random.default_rng(33)
    a_mask = rng.random(NT) < 0.8
    asel = selection_from_mask(gs, device, stream, a_mask)
    r = ref["radii"][1] / 2
    near = np.isfinite(align_np.rows_between(ref["pq"], ref["pt"], 1, r, None, a_mask)[0][:, 0])
    assert 0.1 * NQ < near.sum() < 0.9 * NQ and not near[5:8].any()
    for op in range(len(SELECT_OPS)):
        before = rng.random(NQ) < 0.5
        sel = selection_from_mask(gs, device, stream, before)
        sel.select_near(stream, qb, tb, r, among=asel, model_transform=mq, target_transform=mt, op=op)
        assert np.array_equal(sel.download(stream), np_op(before, near, op)), SELECT_OPS[op]
        sel.destroy()
    asel.destroy(); qb.destroy(); tb.destroy()


def test_chamfer_counts_are_exact_and_sums_within_the_bound(gs, device, stream):
    ref = _scene_ref(gs)
    qb, tb, mq, mt = _scene_buffers(gs, device)
    r = ref["radii"][1] / 2
    ch = qb.chamfer_to(stream, tb, r, model_transform=mq, target_transform=mt)
    for got, (a, b) in ((ch.to_target, (ref["pq"], ref["pt"])), (ch.from_target, (ref["pt"], ref["pq"]))):
        d2 = align_np.rows_between(a, b, 1, r)[0][:, 0]
        point, complete = ~np.isnan(d2), np.isfinite(d2)
        v = np.sqrt(d2[complete]).astype(np.float64)
        assert v.dtype == np.float64 and np.sqrt(d2[complete]).dtype == f32
        assert (got.points, got.complete) == (int(point.sum()), int(complete.sum())) and 0 < got.complete < got.points
        bound = got.complete * 2.0 ** -52
        print("chamfer: sum error %.3g of a bound %.3g" % (abs(got.sum - math.fsum(v)), bound * math.fsum(v)))
        assert abs(got.sum - math.fsum(v)) <= bound * math.fsum(v) and abs(got.sum_sq - math.fsum(v * v)) <= bound * math.fsum(v * v)
    assert ch.incomplete_to == ch.to_target.points - ch.to_target.complete and ch.mean_to == ch.to_target.sum / ch.to_target.complete
    assert ch.distance == ch.mean_to + ch.mean_from
    qb.destroy(); tb.destroy()


# ------------------------------------------------------------------------------------------------
# 5. pair sums
# ------------------------------------------------------------------------------------------------

def _sums_array(s):
    return np.concatenate([s.sp, s.sq, s.spq.reshape(-1), [s.spp, s.sqq, s.sdd]])


def test_pair_sums_are_exact_in_count_and_within_the_bound(gs, device, stream):
    ref = _scene_ref(gs)
    qb, tb, mq, mt = _scene_buffers(gs, device)
    rng = np.random.default_rng(44)
    q_mask = rng.random(NQ) < 0.6
    q_mask[[5, 6, 7]] = True
    qsel = selection_from_mask(gs, device, stream, q_mask)
    r = ref["radii"][1]
    for k, queries, mask in ((1, None, None), (3, qsel, q_mask)):
        d, ix = qb.knn_to(stream, tb, k, r, queries=queries, model_transform=mq, target_transform=mt, indices=True)
        first = align_np.rows_between(ref["pq"], ref["pt"], k, r, mask)[1][:, 0]
        want = align_np.pair_sums(ref["pq"], ref["pt"], first, mask)
        a = qb.pair_sums(stream, tb, ix, k, queries=queries, model_transform=mq, target_transform=mt)
        b = qb.pair_sums(stream, tb, ix, k, queries=queries, model_transform=mq, target_transform=mt)
        assert a.pairs == want["pairs"] and 0.2 * NQ < a.pairs < NQ
        err, bound = np.abs(_sums_array(a) - want["sums"]), want["pairs"] * 2.0 ** -52 * want["abs"]
        print("pair_sums: largest error / (2^-52 sum |v|) = %.3g" % (err / (2.0 ** -52 * want["abs"])).max())
        assert (err <= bound).all(), (err, bound)
        assert bytes(a.record()) == bytes(b.record())                      # the same 152 bytes from run to run
        assert a.rms == pytest.approx(np.sqrt(want["sums"][17] / want["pairs"]), rel=1e-14)
        d.release(); ix.release()
    # an index plane of values >= n_t names no pair and is never followed
    for value in (NT, NT + 1, 0x7FFFFFFF, align_np.NONE):
        plane = gs.Buffer(device, data=np.full(NQ, value, u32))
        s = qb.pair_sums(stream, tb, plane, 1)
        assert s.pairs == 0 and not _sums_array(s).any()
        plane.release()
    # ... an empty query buffer gives zeros
    empty = _buffer_at(gs, device, np.zeros((0, 3), f32))
    plane = gs.Buffer(device, size=4)
    assert empty.pair_sums(stream, tb, plane, 1).pairs == 0
    plane.release(); empty.destroy()
    qsel.destroy(); qb.destroy(); tb.destroy()


# ------------------------------------------------------------------------------------------------
# 6. ICP on the lattice input
# ------------------------------------------------------------------------------------------------

def _adjacent(a, b):
    """how far apart two binary32 values are, in representable values"""
    def key(x):
        v = np.asarray(x, f32).view(u32).astype(np.int64)
        return np.where(v & 0x80000000, -(v & 0x7FFFFFFF), v)
    return np.abs(key(a) - key(b))


def test_align_to_on_the_lattice_input(gs, device, stream):
    case = align_np.icp_case()
    target, query, mate = case["target"], case["query"], case["mate"]
    qb, tb = _buffer_at(gs, device, query, 2, 1), _buffer_at(gs, device, target, 0, 0)
    before_q, before_t = buffer_rows(qb, stream).copy(), buffer_rows(tb, stream).copy()
    radius = 0.45
    pod, report = qb.align_to(stream, tb, radius)
    # iteration 1 pairs every query with its true mate (tests/test_align_api.py shows that in numpy); its fit is exact, so
    # iteration 2 measures an RMS at the rounding level of binary32 and stops
    assert report.stopped == "converged" and len(report.iterations) == 2, report
    (pairs1, rms1), (pairs2, rms2) = report.iterations
    assert pairs1 == pairs2 == len(query) and rms2 < 1e-5 < 0.05 < rms1
    d, ix = qb.knn_to(stream, tb, 1, radius, indices=True)
    assert np.array_equal(np.asarray(ix.download(stream, u32))[:len(query)], mate)
    d.release(); ix.release()
    # the pod against gs_rigid_fit of the restatement's sums, composed with the default pod
    s = align_np.pair_sums(query, target, mate.astype(u32))
    v = s["sums"]
    delta, rms = gs.rigid_fit(gs.PairSums(pairs=s["pairs"], sp=v[0:3], sq=v[3:6], spq=v[6:15].reshape(3, 3), spp=v[15], sqq=v[16], sdd=v[17]))
    want = gs.compose_model_transform(delta, gs.model_transform_pod())
    got_c = np.array(list(pod.pos) + list(pod.rot) + list(pod.scale), f32)
    want_c = np.array(list(want.pos) + list(want.rot) + list(want.scale), f32)
    steps = _adjacent(got_c, want_c)
    print("align_to: %d of 10 pod components differ from the fit of the restatement's sums (by one binary32 step)" % int((steps > 0).sum()))
    assert (steps <= 1).all(), (got_c, want_c)
    assert rms1 == pytest.approx(rms, rel=1e-12)
    # under the pod the queries lie on their mates
    pw = neighbors_np.positions(before_q, pos=tuple(pod.pos), rot=tuple(pod.rot), scale=tuple(pod.scale))
    assert np.abs(pw.astype(np.float64) - target[mate]).max() < 1e-4
    # nothing was edited
    assert np.array_equal(buffer_rows(qb, stream), before_q) and np.array_equal(buffer_rows(tb, stream), before_t)
    # a subsample of the queries and of the target still aligns
    rng = np.random.default_rng(2)
    q_mask = rng.random(len(query)) < 0.5
    qsel = selection_from_mask(gs, device, stream, q_mask)
    pod2, report2 = qb.align_to(stream, tb, radius, queries=qsel, max_iterations=5)
    assert report2.iterations[0][0] == q_mask.sum() and report2.stopped == "converged"
    assert np.allclose(list(pod2.pos), list(pod.pos), atol=1e-4) and np.allclose(list(pod2.rot), list(pod.rot), atol=1e-5)
    # one iteration allowed: it measures and stops at the cap, the pod is the one it was given
    pod3, report3 = qb.align_to(stream, tb, radius, max_iterations=1)
    assert report3.stopped == "iterations" and len(report3.iterations) == 1 and bytes(pod3) == bytes(gs.model_transform_pod())
    qsel.destroy(); qb.destroy(); tb.destroy()
