"""Neighbour counts and select by neighbourhood on the device against the brute-force numpy restatement
of tests/neighbors_np.py: counts and selection words as integers.  The count is defined without a grid, so the restatement
has none; the lattice and the far outlier are the inputs a grid gets wrong."""
import ctypes as C

import numpy as np
import pytest

import neighbors_np
import stats_np
from records import SELECT_OPS, buffer_rows, edited_pods, np_op, sample_edit, selection_from_mask
from scenes import ALL_LAYOUTS, FOUR_LAYOUTS, N, history_masks, pod_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
UMAX = 0xFFFFFFFF
# rotation + translation + non-uniform scale
Q = np.array([0.3, -0.5, 0.2, 0.7])
MT = dict(pos=(0.5, -0.25, 1.5), rot=tuple((Q / np.linalg.norm(Q)).astype(f32)), scale=(1.25, 0.75, 2.0))

_REF = {}


def _kth_distance(pw, k):
    """median over the points of the distance to the k-th nearest other point (binary64; only used to PICK radii)"""
    q = pw[np.isfinite(pw).all(axis=1)].astype(np.float64)
    out = []
    for a in range(0, len(q), 512):
        d2 = ((q[a:a + 512, None, :] - q[None, :, :]) ** 2).sum(axis=2)
        out.append(np.sqrt(np.partition(d2, k, axis=1)[:, k]))        # column 0 is the point itself
    return float(np.median(np.concatenate(out)))


def _scene_ref(gs):
    """pw of the N-scene under MT, three radii (median count 0, about 8, more than half of n) and the restatement's counts
    for each; computed once, never written to"""
    if not _REF:
        pw = neighbors_np.positions(pod_rows(gs, 3, 0), **MT)
        radii = [0.5 * _kth_distance(pw, 1), _kth_distance(pw, 8), _kth_distance(pw, (6 * N) // 10)]
        counts = [neighbors_np.counts(pw, r) for r in radii]
        med = [float(np.median(c[neighbors_np.points(pw)])) for c in counts]
        assert med[0] == 0 and 4 <= med[1] <= 16 and med[2] > N / 2, med
        for a in [pw] + counts:
            a.setflags(write=False)
        _REF.update(pw=pw, radii=radii, counts=counts)
    return _REF


def _plane(buf, stream, r, cap=UMAX, among=None, mt=None):
    out = buf.neighbor_counts(stream, r, cap, among, mt)
    got = np.asarray(out.download(stream, np.uint32))[:buf.len()].copy()
    out.release()
    return got


def _buffer_at(gs, device, positions):
    """a (no SH, rot + scale) buffer with the given positions"""
    import synth
    g = synth.scene(len(positions), first=3)
    g["pos"] = np.asarray(positions, f32)
    pod = gs.GaussianPod(3, 0)
    rows = np.asarray(pod.from_gaussian(g)).reshape(len(positions), pod.size)
    return gs.GaussiansBuffer.new_with_pods(device, pod, rows), rows


# ------------------------------------------------------------------------------------------------
# 1. every layout, three radii, cap above and below the largest count
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", ALL_LAYOUTS)
def test_counts_equal_the_restatement(gs, device, stream, sh, cov):
    ref = _scene_ref(gs)
    rows = pod_rows(gs, sh, cov)
    assert np.array_equal(neighbors_np.positions(rows, **MT).view(np.uint32), ref["pw"].view(np.uint32))
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    mt = gs.model_transform_pod(**MT)
    for r, want in zip(ref["radii"], ref["counts"]):
        cmax = int(want.max())
        for cap in (UMAX, cmax + 1, max(1, cmax // 2), 1):
            got = _plane(buf, stream, r, cap, None, mt)
            assert got.dtype == np.uint32 and np.array_equal(got, neighbors_np.capped(want, cap)), (r, cap)
    assert not got[5:8].any()                     # the planted NaN / inf rows
    assert np.array_equal(buffer_rows(buf, stream), rows)
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 2. small buffers
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1025])
def test_small_buffers(gs, device, stream, n):
    sh, cov = 1, 2
    pod = gs.GaussianPod(sh, cov)
    rows = pod_rows(gs, sh, cov, n) if n else np.zeros((0, pod.size), np.uint8)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, rows)
    pw = neighbors_np.positions(rows) if n else np.zeros((0, 3), f32)
    r = 2.0 * _kth_distance(pw, 1) if n > 12 else 1.0
    want = neighbors_np.counts(pw, r)
    assert np.array_equal(_plane(buf, stream, r), want.astype(np.uint32))
    assert np.array_equal(_plane(buf, stream, r, 2), neighbors_np.capped(want, 2))
    sel = gs.Selection(device, n)
    sel.fill(stream)
    sel.select_neighbors(stream, buf, r, 1, UMAX)
    assert np.array_equal(sel.download_words(stream), stats_np.pack_bits(want >= 1))
    if n > 12:
        assert want.max() >= 1 and (want == 0).any()
    sel.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 3. a lattice of spacing exactly r: every neighbour sits on a cell boundary
# ------------------------------------------------------------------------------------------------

def _lattice():
    k = np.arange(9, dtype=f32) * f32(0.25)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)


def test_lattice_of_spacing_r(gs, device, stream):
    p = _lattice()
    rng = np.random.default_rng(8)
    p = p[rng.permutation(len(p))]
    interior = ((p > 0) & (p < 2)).all(axis=1)
    r = 0.25
    below = float(np.nextafter(f32(r), f32(0)))
    buf, rows = _buffer_at(gs, device, p)
    got = _plane(buf, stream, r)
    assert np.array_equal(got, neighbors_np.counts(p, r).astype(np.uint32))
    assert interior.sum() == 343 and (got[interior] == 6).all() and got.min() == 3 and got.max() == 6
    assert not _plane(buf, stream, below).any()
    assert not neighbors_np.counts(p, below).any()
    # the lattice against another grid origin: moved by the model transform, and moved in the data
    mt = gs.model_transform_pod(pos=(0.1, 0.1, 0.1))
    pw = neighbors_np.positions(rows, pos=(0.1, 0.1, 0.1))
    for rr in (r, below, float(np.nextafter(f32(r), f32(1)))):
        assert np.array_equal(_plane(buf, stream, rr, UMAX, None, mt), neighbors_np.counts(pw, rr).astype(np.uint32)), rr
    buf.destroy()
    for off in ((0.1, 0.1, 0.1), (-0.3, 0.7, 1e-3), (100.1, -33.3, 7.7)):
        q = p + np.asarray(off, f32)
        buf, _ = _buffer_at(gs, device, q)
        want = neighbors_np.counts(q, r)
        assert np.array_equal(_plane(buf, stream, r), want.astype(np.uint32)), off
        assert want.max() >= 1
        buf.destroy()


# ------------------------------------------------------------------------------------------------
# 4. a far outlier changes nobody's count
# ------------------------------------------------------------------------------------------------

def test_far_outlier(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 3, 0
    rows = pod_rows(gs, sh, cov)
    far = rows[11:12].copy()
    far[0, :12] = np.array([1e6, 1e6, 1e6], f32).view(np.uint8)
    mt = gs.model_transform_pod(**MT)
    for extra in (far, np.concatenate([far, far])):
        buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), np.concatenate([rows, extra]))
        for r, want in zip(ref["radii"][:2], ref["counts"][:2]):
            got = _plane(buf, stream, r, UMAX, None, mt)
            assert np.array_equal(got[:N], want.astype(np.uint32)), r
            assert (got[N:] == len(extra) - 1).all()            # two outliers at one place see each other
        buf.destroy()


# ------------------------------------------------------------------------------------------------
# 5. duplicates
# ------------------------------------------------------------------------------------------------

def test_duplicates(gs, device, stream):
    one = np.tile(np.array([[0.3, -1.7, 2.9]], f32), (300, 1))
    buf, _ = _buffer_at(gs, device, one)
    assert (_plane(buf, stream, 0.0) == 299).all()
    assert (_plane(buf, stream, 0.0, 16) == 16).all()
    assert (_plane(buf, stream, 1.0, 298) == 298).all()
    buf.destroy()
    rng = np.random.default_rng(12)
    p = rng.uniform(-2, 2, (1000, 3)).astype(f32)
    dup = rng.permutation(1000)[:90]
    p[dup[30:60]] = p[dup[:30]]              # 30 pairs
    p[dup[60:]] = p[dup[0]]                  # and a group of 32
    p[dup[3], 2] = -p[dup[3], 2] * 0         # +0 and -0 are the same place
    p[dup[33], 2] = 0.0
    buf, _ = _buffer_at(gs, device, p)
    want = neighbors_np.counts(p, 0.0)
    assert (want > 0).sum() == 90 and want.max() == 31
    assert np.array_equal(_plane(buf, stream, 0.0), want.astype(np.uint32))
    sel = gs.Selection(device, 1000)
    sel.select_neighbors(stream, buf, 0.0, min_count=1)
    assert np.array_equal(sel.download_words(stream), stats_np.pack_bits(want > 0))
    sel.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 6. Gaussians that are no points
# ------------------------------------------------------------------------------------------------

def test_non_points(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 0, 0
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    r = ref["radii"][1]
    out = gs.Selection(device, N)
    for name, mask in history_masks():
        among = selection_from_mask(gs, device, stream, mask)
        pt = neighbors_np.points(ref["pw"], mask)
        want = neighbors_np.counts(ref["pw"], r, mask)
        got = _plane(buf, stream, r, UMAX, among, mt)
        assert np.array_equal(got, want.astype(np.uint32)), name
        assert not got[~pt].any() and not pt[5:8].any()
        out.fill(stream)
        out.select_neighbors(stream, buf, r, 0, UMAX, among, mt)
        assert np.array_equal(out.download_words(stream), stats_np.pack_bits(pt)), name
        if among is not None:
            among.destroy()
    # nobody's neighbour: the counts among a subset are those of the subset alone
    mask = history_masks()[0][1]
    sub = ref["pw"][mask]
    assert np.array_equal(neighbors_np.counts(ref["pw"], r, mask)[mask], neighbors_np.counts(sub, r))
    out.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 7. select_neighbors: the five ops, the tail, the ends of the count range
# ------------------------------------------------------------------------------------------------

def test_select_ops(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 2, 1
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    r, c = ref["radii"][1], ref["counts"][1]
    pt = neighbors_np.points(ref["pw"])
    prior = np.random.default_rng(7).random(N) < 0.5
    sel = gs.Selection(device, N)
    for op in SELECT_OPS:
        for lo, hi in ((0, 3), (4, 12), (9, UMAX), (0, UMAX), (0, 0), (5, 4), (UMAX, UMAX)):
            sel.upload(stream, prior)
            sel.select_neighbors(stream, buf, r, lo, hi, None, mt, op)
            want = np_op(prior, neighbors_np.in_count_range(c, pt, lo, hi), op)
            assert np.array_equal(sel.download_words(stream), stats_np.pack_bits(want)), (op, lo, hi)
    assert 0 < neighbors_np.in_count_range(c, pt, 0, 3).sum() < N and neighbors_np.in_count_range(c, pt, 9, UMAX).any()
    sel.destroy(); buf.destroy()


@pytest.mark.parametrize("op", SELECT_OPS)
def test_select_keeps_the_tail_clear(gs, device, stream, op):
    n = 65
    sh, cov = 0, 0
    rows = pod_rows(gs, sh, cov, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    pw = neighbors_np.positions(rows)
    r = 2.0 * _kth_distance(pw, 1)
    c, pt = neighbors_np.counts(pw, r), neighbors_np.points(pw)
    sel = gs.Selection(device, n)
    sel.fill(stream)
    sel.select_neighbors(stream, buf, r, 0, UMAX, op=op)
    words = sel.download_words(stream)
    assert len(words) == 3 and words[2] >> 1 == 0
    assert np.array_equal(words, stats_np.pack_bits(np_op(np.ones(n, bool), pt, op)))
    sel.fill(stream)
    sel.select_neighbors(stream, buf, r, 1, 0, op=op)                   # min_count > max_count: T is empty
    assert np.array_equal(sel.download_words(stream), stats_np.pack_bits(np_op(np.ones(n, bool), np.zeros(n, bool), op)))
    sel.clear(stream)
    sel.select_neighbors(stream, buf, r, 1, UMAX, op=op)
    assert np.array_equal(sel.download_words(stream), stats_np.pack_bits(np_op(np.zeros(n, bool), pt & (c >= 1), op)))
    assert sel.count(stream) <= n
    sel.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 8. the cleanup workflow: delete the floaters
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_delete_the_floaters(gs, device, stream, sh, cov):
    ref = _scene_ref(gs)
    rows = pod_rows(gs, sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    mt = gs.model_transform_pod(**MT)
    k = 4
    isolated = neighbors_np.in_count_range(ref["counts"][1], neighbors_np.points(ref["pw"]), 0, k - 1)
    assert 0 < isolated.sum() < N
    sel = gs.Selection(device, N)
    sel.select_neighbors(stream, buf, ref["radii"][1], max_count=k - 1, model_transform=mt)
    assert sel.count(stream) == int(isolated.sum())
    kept = buf.extract(stream, sel, invert=True)
    assert kept.len() == N - int(isolated.sum())
    assert np.array_equal(buffer_rows(kept, stream), rows[~isolated])
    assert np.array_equal(buffer_rows(buf, stream), rows)
    kept.destroy(); sel.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 9. ordering behind an edit on another stream
# ------------------------------------------------------------------------------------------------

def test_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    orig = pod_rows(gs, sh, cov)
    mask = np.random.default_rng(4).random(N) < 0.3
    s1, s2 = stream, device.create_stream()
    sel, out = selection_from_mask(gs, device, s1, mask), gs.Selection(device, N)
    s1.synchronize()
    edited = edited_pods(gs, sh, cov, orig.reshape(-1), mask, 15).reshape(N, pod.size)
    pw, before = neighbors_np.positions(edited), neighbors_np.positions(orig)
    r = _kth_distance(before, 8)
    c, c0 = neighbors_np.counts(pw, r), neighbors_np.counts(before, r)
    assert not np.array_equal(c, c0), "the edit changes the counts"
    for what in ("counts", "select"):
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
        buf.edit(s1, sel, sample_edit(gs, 15))
        # on stream 2 right behind the edit on stream 1, no host synchronisation in between
        if what == "counts":
            assert np.array_equal(_plane(buf, s2, r), c.astype(np.uint32))
        else:
            out.select_neighbors(s2, buf, r, 0, 3)
            assert np.array_equal(out.download_words(s2), stats_np.pack_bits(neighbors_np.in_count_range(c, neighbors_np.points(pw), 0, 3)))
        s1.synchronize()
        assert np.array_equal(buffer_rows(buf, s1), edited)
        buf.destroy()
    s2.synchronize()
    sel.destroy(); out.destroy()
    s2.close()


# ------------------------------------------------------------------------------------------------
# 10. two runs, one result; a caller's plane; a second stream reuses the scratch
# ------------------------------------------------------------------------------------------------

def test_runs_are_identical(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 1, 2
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    s2 = device.create_stream()
    for r, want in zip(ref["radii"], ref["counts"]):
        a = _plane(buf, stream, r, 7, None, mt)
        b = _plane(buf, s2, r, 7, None, mt)
        assert np.array_equal(a, b) and np.array_equal(a, neighbors_np.capped(want, 7))
    # into the caller's plane, larger than needed: the bytes behind 4 n stay
    plane = gs.Buffer(device, data=np.full(N + 3, 0x5A5A5A5A, np.uint32))
    assert buf.neighbor_counts(stream, ref["radii"][1], 16, None, mt, out=plane) is plane
    got = np.asarray(plane.download(stream, np.uint32))
    assert np.array_equal(got[:N], neighbors_np.capped(ref["counts"][1], 16)) and (got[N:] == 0x5A5A5A5A).all()
    plane.release()
    s2.synchronize()
    s2.close()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 11. argument errors
# ------------------------------------------------------------------------------------------------

def test_argument_errors_change_nothing(gs, device, stream):
    sh, cov = 0, 0
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mask = np.random.default_rng(9).random(N) < 0.3
    sel, short = selection_from_mask(gs, device, stream, mask), gs.Selection(device, N - 1)
    other = gs.Device(0)          # a second device object: its objects belong to another device
    foreign, foreign_plane = gs.Selection(other, N), gs.Buffer(other, size=4 * N)
    words = sel.download_words(stream)
    fill = np.full(N, 0x5A5A5A5A, np.uint32)
    plane, small = gs.Buffer(device, data=fill), gs.Buffer(device, size=4 * N - 4)
    L, bad = gs._L, gs.InvalidArgumentError.code
    mt = C.byref(gs.model_transform_pod(**MT))
    nan, inf = float("nan"), float("inf")

    def counts(g=buf._h, among=sel._h, r=0.5, cap=16, out=plane._h):
        return L.gs_gaussians_buffer_neighbor_counts(g, stream._h, among, mt, r, cap, out)

    assert counts(g=None) == bad and counts(out=None) == bad
    for r in (-1.0, nan, inf, -inf, 1e20):
        assert counts(r=r) == bad, r
    assert counts(cap=0) == bad
    assert counts(out=small._h) == bad and counts(out=foreign_plane._h) == bad
    assert counts(among=short._h) == bad and counts(among=foreign._h) == bad
    assert np.array_equal(np.asarray(plane.download(stream, np.uint32)), fill)

    def select(s=sel._h, g=buf._h, among=None, r=0.5, lo=0, hi=3, op=0):
        return L.gs_select_neighbors(s, stream._h, g, among, mt, r, lo, hi, op)

    assert select(s=None) == bad and select(g=None) == bad
    assert select(op=5) == bad and select(op=-1) == bad
    for r in (-1.0, nan, inf, -inf, 1e20):
        assert select(r=r) == bad, r
    assert select(s=short._h) == bad and select(s=foreign._h) == bad
    assert select(among=short._h) == bad and select(among=foreign._h) == bad
    assert np.array_equal(sel.download_words(stream), words)
    # and the valid calls next to them
    assert counts(r=0.0, cap=1) == 0 and select(r=0.0, lo=0, hi=0, op=1) == 0
    stream.synchronize()
    for o in (sel, short, foreign):
        o.destroy()
    for o in (plane, small, foreign_plane):
        o.release()
    buf.destroy()
