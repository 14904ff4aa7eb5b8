"""Attribute statistics, histograms and select by attribute range on the device against the numpy
restatement of tests/stats_np.py: counts, finite counts, min and max bit for bit, sums inside the first-order bound of a
binary64 summation, histograms and selection words as integers, the ordering behind an edit on another stream, the
cleanup workflow, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import edit_np
import stats_np
from records import SELECT_OPS, buffer_rows, edited_pods, np_op, sample_edit, selection_from_mask
from scenes import ALL_LAYOUTS, FOUR_LAYOUTS, N, history_masks, pod_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
# rotation + translation + non-uniform scale
Q = np.array([0.3, -0.5, 0.2, 0.7])
MT = dict(pos=(0.5, -0.25, 1.5), rot=tuple((Q / np.linalg.norm(Q)).astype(f32)), scale=(1.25, 0.75, 2.0))
REF = (0.25, -0.5, -3.0)
SMALL = [0, 1, 63, 64, 65, 1025]

_VALUES = {}


def _values(gs, sh, cov, n=N, seed=3, rows=None):
    """the nine attributes of the records of pod_rows(...) under MT / REF; computed once per layout and length"""
    key = (sh, cov, n, seed)
    if rows is not None:
        return stats_np.attributes(sh, cov, rows, ref=REF, **MT)
    if key not in _VALUES:
        v = stats_np.attributes(sh, cov, pod_rows(gs, sh, cov, n, seed), ref=REF, **MT) if n else np.zeros((0, 9), f32)
        v.setflags(write=False)
        _VALUES[key] = v
    return _VALUES[key]


def _rows_of(gs, sh, cov, n):
    return pod_rows(gs, sh, cov, n) if n else np.zeros((0, gs.GaussianPod(sh, cov).size), np.uint8)


def _check_stats(got, want, tag):
    assert got.count == want["count"], tag
    assert np.array_equal(got.finite, want["finite"]), (tag, got.finite, want["finite"])
    assert got.min.dtype == f32 and got.max.dtype == f32 and got.sum.dtype == np.float64
    assert np.array_equal(got.min.view(np.uint32), want["min"].view(np.uint32)), (tag, got.min, want["min"])
    assert np.array_equal(got.max.view(np.uint32), want["max"].view(np.uint32)), (tag, got.max, want["max"])
    # first-order bound of any summation order in binary64, doubled: finite 2^-52 sum |v|
    bound = want["finite"].astype(np.float64) * 2.0 ** -52 * want["abs_sum"]
    err = np.abs(got.sum - want["sum"])
    assert (err <= bound).all(), (tag, err, bound)


BINS = (1, 7, 256, 4096)


def _raw_top(vmax, lo, hi, bins):
    """(max - lo) scale in binary32, before the truncation"""
    return (f32(vmax) - f32(lo)) * (f32(bins) / (f32(hi) - f32(lo)))


def _ranges(v):
    """(lo, hi) pairs of one attribute: the whole finite data with hi one step above the maximum (the top clamp), and a
    range strictly inside the data (below and above are not empty)"""
    fin = np.sort(v[np.isfinite(v)])
    hi = np.nextafter(fin[-1], f32(np.inf), dtype=f32)
    # The clamp to bins - 1 is reached when (max - lo) scale rounds up to bins, which needs hi - lo and max - lo to round to
    # the same binary32: lo is moved down (by the restatement's arithmetic alone) until the step above the maximum is lost.
    top = (fin[0], hi)
    for d in (0.0, 1.0, 10.0, 100.0, 1000.0, 1e4, 1e5):
        lo = f32(fin[0] - f32(d))
        if any(_raw_top(fin[-1], lo, hi, bins) >= bins for bins in BINS):
            top = (lo, hi)
            break
    inner = (fin[len(fin) // 4], fin[(3 * len(fin)) // 4])
    assert inner[1] > inner[0] and fin[0] < inner[0] and inner[1] < fin[-1]
    return [top, inner]


# ------------------------------------------------------------------------------------------------
# 1. statistics
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", ALL_LAYOUTS)
def test_stats_equal_the_restatement(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    assert pod.size == edit_np.pod_bytes(sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    vals = _values(gs, sh, cov)
    assert not np.isfinite(vals[5:8, :3]).any(), "the planted NaN and inf rows reach the attributes"
    for name, mask in history_masks():
        sel = selection_from_mask(gs, device, stream, mask)
        got = buf.stats(stream, sel, mt, REF)
        _check_stats(got, stats_np.stats(vals, mask), (sh, cov, name))
        again = buf.stats(stream, sel, mt, REF)
        assert np.array_equal(got.sum.view(np.uint64), again.sum.view(np.uint64)), (name, "the sum is the same bits from run to run")
        if sel is not None:
            sel.destroy()
    # the default transform and the origin as reference, through the same arithmetic
    plain = stats_np.attributes(sh, cov, pod_rows(gs, sh, cov))
    _check_stats(buf.stats(stream), stats_np.stats(plain), (sh, cov, "defaults"))
    st = buf.stats(stream, None, mt, REF)
    want = stats_np.stats(vals)
    assert np.allclose(st.centroid, want["sum"][:3] / want["finite"][:3], rtol=1e-12, atol=0)
    assert np.array_equal(st.bounds[0], want["min"][:3]) and np.array_equal(st.bounds[1], want["max"][:3])
    buf.destroy()


@pytest.mark.parametrize("n", SMALL)
def test_small_buffers(gs, device, stream, n):
    """stats, one histogram and one range select at the lengths around a wave and a 1024-block"""
    mt = gs.model_transform_pod(**MT)
    for sh, cov in [(0, 0), (2, 2)]:
        pod = gs.GaussianPod(sh, cov)
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, _rows_of(gs, sh, cov, n))
        assert buf.len() == n
        vals = _values(gs, sh, cov, n)
        mask = np.random.default_rng(n).random(n) < 0.5
        sel = selection_from_mask(gs, device, stream, mask)
        for s, m in ((None, None), (sel, mask)):
            _check_stats(buf.stats(stream, s, mt, REF), stats_np.stats(vals, m), (sh, cov, n, m is not None))
            for attr in (stats_np.Y, stats_np.GREEN, stats_np.SIZE2, stats_np.DIST2):
                got = buf.histogram(stream, attr, -1.0, 7.0, 7, s, mt, REF)
                assert got.shape == (2, 10) and got.dtype == np.uint64
                assert np.array_equal(got, stats_np.histogram(vals[:, attr], -1.0, 7.0, 7, m)), (sh, cov, n, attr)
        if n == 0:
            st = buf.stats(stream)
            assert st.count == 0 and not st.finite.any() and not st.sum.any()
            assert np.isposinf(st.min).all() and np.isneginf(st.max).all()
        for attr in (stats_np.X, stats_np.OPACITY, stats_np.SIZE2):
            for op in SELECT_OPS:
                sel.upload(stream, mask)
                sel.select_attribute(stream, buf, attr, 0.25, 2.0, op, mt, REF)
                want = stats_np.pack_bits(np_op(mask, stats_np.in_range(vals[:, attr], 0.25, 2.0), op))
                assert np.array_equal(sel.download_words(stream), want), (sh, cov, n, attr, op)
        sel.destroy()
        buf.destroy()


# ------------------------------------------------------------------------------------------------
# 2. histograms
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_histograms_equal_the_restatement(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    vals = _values(gs, sh, cov)
    mask = history_masks()[0][1]
    sel = selection_from_mask(gs, device, stream, mask)
    count = int(mask.sum())
    clamped = 0
    for attr in range(stats_np.ATTR_COUNT):
        v = vals[:, attr]
        for k, (lo, hi) in enumerate(_ranges(v)):
            for bins in BINS:
                got = buf.histogram(stream, attr, lo, hi, bins, sel, mt, REF)
                want = stats_np.histogram(v, lo, hi, bins, mask)
                assert got.shape == (2, bins + 3)
                assert np.array_equal(got, want), (attr, lo, hi, bins, np.flatnonzero((got != want).any(axis=0))[:8])
                assert int(got[0].sum()) == count and int(got[1].sum()) == N - count
                if k == 0:
                    assert got[:, bins].sum() == int(np.isneginf(v).sum()) and got[:, bins + 1].sum() == int(np.isposinf(v).sum())
                    with np.errstate(all="ignore"):
                        raw = (v[np.isfinite(v)] - f32(lo)) * (f32(bins) / (f32(hi) - f32(lo)))
                    clamped += int((raw >= bins).sum())
                else:
                    assert got[:, bins].sum() > 0 and got[:, bins + 1].sum() > 0
                assert got[:, bins + 2].sum() == int(np.isnan(v).sum())
        # no selection: everything in row 0
        lo, hi = _ranges(v)[1]
        got = buf.histogram(stream, attr, lo, hi, 256, None, mt, REF)
        assert np.array_equal(got, stats_np.histogram(v, lo, hi, 256)) and not got[1].any() and int(got[0].sum()) == N
    assert clamped > 0, "no value reached the clamp to bins - 1"
    sel.destroy()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 3. select by range
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", ALL_LAYOUTS)
def test_select_attribute_equals_the_restatement(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    vals = _values(gs, sh, cov)
    pre = np.random.default_rng(7).random(N) < 0.4
    sel = gs.Selection(device, N)
    tail = np.uint32((1 << (N & 31)) - 1)
    for attr in range(stats_np.ATTR_COUNT):
        v = vals[:, attr]
        lo, hi = _ranges(v)[1]
        hit = stats_np.in_range(v, lo, hi)
        assert 0 < hit.sum() < N
        for op in SELECT_OPS:
            sel.upload(stream, pre)
            sel.select_attribute(stream, buf, attr, lo, hi, op, mt, REF)
            got = sel.download_words(stream)
            assert np.array_equal(got, stats_np.pack_bits(np_op(pre, hit, op))), (attr, op)
            assert got[-1] & ~tail == 0
        # lo > hi selects nothing; -inf .. +inf selects every value that is not NaN
        sel.upload(stream, pre)
        sel.select_attribute(stream, buf, attr, hi, lo, "set", mt, REF)
        assert not sel.download_words(stream).any()
        sel.upload(stream, pre)
        sel.select_attribute(stream, buf, attr, -np.inf, np.inf, "set", mt, REF)
        got = sel.download_words(stream)
        assert np.array_equal(got, stats_np.pack_bits(~np.isnan(v))) and got[-1] & ~tail == 0
        sel.select_attribute(stream, buf, attr, -np.inf, np.inf, "xor", mt, REF)
        assert not sel.download_words(stream).any()
    sel.destroy()
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 4. DIST2 is the sphere
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_dist2_range_is_select_sphere(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    a, b = gs.Selection(device, N), gs.Selection(device, N)
    pre = np.random.default_rng(8).random(N) < 0.5
    for r in (f32(0.0), f32(4.0), f32(20.0), f32(40.5), f32(1e6)):
        for op in SELECT_OPS:
            a.upload(stream, pre)
            b.upload(stream, pre)
            a.select_sphere(stream, buf, mt, REF, float(r), op)
            b.select_attribute(stream, buf, gs.ATTR_DIST2, 0.0, float(r * r), op, mt, REF)
            wa, wb = a.download_words(stream), b.download_words(stream)
            assert np.array_equal(wa, wb), (float(r), op)
        a.select_sphere(stream, buf, mt, REF, float(r))
        if r == f32(20.0):
            assert 0 < a.count(stream) < N
    a.destroy(); b.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 5. ordering behind an edit on another stream
# ------------------------------------------------------------------------------------------------

def test_passes_are_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    orig = pod_rows(gs, sh, cov)
    mask = np.random.default_rng(4).random(N) < 0.3
    s1, s2 = stream, device.create_stream()
    mt = gs.model_transform_pod(**MT)
    sel, out = selection_from_mask(gs, device, s1, mask), gs.Selection(device, N)
    s1.synchronize()
    edited = edited_pods(gs, sh, cov, orig.reshape(-1), mask, 15).reshape(N, pod.size)
    vals = _values(gs, sh, cov, rows=edited)
    before = _values(gs, sh, cov)
    assert (vals[mask][:, [0, 3, 6, 7]] != before[mask][:, [0, 3, 6, 7]]).any(axis=0).all(), "the edit changes the attributes"
    # each pass on stream 2 right behind the edit on stream 1, no host synchronisation in between
    for what in ("stats", "histogram", "select"):
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
        buf.edit(s1, sel, sample_edit(gs, 15))
        if what == "stats":
            _check_stats(buf.stats(s2, sel, mt, REF), stats_np.stats(vals, mask), what)
        elif what == "histogram":
            got = buf.histogram(s2, gs.ATTR_OPACITY, 0.0, 1.0, 256, sel, mt, REF)
            assert np.array_equal(got, stats_np.histogram(vals[:, stats_np.OPACITY], 0.0, 1.0, 256, mask))
            assert not np.array_equal(got, stats_np.histogram(before[:, stats_np.OPACITY], 0.0, 1.0, 256, mask))
        else:
            out.select_attribute(s2, buf, gs.ATTR_X, -1.0, 1.0, "set", mt, REF)
            got = out.download_words(s2)
            assert np.array_equal(got, stats_np.pack_bits(stats_np.in_range(vals[:, stats_np.X], -1.0, 1.0)))
            assert not np.array_equal(got, stats_np.pack_bits(stats_np.in_range(before[:, stats_np.X], -1.0, 1.0)))
        s1.synchronize()
        assert np.array_equal(buffer_rows(buf, s1), edited)
        buf.destroy()
    s2.synchronize()
    sel.destroy(); out.destroy()
    s2.close()


# ------------------------------------------------------------------------------------------------
# 6. the cleanup workflow
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_delete_the_faint_gaussians(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    rows = pod_rows(gs, sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, rows)
    sel = gs.Selection(device, N)
    sel.select_attribute(stream, buf, gs.ATTR_OPACITY, 0.0, 0.1)
    faint = rows[:, 15].astype(f32) / f32(255.0) <= f32(0.1)
    assert 0 < faint.sum() < N and sel.count(stream) == int(faint.sum())
    kept = buf.extract(stream, sel, invert=True)
    assert kept.len() == int((~faint).sum())
    assert np.array_equal(buffer_rows(kept, stream), rows[~faint])
    assert np.array_equal(buffer_rows(buf, stream), rows)
    kept.destroy(); sel.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 7. argument errors
# ------------------------------------------------------------------------------------------------

def test_argument_errors_change_nothing(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    rows = pod_rows(gs, sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, rows)
    mask = np.random.default_rng(9).random(N) < 0.3
    sel, short = selection_from_mask(gs, device, stream, mask), gs.Selection(device, N - 1)
    other = gs.Device(0)          # a second device object: its selections belong to another device
    foreign = gs.Selection(other, N)
    words = sel.download_words(stream)
    L, bad = gs._L, gs.InvalidArgumentError.code
    mt = gs.model_transform_pod(**MT)
    nan, inf = float("nan"), float("inf")

    def desc(attr=gs.ATTR_X, ref=(0.0, 0.0, 0.0), reserved=(0, 0)):
        d = gs._capi.AttributeDesc()
        d.attr = attr
        d.ref[:] = ref
        d.reserved[:] = reserved
        return d

    ok = desc()
    bad_descs = [desc(attr=9), desc(attr=0xFFFFFFFF), desc(reserved=(0, 1)), desc(reserved=(3, 0)),
                 desc(attr=gs.ATTR_DIST2, ref=(0.0, nan, 0.0)), desc(attr=gs.ATTR_DIST2, ref=(inf, 0.0, 0.0))]

    # statistics: *out untouched
    out = gs._capi.Stats()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    before = bytes(out)
    ref3 = lambda *v: (C.c_float * 3)(*v)
    for args in [(None, stream._h, sel._h, C.byref(mt), ref3(0, 0, 0), C.byref(out)),
                 (buf._h, stream._h, sel._h, C.byref(mt), ref3(0, 0, 0), None),
                 (buf._h, stream._h, sel._h, C.byref(mt), ref3(0, nan, 0), C.byref(out)),
                 (buf._h, stream._h, sel._h, C.byref(mt), ref3(-inf, 0, 0), C.byref(out)),
                 (buf._h, stream._h, short._h, C.byref(mt), ref3(0, 0, 0), C.byref(out)),
                 (buf._h, stream._h, foreign._h, C.byref(mt), ref3(0, 0, 0), C.byref(out))]:
        assert L.gs_gaussians_buffer_stats(*args) == bad, args
        assert bytes(out) == before

    # histogram: counts_out untouched
    bins = 16
    counts = np.full(2 * (bins + 3), 0x5A5A, np.uint64)
    hist = lambda g=buf._h, s=sel._h, d=ok, lo=0.0, hi=1.0, b=bins, c=counts: L.gs_gaussians_buffer_histogram(
        g, stream._h, s, C.byref(d) if d is not None else None, lo, hi, b, gs._ptr(c) if c is not None else None)
    assert hist(g=None) == bad and hist(d=None) == bad and hist(c=None) == bad
    for d in bad_descs:
        assert hist(d=d) == bad, (d.attr, list(d.ref), list(d.reserved))
    assert hist(s=short._h) == bad and hist(s=foreign._h) == bad
    assert hist(b=0) == bad and hist(b=4097) == bad
    big = np.zeros(2 * 4100, np.uint64)
    assert hist(b=4097, c=big) == bad and not big.any()
    for lo, hi in [(nan, 1.0), (0.0, nan), (-inf, 1.0), (0.0, inf), (1.0, 1.0), (1.0, 0.0), (-3e38, 3e38), (0.0, 1e-45)]:
        assert hist(lo=lo, hi=hi) == bad, (lo, hi)
    assert (counts == 0x5A5A).all() and not big.any()
    assert hist() == 0
    assert int(counts[:bins + 3].sum()) == int(mask.sum()) and int(counts.sum()) == N

    # select: the selection unchanged, word for word
    select = lambda sl=sel._h, st=stream._h, g=buf._h, d=ok, lo=0.0, hi=1.0, op=0: L.gs_select_attribute(
        sl, st, g, C.byref(d) if d is not None else None, lo, hi, op)
    assert select(sl=None) == bad and select(st=None) == bad and select(g=None) == bad and select(d=None) == bad
    for d in bad_descs:
        assert select(d=d) == bad, (d.attr, list(d.ref), list(d.reserved))
    assert select(lo=nan) == bad and select(hi=nan) == bad and select(op=5) == bad
    assert select(sl=short._h) == bad and select(sl=foreign._h) == bad
    assert np.array_equal(sel.download_words(stream), words)
    assert not short.download_words(stream).any()
    assert np.array_equal(buffer_rows(buf, stream), rows)
    # the Python layer raises the library's error for what only the library can know
    with pytest.raises(gs.InvalidArgumentError):
        buf.stats(stream, short)
    with pytest.raises(gs.InvalidArgumentError):
        buf.histogram(stream, gs.ATTR_X, 1.0, 0.0, 8)
    with pytest.raises(gs.InvalidArgumentError):
        short.select_attribute(stream, buf, gs.ATTR_X, 0.0, 1.0)
    for o in (foreign, short, sel, buf):
        o.destroy()
    other.close()
