"""Snapshots of the selected records, their restore and exchange, concatenation and range select.
No oracle: a snapshot, a restore and a concatenation move bytes, so every expectation is numpy indexing on the arrays the
test uploaded itself, and every comparison is on bytes (frames: on the bits of the floats)."""
import numpy as np
import pytest

from records import buffer_rows, np_op, sample_edit, selection_from_mask
from scenes import ALL_LAYOUTS, FOUR_LAYOUTS, N, history_masks, pod_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
ALL_FLAGS = 15


# ------------------------------------------------------------------------------------------------
# 1. restore gives the bytes back
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", ALL_LAYOUTS)
def test_restore_gives_the_bytes_back(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    orig = pod_rows(gs, sh, cov)
    for name, mask in history_masks():
        m = np.ones(N, bool) if mask is None else mask
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
        sel = selection_from_mask(gs, device, stream, mask)
        snap = buf.snapshot(stream, sel)
        assert (snap.len, snap.count) == (N, int(m.sum())), name
        buf.edit(stream, sel, sample_edit(gs, ALL_FLAGS))
        edited = buffer_rows(buf, stream)
        changed = (edited != orig).any(axis=1)
        assert changed.any() == m.any() and not changed[~m].any(), name
        if m.any():
            assert changed[m].mean() > 0.9, name          # (a NaN row may re-encode to itself)
        buf.restore(stream, snap)
        got = buffer_rows(buf, stream)
        assert np.array_equal(got, orig), (name, int((got != orig).any(axis=1).sum()))
        snap.destroy()
        if sel is not None:
            sel.destroy()
        buf.destroy()


# ------------------------------------------------------------------------------------------------
# 2. the snapshot is independent of the selection
# ------------------------------------------------------------------------------------------------

def test_snapshot_is_independent_of_the_selection(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    orig = pod_rows(gs, sh, cov)
    mask = np.random.default_rng(5).random(N) < 0.3
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
    sel = selection_from_mask(gs, device, stream, mask)
    snap = buf.snapshot(stream, sel)
    count = int(mask.sum())
    assert snap.count == count and snap.len == N
    print("snapshot of %d of %d records: %d bytes, records alone %d" % (count, N, snap.nbytes, count * pod.size))
    assert count * pod.size <= snap.nbytes <= count * pod.size + 8 * ((N + 31) // 32) + 4096
    buf.edit(stream, sel, sample_edit(gs, ALL_FLAGS))
    sel.clear(stream)                       # the snapshot has its own mask
    assert sel.count(stream) == 0
    buf.restore(stream, snap)
    assert np.array_equal(buffer_rows(buf, stream), orig)
    # the mask comes back, alone and folded into another selection
    snap.selection(stream, sel, gs.SEL_SET)
    assert np.array_equal(sel.download(stream), mask)
    other = np.random.default_rng(6).random(N) < 0.2
    sel.upload(stream, other)
    snap.selection(stream, sel, gs.SEL_OR)
    assert np.array_equal(sel.download(stream), mask | other)
    sel.upload(stream, other)
    snap.selection(stream, sel, "andnot")
    assert np.array_equal(sel.download(stream), other & ~mask)
    short = gs.Selection(device, N - 1)
    with pytest.raises(gs.InvalidArgumentError):
        snap.selection(stream, short)
    # a snapshot of everything (no selection) selects everything; an empty one, and one of an empty buffer, are valid
    whole = buf.snapshot(stream)
    whole.selection(stream, sel)
    assert whole.count == N and sel.download(stream).all() and (sel.download_words(stream)[-1] >> (N & 31)) == 0
    sel.clear(stream)
    empty = buf.snapshot(stream, sel)
    assert (empty.len, empty.count) == (N, 0) and empty.nbytes <= 8 * ((N + 31) // 32) + 4096
    buf.restore(stream, empty)
    buf.restore(stream, empty, exchange=True)
    assert np.array_equal(buffer_rows(buf, stream), orig)
    nothing = gs.GaussiansBuffer.new_empty(device, pod, 0)
    zero = nothing.snapshot(stream)
    assert (zero.len, zero.count) == (0, 0)
    nothing.restore(stream, zero)
    with pytest.raises(gs.InvalidArgumentError):
        buf.snapshot(stream, short)
    for o in (zero, nothing, empty, whole, snap, short, sel, buf):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 3. exchange is undo, then redo
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_exchange_is_undo_then_redo(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    O = pod_rows(gs, sh, cov)
    mask = np.random.default_rng(2).random(N) < 0.3
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, O)
    sel = selection_from_mask(gs, device, stream, mask)
    snap = buf.snapshot(stream, sel)
    buf.edit(stream, sel, sample_edit(gs, ALL_FLAGS))
    E = buffer_rows(buf, stream)
    assert (E != O).any(axis=1)[mask].mean() > 0.9 and np.array_equal(E[~mask], O[~mask])
    for step, want in enumerate([O, E, O]):
        buf.restore(stream, snap, exchange=True)
        got = buffer_rows(buf, stream)
        assert np.array_equal(got[~mask], O[~mask]), step
        assert np.array_equal(got, want), step
    # the snapshot now holds E: a plain restore pastes it and leaves the snapshot alone
    buf.restore(stream, snap)
    buf.restore(stream, snap)
    assert np.array_equal(buffer_rows(buf, stream), E)
    for o in (snap, sel, buf):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 4. another target
# ------------------------------------------------------------------------------------------------

def test_restore_into_another_buffer(gs, device, stream):
    sh, cov = 1, 1
    pod = gs.GaussianPod(sh, cov)
    A, B = pod_rows(gs, sh, cov), pod_rows(gs, sh, cov, seed=8)
    assert (A != B).any(axis=1).mean() > 0.9
    mask = np.random.default_rng(3).random(N) < 0.3
    a = gs.GaussiansBuffer.new_with_pods(device, pod, A)
    b = gs.GaussiansBuffer.new_with_pods(device, pod, B)
    sel = selection_from_mask(gs, device, stream, mask)
    snap = a.snapshot(stream, sel)
    b.restore(stream, snap)
    assert np.array_equal(buffer_rows(b, stream), np.where(mask[:, None], A, B))
    assert np.array_equal(buffer_rows(a, stream), A)
    # another length, another layout: refused, nothing written
    b.update_with_pod(stream, B)
    longer = gs.GaussiansBuffer.new_with_pods(device, pod, pod_rows(gs, sh, cov, n=N + 1, seed=8))
    other_pod = gs.GaussianPod(sh, 2)
    other = gs.GaussiansBuffer.new_with_pods(device, other_pod, pod_rows(gs, sh, 2, seed=8))
    for target in (longer, other):
        before = buffer_rows(target, stream)
        for exchange in (False, True):
            with pytest.raises(gs.InvalidArgumentError):
                target.restore(stream, snap, exchange=exchange)
        assert np.array_equal(buffer_rows(target, stream), before)
    assert np.array_equal(buffer_rows(b, stream), B)
    for o in (snap, sel, other, longer, b, a):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 5. frames
# ------------------------------------------------------------------------------------------------

W, H = 128, 96


def _frame(gs, device, stream, r, buf, aux=False):
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    img = gs.Buffer(device, data=np.full(H * W * 4, f32(np.nan)))
    planes = []
    kw = {}
    if aux:
        depth = gs.Buffer(device, data=np.full(H * W, f32(np.nan)))
        pick = gs.Buffer(device, data=np.full(H * W, 0xDEADBEEF, np.uint32))
        planes = [depth, pick]
        kw = dict(depth_device_ptr=depth.device_ptr(), pick_device_ptr=pick.device_ptr())
    r.render(stream, buf, gt, mt, cam, img.device_ptr(), **kw)
    stream.synchronize()
    out = [img.download(stream, np.uint32).copy()] + [p.download(stream, np.uint32).copy() for p in planes]
    for b in [img] + planes:
        b.release()
    return out


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("sh,cov,aux", [(0, 0, False), (1, 2, False), (3, 0, False), (0, 0, True)])
def test_frames_after_a_restore(gs, device, stream, sh, cov, aux):
    import synth
    n = 3001
    pod = gs.GaussianPod(sh, cov)
    pods = np.asarray(pod.from_gaussian(synth.scene(n, first=21)))
    mask = np.random.default_rng(2).random(n) < 0.3
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    sel = selection_from_mask(gs, device, stream, mask)
    r, r2 = gs.Renderer(device), gs.Renderer(device)
    A = _frame(gs, device, stream, r, buf, aux)
    snap = buf.snapshot(stream, sel)
    buf.edit(stream, sel, sample_edit(gs, gs.EDIT_TRANSFORM | gs.EDIT_ROTATE_SH))
    B = _frame(gs, device, stream, r, buf, aux)
    buf.restore(stream, snap)
    C = _frame(gs, device, stream, r, buf, aux)
    assert (A[0] != 0).any(), "the scene must reach the image"
    assert not np.array_equal(A[0], B[0]), "the edit must change the frame"
    assert _same(C, A)
    fresh = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    assert _same(C, _frame(gs, device, stream, r2, fresh, aux))
    if aux:
        assert not np.array_equal(A[2], B[2]) and (A[2] != gs.PICK_NONE).any()
    for o in (r, r2, snap, sel, fresh, buf):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 6. streams
# ------------------------------------------------------------------------------------------------

def test_restore_and_snapshot_are_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    orig = pod_rows(gs, sh, cov)
    mask = np.random.default_rng(4).random(N) < 0.3
    s1, s2 = stream, device.create_stream()
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
    sel = selection_from_mask(gs, device, s1, mask)
    s1.synchronize()
    snap = buf.snapshot(s1, sel)
    # edit on stream 1, restore on stream 2, no host synchronisation in between
    buf.edit(s1, sel, sample_edit(gs, ALL_FLAGS))
    buf.restore(s2, snap)
    assert np.array_equal(buffer_rows(buf, s2), orig)
    # a snapshot on stream 2 right behind an edit on stream 1 holds the edited records
    buf.edit(s1, sel, sample_edit(gs, ALL_FLAGS))
    late = buf.snapshot(s2, sel)
    s1.synchronize()
    edited = buffer_rows(buf, s1)
    assert (edited != orig).any(axis=1)[mask].mean() > 0.9
    fresh = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
    fresh.restore(s2, late)
    assert np.array_equal(buffer_rows(fresh, s2), edited)
    s2.synchronize()
    for o in (late, snap, sel, fresh, buf):
        o.destroy()
    s2.close()


# ------------------------------------------------------------------------------------------------
# 7. concatenation
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_concat(gs, device, stream, sh, cov):
    pod = gs.GaussianPod(sh, cov)
    lens = [N, 0, 1, 2049]
    rows = [pod_rows(gs, sh, cov, n=n, seed=10 + k) if n else np.zeros((0, pod.size), np.uint8) for k, n in enumerate(lens)]
    bufs = [gs.GaussiansBuffer.new_with_pods(device, pod, r) for r in rows]
    rng = np.random.default_rng(12)
    # sources 0, 1, 2, 3 and source 0 once more: all, all (of nothing), all by a filled selection, 50 %, 30 %
    order = [0, 1, 2, 3, 0]
    masks = [None, None, np.ones(1, bool), rng.random(2049) < 0.5, rng.random(N) < 0.3]
    sels = [selection_from_mask(gs, device, stream, m) for m in masks]
    out, counts = gs.GaussiansBuffer.concat(stream, [bufs[k] for k in order], sels)
    parts = [rows[k] if m is None else rows[k][m] for k, m in zip(order, masks)]
    assert counts == [len(p) for p in parts] and counts[1] == 0
    assert out.len() == sum(counts) and out.pod == pod
    got = buffer_rows(out, stream)
    want = np.concatenate(parts)
    assert np.array_equal(got, want), int((got != want).any(axis=1).sum())
    for k, b in enumerate(bufs):
        assert np.array_equal(buffer_rows(b, stream), rows[k]), "the sources are untouched"
    # selections=None: everything of every source; a single source is a copy
    every, c2 = gs.GaussiansBuffer.concat(stream, bufs)
    assert c2 == lens and np.array_equal(buffer_rows(every, stream), np.concatenate(rows))
    one, c1 = gs.GaussiansBuffer.concat(stream, [bufs[3]], [sels[3]])
    assert c1 == [int(masks[3].sum())] and np.array_equal(buffer_rows(one, stream), rows[3][masks[3]])
    for o in [out, every, one] + [s for s in sels if s is not None] + bufs:
        o.destroy()


def test_concat_of_nothing_and_errors(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    a = gs.GaussiansBuffer.new_with_pods(device, pod, pod_rows(gs, sh, cov))
    b = gs.GaussiansBuffer.new_with_pods(device, pod, pod_rows(gs, sh, cov, n=2049, seed=13))
    none_a, none_b = gs.Selection(device, N), gs.Selection(device, 2049)
    out, counts = gs.GaussiansBuffer.concat(stream, [a, b], [none_a, none_b])
    assert counts == [0, 0] and out.len() == 0 and out.is_empty() and out.download(stream).size == 0
    r = gs.Renderer(device)
    frame = _frame(gs, device, stream, r, out)[0].view(f32).reshape(H, W, 4)
    assert np.array_equal(frame, np.zeros_like(frame))           # the camera's background, alpha 0
    # errors: two layouts, no source, a selection of another length; nothing is created
    c = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(1, 0), pod_rows(gs, 1, 0))
    with pytest.raises(gs.InvalidArgumentError):
        gs.GaussiansBuffer.concat(stream, [a, c])
    with pytest.raises(gs.InvalidArgumentError):
        gs.GaussiansBuffer.concat(stream, [])
    with pytest.raises(gs.InvalidArgumentError):
        gs.GaussiansBuffer.concat(stream, [a, b], [none_b, none_b])
    with pytest.raises(gs.InvalidArgumentError):
        gs.GaussiansBuffer.concat(stream, [a] * 65)
    assert np.array_equal(buffer_rows(a, stream), pod_rows(gs, sh, cov))
    for o in (r, out, none_a, none_b, c, b, a):
        o.destroy()


def test_frame_of_a_concat(gs, device, stream):
    """index order on both sides, so that the comparison does not rest on the order of exact-depth ties"""
    import synth
    pod = gs.GaussianPod(0, 0)
    pa = np.asarray(pod.from_gaussian(synth.scene(3001, first=21)))
    pb = np.asarray(pod.from_gaussian(synth.scene(1500, first=40)))
    a, b = gs.GaussiansBuffer.new_with_pods(device, pod, pa), gs.GaussiansBuffer.new_with_pods(device, pod, pb)
    a.set_spatial_order(False)
    b.set_spatial_order(False)
    both, counts = gs.GaussiansBuffer.concat(stream, [a, b])
    assert counts == [3001, 1500] and not both.spatial_order()
    fresh = gs.GaussiansBuffer.new_with_pods(device, pod, np.concatenate([pa, pb]))
    fresh.set_spatial_order(False)
    r1, r2, r3 = gs.Renderer(device), gs.Renderer(device), gs.Renderer(device)
    got, want, alone = (_frame(gs, device, stream, r, g) for r, g in ((r1, both), (r2, fresh), (r3, a)))
    assert _same(got, want) and not _same(got, alone)
    for o in (r1, r2, r3, fresh, both, b, a):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 8. select_range
# ------------------------------------------------------------------------------------------------

def test_select_range(gs, device, stream):
    n = N
    start_mask = np.random.default_rng(7).random(n) < 0.5
    sel = gs.Selection(device, n)
    cases = [(0, 0), (0, n), (31, 2), (32, 32), (33, 1), (n - 1, 1), (n, 0), (5, 1000)]
    for op in (gs.SEL_SET, gs.SEL_OR, gs.SEL_AND, gs.SEL_ANDNOT, gs.SEL_XOR):
        for start, count in cases:
            sel.upload(stream, start_mask)
            sel.select_range(stream, start, count, op)
            rng_mask = np.zeros(n, bool)
            rng_mask[start:start + count] = True
            words = sel.download_words(stream)
            assert (int(words[-1]) >> (n & 31)) == 0, (op, start, count)
            assert np.array_equal(sel.download(stream), np_op(start_mask, rng_mask, op)), (op, start, count)
            assert sel.count(stream) == int(np_op(start_mask, rng_mask, op).sum())
    # out of range: refused, the selection stays
    sel.upload(stream, start_mask)
    for start, count in [(n, 1), (1, n), (2 ** 64 - 1, 2), (0, n + 1)]:
        with pytest.raises(gs.InvalidArgumentError):
            sel.select_range(stream, start, count, gs.SEL_SET)
    assert np.array_equal(sel.download(stream), start_mask)
    # names of the ops, as everywhere; a selection of a whole number of words
    sel.select_range(stream, 0, n, "xor")
    assert np.array_equal(sel.download(stream), ~start_mask)
    even = gs.Selection(device, 64)
    even.select_range(stream, 32, 32)
    assert np.array_equal(even.download_words(stream), np.array([0, 0xFFFFFFFF], np.uint32))
    even.select_range(stream, 0, 64, gs.SEL_XOR)
    assert np.array_equal(even.download_words(stream), np.array([0xFFFFFFFF, 0], np.uint32))
    even.destroy(); sel.destroy()
