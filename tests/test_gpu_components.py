"""Connected components of the neighbour graph and the selects by cluster on the device against the
brute-force numpy restatement of tests/components_np.py: labels, sizes, info and selection words as integers.  The
components are defined without a grid and without a union-find, so the restatement has neither; the chain, the lattice,
the blob and the far outlier are the inputs a traversal or a lock-free forest gets wrong."""
import ctypes as C

import numpy as np
import pytest

import components_np
import neighbors_np
import stats_np
from records import SELECT_OPS, buffer_rows, edited_pods, np_op, sample_edit, selection_from_mask
from scenes import ALL_LAYOUTS, FOUR_LAYOUTS, N, history_masks, pod_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
UMAX = 0xFFFFFFFF
NONE = components_np.NONE
# rotation + translation + non-uniform scale (the transform of the neighbour tests)
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
    """pw of the N-scene under MT, three radii (mostly singletons; many clusters of every size; one giant cluster) and the
    restatement's labels, sizes and info for each; computed once, never written to"""
    if not _REF:
        pw = neighbors_np.positions(pod_rows(gs, 3, 0), **MT)
        d1, d8 = _kth_distance(pw, 1), _kth_distance(pw, 8)
        radii = [0.5 * d1, 1.5 * d1, d8]
        refs = [components_np.components(pw, r) for r in radii]
        # the restatement itself must see structure, or a wrong implementation could pass on a degenerate input
        S = [ref[1] for ref in refs]
        roots = [ref[0] == np.arange(N) for ref in refs]
        assert (S[0] == 1).sum() > 0.8 * N, (S[0] == 1).sum()
        mid = S[1][roots[1]]
        assert ((mid >= 2) & (mid <= 20)).sum() >= 100 and (mid > 20).sum() >= 10 and refs[1][2]["largest"] < N / 4, \
            (((mid >= 2) & (mid <= 20)).sum(), (mid > 20).sum(), refs[1][2])
        assert refs[2][2]["largest"] > 0.9 * N, refs[2][2]
        for a in [pw] + [x for ref in refs for x in ref[:2]]:
            a.setflags(write=False)
        _REF.update(pw=pw, radii=radii, refs=refs)
    return _REF


def _components(buf, stream, r, among=None, mt=None):
    """(L, S, info tuple) of the device"""
    labels, sizes, info = buf.components(stream, r, among, mt)
    n = buf.len()
    L = np.asarray(labels.download(stream, np.uint32))[:n].copy()
    S = np.asarray(sizes.download(stream, np.uint32))[:n].copy()
    i = tuple(int(v) for v in np.asarray(info.download(stream, np.uint32))[:4])
    for b in (labels, sizes, info):
        b.release()
    return L, S, i


def _agrees(got, want):
    L, S, info = got
    return np.array_equal(L, want[0]) and np.array_equal(S, want[1]) and info == components_np.info_tuple(want[2])


def _buffer_at(gs, device, positions):
    """a (no SH, rot + scale) buffer with the given positions"""
    import synth
    g = synth.scene(len(positions), first=3)
    g["pos"] = np.asarray(positions, f32)
    pod = gs.GaussianPod(3, 0)
    rows = np.asarray(pod.from_gaussian(g)).reshape(len(positions), pod.size)
    return gs.GaussiansBuffer.new_with_pods(device, pod, rows), rows


def _words(mask):
    return stats_np.pack_bits(np.asarray(mask, bool))


# ------------------------------------------------------------------------------------------------
# 1. every layout, three radii
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", ALL_LAYOUTS)
def test_components_equal_the_restatement(gs, device, stream, sh, cov):
    ref = _scene_ref(gs)
    rows = pod_rows(gs, sh, cov)
    assert np.array_equal(neighbors_np.positions(rows, **MT).view(np.uint32), ref["pw"].view(np.uint32))
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    mt = gs.model_transform_pod(**MT)
    for r, want in zip(ref["radii"], ref["refs"]):
        L, S, info = _components(buf, stream, r, None, mt)
        print(r, info, components_np.info_tuple(want[2]))
        assert L.dtype == np.uint32 and np.array_equal(L, want[0]), r
        assert np.array_equal(S, want[1]), r
        assert info == components_np.info_tuple(want[2]), r
        assert (L[5:8] == NONE).all() and not S[5:8].any()          # the planted NaN / inf rows
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
    want = components_np.components(pw, r)
    assert _agrees(_components(buf, stream, r), want)
    if n > 12:
        assert 1 < want[2]["components"] < want[2]["points"]
    sel, seeds = gs.Selection(device, n), gs.Selection(device, n)
    for lo, hi in ((1, 1), (2, UMAX), (0, UMAX)):
        sel.fill(stream)
        sel.select_components(stream, buf, r, lo, hi)
        words = sel.download_words(stream)
        assert np.array_equal(words, _words(components_np.in_size_range(want[1], lo, hi))), (lo, hi)
        if n % 32:
            assert words[-1] >> (n % 32) == 0
    seed = np.zeros(n, bool)
    seed[n // 2:n // 2 + 1] = True
    if n:
        seeds.upload(stream, seed)
    sel.fill(stream)
    sel.select_connected(stream, buf, r, seeds)
    words = sel.download_words(stream)
    assert np.array_equal(words, _words(components_np.connected(want[0], seed)))
    if n % 32:
        assert words[-1] >> (n % 32) == 0
    sel.destroy(); seeds.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 3. a chain of 4097 points spaced exactly r: diameter 4096, every edge on a cell boundary
# ------------------------------------------------------------------------------------------------

def _chain(n, y=0.0):
    return np.stack([np.arange(n, dtype=f32) * f32(0.25), np.full(n, y, f32), np.zeros(n, f32)], axis=1)


def test_chain(gs, device, stream):
    n, r = 4097, 0.25
    below = float(np.nextafter(f32(r), f32(0)))
    p = _chain(n)[np.random.default_rng(21).permutation(n)]
    buf, _ = _buffer_at(gs, device, p)
    L, S, info = _components(buf, stream, r)
    assert (L == 0).all() and (S == n).all() and info == (n, 1, n, 0)
    L, S, info = _components(buf, stream, below)
    assert np.array_equal(L, np.arange(n)) and (S == 1).all() and info == (n, n, 1, 0)
    buf.destroy()
    # two such chains 3 r apart in one buffer
    both = np.concatenate([_chain(n), _chain(n, 0.75)])
    perm = np.random.default_rng(22).permutation(2 * n)
    p = both[perm]
    second = perm >= n
    lab = np.where(second, np.flatnonzero(second)[0], np.flatnonzero(~second)[0]).astype(np.uint32)
    buf, _ = _buffer_at(gs, device, p)
    L, S, info = _components(buf, stream, r)
    assert np.array_equal(L, lab) and (S == n).all() and info == (2 * n, 2, n, 0)
    assert lab.min() == 0 and len(set(lab.tolist())) == 2
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 4. a lattice of spacing exactly r
# ------------------------------------------------------------------------------------------------

def test_lattice(gs, device, stream):
    k = np.arange(9, dtype=f32) * f32(0.25)
    p = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    p = p[np.random.default_rng(8).permutation(len(p))]
    r = 0.25
    below = float(np.nextafter(f32(r), f32(0)))
    buf, rows = _buffer_at(gs, device, p)
    L, S, info = _components(buf, stream, r)
    assert (L == 0).all() and (S == 729).all() and info == (729, 1, 729, 0)
    L, S, info = _components(buf, stream, below)
    assert np.array_equal(L, np.arange(729)) and (S == 1).all() and info == (729, 729, 1, 0)
    # the lattice against another grid origin: moved by the model transform, and moved in the data
    mt = gs.model_transform_pod(pos=(0.1, 0.1, 0.1))
    pw = neighbors_np.positions(rows, pos=(0.1, 0.1, 0.1))
    for rr in (r, below, float(np.nextafter(f32(r), f32(1)))):
        assert _agrees(_components(buf, stream, rr, None, mt), components_np.components(pw, rr)), rr
    buf.destroy()
    for off in ((0.1, 0.1, 0.1), (-0.3, 0.7, 1e-3), (100.1, -33.3, 7.7)):
        q = p + np.asarray(off, f32)
        buf, _ = _buffer_at(gs, device, q)
        want = components_np.components(q, r)
        assert _agrees(_components(buf, stream, r), want), off
        assert want[2]["largest"] > 1
        buf.destroy()


# ------------------------------------------------------------------------------------------------
# 5. contention: a complete graph of 2000, duplicates
# ------------------------------------------------------------------------------------------------

def test_contention(gs, device, stream):
    rng = np.random.default_rng(31)
    r = 1.0
    h = r * (1.0 + 2.0 ** -10)
    # 2000 singletons on a grid of spacing 3 r whose corner is the corner of the bounding box; the blob (a cube of side
    # r / 4 inside a ball of diameter r / 2) sits on a corner of the cells, so that it lies in eight of them
    g = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:2000]
    singles = (f32(-20.0) + f32(3.0) * g.astype(f32)).astype(f32)
    blob = (f32(-20.0 + 7 * h) + rng.uniform(-0.125, 0.125, (2000, 3))).astype(f32)
    d = np.sqrt(((singles.astype(np.float64) - (-20.0 + 7 * h)) ** 2).sum(axis=1))
    assert d.min() - 0.125 * np.sqrt(3.0) > 1.25 * r, "no singleton within r of the blob"
    perm = rng.permutation(4000)
    p = np.concatenate([blob, singles])[perm]
    is_blob = perm < 2000
    first = int(np.flatnonzero(is_blob)[0])
    # the blob's smallest index takes the place of its member with the largest z: it is not first in sorted order
    top = int(np.flatnonzero(is_blob)[np.argmax(p[is_blob, 2])])
    p[[first, top]] = p[[top, first]]
    assert p[first, 2] > -20.0 + 7 * h > p[is_blob, 2].min()
    buf, _ = _buffer_at(gs, device, p)
    L, S, info = _components(buf, stream, r)
    assert (L[is_blob] == first).all() and (S[is_blob] == 2000).all()
    assert np.array_equal(L[~is_blob], np.flatnonzero(~is_blob)) and (S[~is_blob] == 1).all()
    assert info == (4000, 2001, 2000, first)
    sel = gs.Selection(device, 4000)
    sel.select_components(stream, buf, r, 2, UMAX)
    assert np.array_equal(sel.download_words(stream), _words(is_blob))
    sel.destroy(); buf.destroy()
    # 300 exact duplicates at r = 0; +0 and -0 are the same place
    one = np.tile(np.array([[0.3, -1.7, 0.0]], f32), (300, 1))
    one[::3, 2] = -0.0
    assert np.signbit(one[0, 2]) and not np.signbit(one[1, 2])
    buf, _ = _buffer_at(gs, device, one)
    L, S, info = _components(buf, stream, 0.0)
    assert (L == 0).all() and (S == 300).all() and info == (300, 1, 300, 0)
    buf.destroy()


# ------------------------------------------------------------------------------------------------
# 6. Gaussians that are no points, `among`
# ------------------------------------------------------------------------------------------------

def test_non_points_and_among(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 0, 0
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    r = ref["radii"][1]
    out = gs.Selection(device, N)
    for name, mask in history_masks():
        among = selection_from_mask(gs, device, stream, mask)
        pt = neighbors_np.points(ref["pw"], mask)
        want = components_np.components(ref["pw"], r, mask)
        L, S, info = _components(buf, stream, r, among, mt)
        assert _agrees((L, S, info), want), name
        assert (L[~pt] == NONE).all() and not S[~pt].any() and not pt[5:8].any()
        assert (L[pt] <= np.flatnonzero(pt)).all()                    # caller indices of the full buffer
        out.fill(stream)
        out.select_components(stream, buf, r, 0, UMAX, among, mt)      # a non-point is never selected
        assert np.array_equal(out.download_words(stream), _words(pt)), name
        if among is not None:
            among.destroy()
    # the sizes among a subset are those of the subset alone, its labels the subset's mapped back
    mask = history_masks()[0][1]
    whole, sub = components_np.components(ref["pw"], r, mask), components_np.components(ref["pw"][mask], r)
    assert np.array_equal(whole[1][mask], sub[1])
    idx = np.flatnonzero(mask)
    subpt = sub[0] != NONE
    assert np.array_equal(whole[0][mask][subpt], idx[sub[0][subpt]])
    out.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 7. a far outlier changes nobody's label or size
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
        for r, want in zip(ref["radii"][:2], ref["refs"][:2]):
            L, S, info = _components(buf, stream, r, None, mt)
            assert np.array_equal(L[:N], want[0]) and np.array_equal(S[:N], want[1]), r
            assert (L[N:] == N).all() and (S[N:] == len(extra)).all()      # two outliers at one place are a component of 2
            w = want[2]
            assert info == (w["points"] + len(extra), w["components"] + 1, w["largest"], w["largest_label"])
        buf.destroy()


# ------------------------------------------------------------------------------------------------
# 8. select_components: the five ops, the ends of the size range, the tail
# ------------------------------------------------------------------------------------------------

def test_select_components_ops(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 2, 1
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    r, S = ref["radii"][1], ref["refs"][1][1]
    prior = np.random.default_rng(7).random(N) < 0.5
    sel = gs.Selection(device, N)
    for op in SELECT_OPS:
        for lo, hi in ((1, 1), (2, 20), (21, UMAX), (0, UMAX), (0, 0), (5, 4), (UMAX, UMAX)):
            sel.upload(stream, prior)
            sel.select_components(stream, buf, r, lo, hi, None, mt, op)
            want = np_op(prior, components_np.in_size_range(S, lo, hi), op)
            assert np.array_equal(sel.download_words(stream), _words(want)), (op, lo, hi)
    for lo, hi in ((1, 1), (2, 20), (21, UMAX)):
        assert 0 < components_np.in_size_range(S, lo, hi).sum() < N
    assert not components_np.in_size_range(S, 0, 0).any() and components_np.in_size_range(S, 0, UMAX).sum() == N - 3
    sel.destroy(); buf.destroy()


@pytest.mark.parametrize("op", SELECT_OPS)
def test_selects_keep_the_tail_clear(gs, device, stream, op):
    n = 65
    sh, cov = 0, 0
    rows = pod_rows(gs, sh, cov, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    pw = neighbors_np.positions(rows)
    r = 2.0 * _kth_distance(pw, 1)
    L, S, _ = components_np.components(pw, r)
    pt = neighbors_np.points(pw)
    ones, zeros = np.ones(n, bool), np.zeros(n, bool)
    sel, seeds = gs.Selection(device, n), gs.Selection(device, n)
    sel.fill(stream)
    sel.select_components(stream, buf, r, 0, UMAX, op=op)
    words = sel.download_words(stream)
    assert len(words) == 3 and words[2] >> 1 == 0
    assert np.array_equal(words, _words(np_op(ones, pt, op)))
    sel.fill(stream)
    sel.select_components(stream, buf, r, 2, 1, op=op)                   # min_size > max_size: T is empty
    assert np.array_equal(sel.download_words(stream), _words(np_op(ones, zeros, op)))
    sel.clear(stream)
    sel.select_components(stream, buf, r, 2, UMAX, op=op)
    assert np.array_equal(sel.download_words(stream), _words(np_op(zeros, S >= 2, op)))
    seeds.fill(stream)
    sel.fill(stream)
    sel.select_connected(stream, buf, r, seeds, op=op)
    words = sel.download_words(stream)
    assert words[2] >> 1 == 0 and np.array_equal(words, _words(np_op(ones, pt, op)))
    assert sel.count(stream) <= n
    sel.destroy(); seeds.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 9. select_connected
# ------------------------------------------------------------------------------------------------

def test_select_connected(gs, device, stream):
    ref = _scene_ref(gs)
    sh, cov = 1, 0
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    r, (L, S, _) = ref["radii"][1], ref["refs"][1]
    sel, seeds = gs.Selection(device, N), gs.Selection(device, N)

    def grown(seed_mask, op="set", prior=None):
        seeds.upload(stream, seed_mask)
        if prior is None:
            sel.fill(stream)
        else:
            sel.upload(stream, prior)
        sel.select_connected(stream, buf, r, seeds, None, mt, op)
        return sel.download_words(stream)

    def one(i):
        m = np.zeros(N, bool)
        m[i] = True
        return m

    mid = int(np.flatnonzero((S >= 8) & (S <= 20))[-1])                 # inside a mid-size component, not its label
    assert L[mid] != mid
    assert np.array_equal(grown(one(mid)), _words(L == L[mid])) and (L == L[mid]).sum() == S[mid]
    # a picked index becomes a seed through select_range
    seeds.select_range(stream, mid, 1)
    sel.select_connected(stream, buf, r, seeds, model_transform=mt)
    assert np.array_equal(sel.download_words(stream), _words(L == L[mid]))
    single = int(np.flatnonzero(S == 1)[3])
    assert np.array_equal(grown(one(single)), _words(one(single)))
    assert not grown(one(6)).any() and L[6] == NONE                      # a seed on a non-point selects nothing
    assert not grown(np.zeros(N, bool)).any()                            # empty seeds
    assert np.array_equal(grown(np.ones(N, bool)), _words(L != NONE))    # all seeds: all points
    rng = np.random.default_rng(17)
    some = rng.random(N) < 0.01
    prior = rng.random(N) < 0.5
    for op in SELECT_OPS:
        want = np_op(prior, components_np.connected(L, some), op)
        assert np.array_equal(grown(some, op, prior), _words(want)), op
    # seeds is sel: grow a selection to whole clusters
    for op in ("set", "or"):
        sel.upload(stream, some)
        sel.select_connected(stream, buf, r, sel, None, mt, op)
        want = np_op(some, components_np.connected(L, some), op)
        assert np.array_equal(sel.download_words(stream), _words(want)), op
    assert components_np.connected(L, some).sum() > some.sum()
    sel.destroy(); seeds.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 10. the cleanup workflow: remove the small clusters
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", FOUR_LAYOUTS)
def test_remove_small_clusters(gs, device, stream, sh, cov):
    ref = _scene_ref(gs)
    rows = pod_rows(gs, sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), rows)
    mt = gs.model_transform_pod(**MT)
    m = 21
    small = components_np.in_size_range(ref["refs"][1][1], 1, m - 1)
    assert 0 < small.sum() < N - 3
    sel = gs.Selection(device, N)
    sel.select_components(stream, buf, ref["radii"][1], max_size=m - 1, model_transform=mt)
    assert sel.count(stream) == int(small.sum())
    kept = buf.extract(stream, sel, invert=True)
    assert kept.len() == N - int(small.sum())
    assert np.array_equal(buffer_rows(kept, stream), rows[~small])
    assert np.array_equal(buffer_rows(buf, stream), rows)
    kept.destroy(); sel.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# 11. ordering behind an edit on another stream
# ------------------------------------------------------------------------------------------------

def test_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    sh, cov = 0, 0
    pod = gs.GaussianPod(sh, cov)
    orig = pod_rows(gs, sh, cov)
    mask = np.random.default_rng(4).random(N) < 0.3
    s1, s2 = stream, device.create_stream()
    sel, out, seeds = selection_from_mask(gs, device, s1, mask), gs.Selection(device, N), gs.Selection(device, N)
    s1.synchronize()
    edited = edited_pods(gs, sh, cov, orig.reshape(-1), mask, 15).reshape(N, pod.size)
    pw, before = neighbors_np.positions(edited), neighbors_np.positions(orig)
    r = 1.5 * _kth_distance(before, 1)
    want, want0 = components_np.components(pw, r), components_np.components(before, r)
    assert not np.array_equal(want[0], want0[0]) and not np.array_equal(want[1], want0[1]), "the edit changes the components"
    seed = np.zeros(N, bool)
    seed[np.flatnonzero(want[1] >= 5)[-1]] = True                   # inside a cluster of the EDITED scene
    seeds.upload(s1, seed)
    s1.synchronize()
    assert components_np.connected(want[0], seed).sum() >= 5
    for what in ("components", "select", "connected"):
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, orig)
        buf.edit(s1, sel, sample_edit(gs, 15))
        # on stream 2 right behind the edit on stream 1, no host synchronisation in between
        if what == "components":
            assert _agrees(_components(buf, s2, r), want)
        elif what == "select":
            out.select_components(s2, buf, r, 2, 20)
            assert np.array_equal(out.download_words(s2), _words(components_np.in_size_range(want[1], 2, 20)))
        else:
            out.select_connected(s2, buf, r, seeds)
            assert np.array_equal(out.download_words(s2), _words(components_np.connected(want[0], seed)))
        s1.synchronize()
        assert np.array_equal(buffer_rows(buf, s1), edited)
        buf.destroy()
    s2.synchronize()
    sel.destroy(); out.destroy(); seeds.destroy()
    s2.close()


# ------------------------------------------------------------------------------------------------
# 12. runs are identical; a caller's plane; the scratch shared with the neighbour counts
# ------------------------------------------------------------------------------------------------

def _bytes(buf, stream, r, mt=None):
    """the three outputs as the device wrote them, every byte"""
    out = buf.components(stream, r, None, mt)
    raw = [np.asarray(b.download(stream, np.uint32)).copy() for b in out]
    for b in out:
        b.release()
    return raw


def test_runs_are_identical(gs, device, stream):
    ref = _scene_ref(gs)
    s2 = device.create_stream()
    n = 4097
    chain, _ = _buffer_at(gs, device, _chain(n)[np.random.default_rng(21).permutation(n)])
    rng = np.random.default_rng(33)
    blob_p = np.concatenate([rng.uniform(-0.1, 0.1, (2000, 3)), rng.uniform(5, 50, (500, 3))]).astype(f32)[rng.permutation(2500)]
    blob, _ = _buffer_at(gs, device, blob_p)
    sh, cov = 1, 2
    scene = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(sh, cov), pod_rows(gs, sh, cov))
    mt = gs.model_transform_pod(**MT)
    for buf, r, m in ((chain, 0.25, None), (blob, 1.0, None), (scene, ref["radii"][2], mt)):
        a, b, c = _bytes(buf, stream, r, m), _bytes(buf, stream, r, m), _bytes(buf, s2, r, m)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.array_equal(a[0][:N], ref["refs"][2][0]) and np.array_equal(a[1][:N], ref["refs"][2][1])
    # labels into the caller's plane, larger than needed: the bytes behind 4 n stay; so do those behind the info's 16
    plane = gs.Buffer(device, data=np.full(N + 3, 0x5A5A5A5A, np.uint32))
    info = gs.Buffer(device, data=np.full(6, 0x5A5A5A5A, np.uint32))
    r, want = ref["radii"][1], ref["refs"][1]
    out = scene.components(stream, r, None, mt, labels_out=plane, info_out=info)
    assert out[0] is plane and out[2] is info
    got = np.asarray(plane.download(stream, np.uint32))
    assert np.array_equal(got[:N], want[0]) and (got[N:] == 0x5A5A5A5A).all()
    got = np.asarray(info.download(stream, np.uint32))
    assert tuple(got[:4].tolist()) == components_np.info_tuple(want[2]) and (got[4:] == 0x5A5A5A5A).all()
    assert np.array_equal(np.asarray(out[1].download(stream, np.uint32))[:N], want[1])
    out[1].release(); plane.release(); info.release()
    # neighbour counts between two component calls on one buffer share the scratch: all three stay right
    assert _agrees(_components(scene, stream, r, None, mt), want)
    counts = scene.neighbor_counts(s2, r, UMAX, None, mt)
    again = _components(scene, stream, r, None, mt)
    assert np.array_equal(np.asarray(counts.download(s2, np.uint32))[:N], neighbors_np.counts(ref["pw"], r).astype(np.uint32))
    assert _agrees(again, want)
    counts.release()
    s2.synchronize()
    s2.close()
    for b in (chain, blob, scene):
        b.destroy()


# ------------------------------------------------------------------------------------------------
# 13. argument errors
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
    labels, sizes, info = gs.Buffer(device, data=fill), gs.Buffer(device, data=fill), gs.Buffer(device, data=fill[:4])
    small, small_info = gs.Buffer(device, size=4 * N - 4), gs.Buffer(device, size=12)
    L, bad = gs._L, gs.InvalidArgumentError.code
    mt = C.byref(gs.model_transform_pod(**MT))
    nan, inf = float("nan"), float("inf")

    def components(g=buf._h, among=sel._h, r=0.5, lab=labels._h, siz=sizes._h, inf_=info._h):
        return L.gs_gaussians_buffer_components(g, stream._h, among, mt, r, lab, siz, inf_)

    assert components(g=None) == bad and components(lab=None, siz=None, inf_=None) == bad
    for r in (-1.0, nan, inf, -inf, 1e20):
        assert components(r=r) == bad, r
    for k in ("lab", "siz"):
        assert components(**{k: small._h}) == bad and components(**{k: foreign_plane._h}) == bad
    assert components(inf_=small_info._h) == bad and components(inf_=foreign_plane._h) == bad
    assert components(among=short._h) == bad and components(among=foreign._h) == bad
    for b in (labels, sizes):
        assert np.array_equal(np.asarray(b.download(stream, np.uint32)), fill)
    assert np.array_equal(np.asarray(info.download(stream, np.uint32)), fill[:4])

    def select(s=sel._h, g=buf._h, among=None, r=0.5, lo=1, hi=3, op=0):
        return L.gs_select_components(s, stream._h, g, among, mt, r, lo, hi, op)

    def connected(s=sel._h, g=buf._h, among=None, r=0.5, seeds=sel._h, op=0):
        return L.gs_select_connected(s, stream._h, g, among, mt, r, seeds, op)

    for call in (select, connected):
        assert call(s=None) == bad and call(g=None) == bad
        assert call(op=5) == bad and call(op=-1) == bad
        for r in (-1.0, nan, inf, -inf, 1e20):
            assert call(r=r) == bad, r
        assert call(s=short._h) == bad and call(s=foreign._h) == bad
        assert call(among=short._h) == bad and call(among=foreign._h) == bad
    assert connected(seeds=None) == bad and connected(seeds=short._h) == bad and connected(seeds=foreign._h) == bad
    assert np.array_equal(sel.download_words(stream), words)
    # and the valid calls next to them
    assert components(r=0.0) == 0 and components(lab=None, siz=None) == 0 and components(inf_=None, among=None) == 0
    assert select(r=0.0, lo=0, hi=0, op=1) == 0 and connected(r=0.0, op=1) == 0
    stream.synchronize()
    # OR with nothing, then OR with the clusters of itself at r = 0: the exact duplicates of a selected point join
    L0 = components_np.components(neighbors_np.positions(pod_rows(gs, sh, cov), **MT), 0.0)[0]
    assert np.array_equal(sel.download_words(stream), _words(mask | components_np.connected(L0, mask)))
    for o in (sel, short, foreign):
        o.destroy()
    for o in (labels, sizes, info, small, small_info, foreign_plane):
        o.release()
    buf.destroy()
