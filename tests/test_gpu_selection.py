"""Gaussian selections: the device bitmask and its ops against numpy, the sphere / box / visible select
ops against their binary32 definitions, and frames that hide or tint a selection against the oracle.  A hidden Gaussian is
a culled one, and the oracle culls a Gaussian whose opacity byte is 0 (splat mode), so "scene with S hidden" has an exact
oracle twin: the same scene — same positions, same mirror order — with the opacity byte of S set to 0."""
import numpy as np
import pytest

import helpers
from frames import Scene, tint32
from helpers import band_rows, bits, deep_scene
from records import SELECT_OPS, np_op

pytestmark = pytest.mark.gpu

f32 = np.float32


def _tail_mask(n):
    return np.uint32((1 << (n & 31)) - 1 if n & 31 else 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------
# 1. bit operations
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 31, 32, 33, 1024, 100003])
def test_bit_operations(gs, device, stream, n):
    rng = np.random.default_rng(n)
    nw = gs.selection_words(n)
    a, b = gs.Selection(device, n), gs.Selection(device, n)
    assert len(a) == n and a.count(stream) == 0 and not a.download(stream).any()
    a.fill(stream)
    w = a.download_words(stream)
    assert (w[:-1] == 0xFFFFFFFF).all() and w[-1] == _tail_mask(n) and a.count(stream) == n
    a.clear(stream)
    assert a.count(stream) == 0
    a.invert(stream)
    w = a.download_words(stream)
    assert (w[:-1] == 0xFFFFFFFF).all() and w[-1] == _tail_mask(n), "invert must mask the tail"
    # upload: random words, tail bits included — they are dropped
    wa = rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)
    wb = rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)
    a.upload(stream, wa)
    b.upload(stream, wb)
    wa[-1] &= _tail_mask(n)
    wb[-1] &= _tail_mask(n)
    assert np.array_equal(a.download_words(stream), wa) and np.array_equal(b.download_words(stream), wb)
    assert a.count(stream) == int(np.unpackbits(wa.view(np.uint8)).sum())
    flags = a.download(stream)
    assert flags.dtype == np.bool_ and flags.shape == (n,)
    assert np.array_equal(flags, np.unpackbits(wa.view(np.uint8), bitorder="little")[:n].astype(bool))
    # bool round trip
    fl = rng.random(n) < 0.3
    a.upload(stream, fl)
    assert np.array_equal(a.download(stream), fl) and a.count(stream) == int(fl.sum())
    a.upload(stream, wa)
    for op in SELECT_OPS:
        a.upload(stream, wa)
        a.combine(stream, op, b)
        want = np_op(wa, wb, op)
        got = a.download_words(stream)
        assert np.array_equal(got, want), op
        assert got[-1] & ~_tail_mask(n) == 0
        assert a.count(stream) == int(np.unpackbits(want.view(np.uint8)).sum())
    a.upload(stream, wa)
    a.invert(stream)
    want = ~wa
    want[-1] &= _tail_mask(n)
    assert np.array_equal(a.download_words(stream), want)
    c = gs.Selection(device, n + 1)
    with pytest.raises(gs.InvalidArgumentError):
        a.combine(stream, "or", c)
    with pytest.raises(gs.InvalidArgumentError):
        gs._check(gs._L.gs_selection_upload(a._h, stream._h, gs._ptr(np.zeros(nw + 1, np.uint32)), nw + 1))
    for s in (a, b, c):
        s.destroy()


# ------------------------------------------------------------------------------------------------
# 2 / 3. sphere and box
# ------------------------------------------------------------------------------------------------

def _model_mat32(mt):
    """model_transform_mat for the transforms of the exact cases: identity rotation, so M = diag(scale)
    with the translation in the last column — every entry exact in f32"""
    assert tuple(mt.rot) == (0.0, 0.0, 0.0, 1.0)
    m = np.zeros((4, 4), f32)
    for k in range(3):
        m[k, k] = mt.scale[k]
        m[k, 3] = mt.pos[k]
    m[3, 3] = 1.0
    return m


def _world32(m, p):
    """pw = M (p, 1), ((c0 + c1) + c2) + c3 in binary32, every operation rounded"""
    p = p.astype(f32)
    with np.errstate(all="ignore"):
        return np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], axis=1)


def _sphere32(pw, c, radius):
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        d = pw - c
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= f32(radius) * f32(radius)


def _box32(pw, b):
    b = np.asarray(b, f32)
    with np.errstate(all="ignore"):
        q = [((b[r] * pw[:, 0] + b[3 + r] * pw[:, 1]) + b[6 + r] * pw[:, 2]) + b[9 + r] for r in range(3)]
        return (np.abs(q[0]) <= 1) & (np.abs(q[1]) <= 1) & (np.abs(q[2]) <= 1)


def _uniform_scene(n, seed, half=8.0):
    import synth
    g = synth.scene(n, first=seed)
    rng = np.random.default_rng(seed)
    g["pos"] = rng.uniform(-half, half, (n, 3)).astype(f32)
    return g


@pytest.mark.parametrize("sh,cov", [(0, 0), (3, 2)])
def test_sphere_and_box_exact(gs, device, stream, sh, cov):
    n = 50_001
    g = _uniform_scene(n, 3)
    g["pos"][17] = np.nan
    g["pos"][18, 1] = np.nan
    g["pos"][19] = np.inf
    pod = gs.GaussianPod(sh, cov)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod.from_gaussian(g))
    sel = gs.Selection(device, n)
    transforms = [gs.model_transform_pod(),
                  gs.model_transform_pod(pos=(0.5, -2.0, 0.125)),
                  gs.model_transform_pod(scale=(2.0, 0.5, 4.0)),
                  gs.model_transform_pod(pos=(-1.0, 0.25, 3.0), scale=(0.5, 0.5, 2.0))]
    rng = np.random.default_rng(5)
    for mt in transforms:
        pw = _world32(_model_mat32(mt), g["pos"])
        for center, radius in [((0.0, 0.0, 0.0), 5.0), ((1.25, -0.5, 2.0), 3.3), ((3.0, 3.0, 3.0), 0.0), ((0, 0, 0), 1e9)]:
            sel.select_sphere(stream, buf, mt, center, radius)
            want = _sphere32(pw, center, radius)
            got = sel.download(stream)
            assert np.array_equal(got, want), (tuple(mt.pos), tuple(mt.scale), center, radius, int((got != want).sum()))
            assert not got[17:20].any(), "NaN / inf positions select nothing"
        # a radius-0 sphere on a Gaussian's own world position selects it
        k = 4711
        sel.select_sphere(stream, buf, mt, pw[k], 0.0)
        got = sel.download(stream)
        assert got[k] and np.array_equal(got, _sphere32(pw, pw[k], 0.0))
        for lo, hi in [((-4, -4, -4), (4, 4, 4)), ((-1.5, 0.25, -6.0), (7.0, 2.0, 1.0))]:
            b = gs.box_from_bounds(lo, hi)
            sel.select_box(stream, buf, mt, b)
            want = _box32(pw, b)
            got = sel.download(stream)
            assert np.array_equal(got, want) and not got[17:20].any()
            assert 0 < want.sum() < n
        # a sheared box, and every op on top of a random selection
        b = rng.uniform(-0.2, 0.2, 12).astype(f32)
        want_box = _box32(pw, b)
        for op in SELECT_OPS:
            base = rng.random(n) < 0.5
            sel.upload(stream, base)
            sel.select_box(stream, buf, mt, b, op=op)
            assert np.array_equal(sel.download(stream), np_op(base, want_box, op)), op
            sel.upload(stream, base)
            sel.select_sphere(stream, buf, mt, (1.0, 1.0, 1.0), 6.0, op=op)
            assert np.array_equal(sel.download(stream), np_op(base, _sphere32(pw, (1.0, 1.0, 1.0), 6.0), op)), op
    for bad in (-1.0, float("nan")):
        with pytest.raises(gs.InvalidArgumentError):
            sel.select_sphere(stream, buf, transforms[0], (0, 0, 0), bad)
    short = gs.Selection(device, n - 1)
    with pytest.raises(gs.InvalidArgumentError):
        short.select_sphere(stream, buf, transforms[0], (0, 0, 0), 1.0)
    with pytest.raises(gs.InvalidArgumentError):
        short.select_box(stream, buf, transforms[0], gs.box_from_bounds((-1, -1, -1), (1, 1, 1)))
    short.destroy(); sel.destroy(); buf.destroy()


def _quat_mat64(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_sphere_and_box_general_transform(gs, device, stream):
    """a general rotation and scale against float64; Gaussians within a relative 1e-5 of the boundary are left out, and
    they must be at most 0.1 % (uniform positions, shapes well inside the scene: the shell is ~3e-5 of the volume)"""
    n = 200_000
    g = _uniform_scene(n, 9)
    pod = gs.GaussianPod(3, 0)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod.from_gaussian(g))
    sel = gs.Selection(device, n)
    q = np.array([0.3, -0.5, 0.2, 0.7])
    q = (q / np.linalg.norm(q)).astype(f32)
    scale, pos = np.array([1.3, 0.7, 0.9], f32), np.array([0.3, -0.4, 0.6], f32)
    mt = gs.model_transform_pod(pos=tuple(pos), rot=tuple(q), scale=tuple(scale))
    pw = g["pos"].astype(np.float64) @ (_quat_mat64(q) * scale.astype(np.float64)).T + pos.astype(np.float64)
    center, radius = np.array([0.5, 0.25, -0.75], f32), f32(4.0)
    sel.select_sphere(stream, buf, mt, center, radius)
    got = sel.download(stream)
    d2 = ((pw - center.astype(np.float64)) ** 2).sum(axis=1)
    r2 = float(radius) ** 2
    near = np.abs(d2 - r2) <= 1e-5 * r2
    assert near.mean() <= 1e-3
    assert np.array_equal(got[~near], (d2 <= r2)[~near])
    assert 0.05 * n < got.sum() < 0.5 * n
    ang = 0.4
    rot = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    lin = np.diag([1 / 3.0, 1 / 2.5, 1 / 3.5]) @ rot
    b = np.concatenate([lin.T.reshape(-1), -lin @ np.array([0.5, -0.5, 0.25])]).astype(f32)
    sel.select_box(stream, buf, mt, b)
    got = sel.download(stream)
    b64 = b.astype(np.float64)
    qv = pw @ b64[:9].reshape(3, 3) + b64[9:]
    near = (np.abs(np.abs(qv) - 1.0) <= 1e-5).any(axis=1)
    assert near.mean() <= 1e-3
    assert np.array_equal(got[~near], (np.abs(qv) <= 1.0).all(axis=1)[~near])
    assert 0.01 * n < got.sum() < 0.5 * n
    sel.destroy(); buf.destroy()


# ------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------

def _check_hidden_frame(sc, r, fr, hidden, band=None, cam=None, ocam=None, taps=True):
    """image bit-equal to the oracle twin's; with `taps` also V, D, the sorted keys and caller indices and the projected tap"""
    o = sc.oracle(sc.twin_pods(hidden), band=band, ocam=ocam)
    y0, y1 = band_rows(band, sc.H)
    img = sc.image()
    bad = bits(img[y0:y1]) != bits(o["rgba"][y0:y1])
    assert not bad.any(), "%d words of the image differ from the oracle twin" % bad.sum()
    if not taps:
        return o
    assert fr.visible == int((o["tiles"] > 0).sum()) and fr.pairs == int(o["tiles"].astype(np.uint64).sum())
    keys, idx = r.download_sorted()
    assert np.array_equal(keys, o["keys"]) and np.array_equal(idx, o["idx"])
    proj, tiles = r.download_projected(sc.n)
    assert np.array_equal(tiles, o["tiles"])
    assert not tiles[np.asarray(hidden, bool)].any()
    keep = tiles > 0
    assert np.array_equal(proj[keep].tobytes(), o["proj"][keep].tobytes())
    return o


# ------------------------------------------------------------------------------------------------
# 4. select_visible
# ------------------------------------------------------------------------------------------------

def _visible_want(o, x0, y0, x1, y1, mask, W, H):
    mx, my = o["proj"]["mx"], o["proj"]["my"]
    with np.errstate(all="ignore"):
        want = (o["tiles"] > 0) & (f32(x0) <= mx) & (mx < f32(x1)) & (f32(y0) <= my) & (my < f32(y1))
        if mask is not None:
            inside = (mx >= 0) & (my >= 0) & (mx < W) & (my < H)
            px = np.where(inside, np.floor(mx), 0).astype(np.int64)
            py = np.where(inside, np.floor(my), 0).astype(np.int64)
            want &= inside & (mask[py, px] != 0)
    return want


@pytest.mark.parametrize("spatial", [True, False])
def test_select_visible(gs, ob, device, stream, spatial):
    n, W, H = 90_000, 320, 192
    sc = Scene(gs, ob, device, stream, 1, 0, n, W, H, first=4242, spatial=spatial)
    views = {"all": ((0, 0, 12), (0, 0, -14), 70.0), "corner": ((0, 0, 0), (13, 7, -3), 25.0)}
    rng = np.random.default_rng(1)
    mask = (rng.random((H, W)) < 0.5).astype(np.uint8)
    mask_buf = gs.Buffer(device, data=mask)
    r = gs.Renderer(device)
    sel = gs.Selection(device, n)
    with pytest.raises(gs.InvalidArgumentError):      # no last frame
        r.select_visible(stream, sel, 0, 0, W, H)
    launches = []
    # all -> corner (in-kernel block test) -> corner (block list) -> a band of the wide view
    for name, band in [("all", None), ("corner", None), ("corner", None), ("all", (3, 8))]:
        e, t, fov = views[name]
        ocam = helpers.default_camera(ob, W, H, eye=e, target=t, vfov_deg=fov)
        cam = helpers.copy_camera(ocam, gs.Camera)
        fr = sc.render(r, band=band, cam=cam)
        launches.append(fr.launches)
        o = sc.oracle(sc.pods, band=band, ocam=ocam)
        assert fr.visible == int((o["tiles"] > 0).sum())
        for region in [(-1e9, -1e9, 1e9, 1e9), (40.5, 30.0, 200.25, 150.0), (0.0, 0.0, 0.0, 0.0)]:
            for m, mptr in ((None, None), (mask, mask_buf.device_ptr())):
                r.select_visible(stream, sel, *region, mask_device_ptr=mptr)
                want = _visible_want(o, *region, m, W, H)
                got = sel.download(stream)
                assert np.array_equal(got, want), (name, band, region, m is not None, int((got != want).sum()))
        want = _visible_want(o, 40.5, 30.0, 200.25, 150.0, mask, W, H)
        for op in SELECT_OPS:
            base = rng.random(n) < 0.5
            sel.upload(stream, base)
            r.select_visible(stream, sel, 40.5, 30.0, 200.25, 150.0, mask_device_ptr=mask_buf.device_ptr(), op=op)
            assert np.array_equal(sel.download(stream), np_op(base, want, op)), (name, op)
    if spatial:
        assert launches[2] == launches[1] + 1, "the second corner frame should take the block list"
    # Gaussians hidden in the frame are not visible
    hidden = rng.random(n) < 0.5
    hs = sc.selection(hidden)
    sc.render(r, hide=hs)
    r.select_visible(stream, sel, -1e9, -1e9, 1e9, 1e9)
    got = sel.download(stream)
    o = sc.oracle(sc.twin_pods(hidden))
    assert np.array_equal(got, o["tiles"] > 0) and not (got & hidden).any() and got.any()
    short = gs.Selection(device, n - 1)
    with pytest.raises(gs.InvalidArgumentError):
        r.select_visible(stream, short, 0, 0, W, H)
    for s in (short, hs, sel):
        s.destroy()
    mask_buf.release(); r.destroy(); sc.release()


# ------------------------------------------------------------------------------------------------
# 5. hide
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", [(0, 0), (3, 0), (1, 2)])      # f32 SH (banded), SH-less (k_preprocess), f16 SH + f16 cov
def test_hide_matches_the_oracle_twin(gs, ob, device, stream, sh, cov):
    n, W, H = 30_001, 333, 197                                  # n is no multiple of 1024
    sc = Scene(gs, ob, device, stream, sh, cov, n, W, H)
    rng = np.random.default_rng(sh * 3 + cov)
    hidden = rng.random(n) < 0.4
    hs = sc.selection(hidden)
    r = gs.Renderer(device)
    for band in (None, (3, 9)):
        sc.poison()
        fr = sc.render(r, band=band, hide=hs)
        _check_hidden_frame(sc, r, fr, hidden, band=band)
        y0, y1 = band_rows(band, H)
        img = sc.image()
        assert np.isnan(img[:y0]).all() and np.isnan(img[y1:]).all()
    r.destroy(); hs.destroy(); sc.release()


@pytest.mark.parametrize("mode", [1, 2])
def test_hide_ellipse_and_point_modes(gs, ob, device, stream, mode):
    """the oracle does not cull opacity 0 in these modes (the counts differ); the image is the twin's bit for bit"""
    n, W, H = 20_000, 333, 197
    sc = Scene(gs, ob, device, stream, 0, 0, n, W, H, mode=mode)
    hidden = np.random.default_rng(mode).random(n) < 0.5
    hs = sc.selection(hidden)
    r = gs.Renderer(device)
    fr = sc.render(r, hide=hs)
    _check_hidden_frame(sc, r, fr, hidden, taps=False)
    proj, tiles = r.download_projected(n)
    assert not tiles[hidden].any()
    r.destroy(); hs.destroy(); sc.release()


@pytest.mark.parametrize("spatial", [True, False])
def test_hide_box_list_frame_and_block_skip(gs, ob, device, stream, spatial):
    """a crop box hides whole 1024-blocks of the spatially ordered mirror; the narrow view takes the block list"""
    n, W, H = 90_000, 320, 192
    sc = Scene(gs, ob, device, stream, 1, 0, n, W, H, first=4242, spatial=spatial)
    sel = gs.Selection(device, n)
    pos = sc.g["pos"]
    lo, hi = np.percentile(pos, 30, axis=0), np.percentile(pos, 80, axis=0)
    sel.select_box(stream, sc.buf, sc.mt, gs.box_from_bounds(lo, hi))
    sel.invert(stream)                      # hide what lies OUTSIDE the box
    hidden = sel.download(stream)
    assert 0.5 * n < hidden.sum() < n
    order = sc.order()
    full_blocks = hidden[order][: n // 1024 * 1024].reshape(-1, 1024).all(axis=1).sum()
    if spatial:
        assert full_blocks > 0, "the scene should have fully hidden blocks"
    r = gs.Renderer(device)
    views = {"all": ((0, 0, 12), (0, 0, -14), 70.0), "corner": ((0, 0, 0), (13, 7, -3), 25.0)}
    for k, name in enumerate(["all", "corner", "corner", "all"]):
        e, t, fov = views[name]
        ocam = helpers.default_camera(ob, W, H, eye=e, target=t, vfov_deg=fov)
        fr = sc.render(r, cam=helpers.copy_camera(ocam, gs.Camera), hide=sel)
        _check_hidden_frame(sc, r, fr, hidden, ocam=ocam)
    r.destroy(); sel.destroy(); sc.release()


def test_hide_two_rounds(gs, ob, device, stream):
    n, W, H = 120_000, 640, 360
    sc = Scene(gs, ob, device, stream, gs.SH_NONE, 0, n, W, H, g=deep_scene(n))
    hidden = np.random.default_rng(2).random(n) < 0.3
    hs = sc.selection(hidden)
    o = sc.oracle(sc.twin_pods(hidden))
    for k in (5_000, 40_000):
        r = gs.Renderer(device)
        r.set_rounds(1, k)
        for frame in range(2):              # the second frame is partitioned
            sc.poison()
            sc.render(r, hide=hs)
            assert r.sort_info().rounds == 2
            assert np.array_equal(bits(sc.image()), bits(o["rgba"])), (k, frame)
        r.destroy()
    hs.destroy(); sc.release()


def test_hide_everything_and_shared_selection(gs, ob, device, stream):
    n, W, H = 20_000, 200, 120
    sc = Scene(gs, ob, device, stream, 0, 0, n, W, H)
    sc.ocam.background[:] = [0.25, 0.5, 0.75]
    sc.cam = helpers.copy_camera(sc.ocam, gs.Camera)
    hs = gs.Selection(device, n)
    hs.fill(stream)
    r1, r2 = gs.Renderer(device), gs.Renderer(device)
    fr = sc.render(r1, hide=hs)
    assert fr.visible == 0 and fr.pairs == 0
    img = sc.image()
    assert np.array_equal(bits(img), bits(sc.oracle(sc.twin_pods(np.ones(n, bool)))["rgba"]))
    assert (img[..., :3] == np.array([0.25, 0.5, 0.75], f32)).all()
    # two renderers share one selection; a change reaches both
    hidden = np.random.default_rng(3).random(n) < 0.5
    hs.upload(stream, hidden)
    for r in (r1, r2, r1, r2):
        sc.poison()
        fr = sc.render(r, hide=hs)
        _check_hidden_frame(sc, r, fr, hidden)
    hs.invert(stream)
    for r in (r2, r1):
        sc.poison()
        fr = sc.render(r, hide=hs)
        _check_hidden_frame(sc, r, fr, ~hidden)
    r1.destroy(); r2.destroy(); hs.destroy(); sc.release()


def test_hide_follows_caller_indices_across_a_reorder(gs, ob, device, stream):
    """an update_range large enough to rebuild the mirror order between two frames: the mask still names caller indices"""
    import synth
    n, W, H = 40_000, 320, 192
    sc = Scene(gs, ob, device, stream, 0, 0, n, W, H)
    hidden = np.random.default_rng(4).random(n) < 0.5
    hs = sc.selection(hidden)
    r = gs.Renderer(device)
    fr = sc.render(r, hide=hs)
    _check_hidden_frame(sc, r, fr, hidden)
    order0 = sc.order()
    m = n // 2                                    # more than a quarter of the buffer: the next frame re-sorts
    g2 = synth.scene(m, first=99)
    sc.g[:m] = g2
    sc.pods = sc.pod.from_gaussian(sc.g)
    sc.buf.update_range(stream, 0, g2)
    fr = sc.render(r, hide=hs)
    assert not np.array_equal(sc.order(), order0), "the mirror order should have been rebuilt"
    _check_hidden_frame(sc, r, fr, hidden)
    r.destroy(); hs.destroy(); sc.release()


def test_hide_with_aux_planes(gs, ob, device, stream):
    n, W, H = 30_000, 333, 197
    sc = Scene(gs, ob, device, stream, 0, 0, n, W, H)
    hidden = np.random.default_rng(6).random(n) < 0.5
    hs = sc.selection(hidden)
    depth = gs.Buffer(device, data=np.full(H * W, f32(np.nan)))
    pick = gs.Buffer(device, data=np.full(H * W, 0xDEADBEEF, dtype=np.uint32))
    r = gs.Renderer(device)
    fr = sc.render(r, hide=hs, depth_device_ptr=depth.device_ptr(), pick_device_ptr=pick.device_ptr())
    o = _check_hidden_frame(sc, r, fr, hidden)
    p = o["proj"].copy()
    p["r"], p["g"], p["b"] = p["depth"], 0.0, 0.0
    cam0 = ob.Camera.from_buffer_copy(bytes(sc.ocam))
    cam0.background[:] = [0.0, 0.0, 0.0]
    o_depth = ob.blend(p, o["idx"], o["ranges"], cam0, gt=sc.ogt)[..., 0]
    assert np.array_equal(bits(depth.download(stream, f32).reshape(H, W)), bits(o_depth))
    pk = pick.download(stream, np.uint32)
    picked = pk[pk != gs.PICK_NONE]
    assert len(picked) and (picked < n).all() and not hidden[picked].any(), "pick names a hidden Gaussian"
    depth.release(); pick.release(); r.destroy(); hs.destroy(); sc.release()


# ------------------------------------------------------------------------------------------------
# 6. tint
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", [(0, 0), (3, 0)])
def test_tint(gs, ob, device, stream, sh, cov):
    n, W, H = 30_001, 333, 197
    sc = Scene(gs, ob, device, stream, sh, cov, n, W, H)
    rng = np.random.default_rng(8)
    tinted, hidden = rng.random(n) < 0.5, rng.random(n) < 0.2
    ts, hs = sc.selection(tinted), sc.selection(hidden)
    r = gs.Renderer(device)
    plain = gs.Renderer(device)
    sc.render(plain)
    img_plain = sc.image()
    proj_plain, tiles_plain = plain.download_projected(n)
    for rgba in [(1.0, 0.25, 0.0, 0.5), (0.3, 0.7, 0.9, 0.37), (0.3, 0.7, 0.9, 1.0), (0.3, 0.7, 0.9, 0.0)]:
        def recolour(p, rgba=rgba, sel=tinted):
            for ch, t in zip("rgb", rgba[:3]):
                p[ch][sel] = tint32(p[ch][sel], rgba[3], t)
        o = sc.oracle(sc.pods, recolour=recolour)
        sc.poison()
        sc.render(r, tint=ts, tint_rgba=rgba)
        proj, tiles = r.download_projected(n)
        keep = tiles > 0
        assert np.array_equal(tiles, o["tiles"])
        assert np.array_equal(proj[keep].tobytes(), o["proj"][keep].tobytes()), rgba
        assert np.array_equal(bits(sc.image()), bits(o["rgba"])), rgba
        if rgba[3] == 0.0:
            assert np.array_equal(bits(sc.image()), bits(img_plain))
            assert np.array_equal(proj[keep].tobytes(), proj_plain[keep].tobytes())
        if rgba[3] == 1.0:
            for ch, t in zip("rgb", rgba[:3]):
                assert (proj[ch][keep & tinted] == f32(t)).all()
                assert np.array_equal(proj[ch][keep & ~tinted], proj_plain[ch][keep & ~tinted])
    # hide wins over tint
    rgba = (1.0, 0.25, 0.0, 0.5)

    def recolour(p):
        for ch, t in zip("rgb", rgba[:3]):
            p[ch][tinted] = tint32(p[ch][tinted], rgba[3], t)
    o = sc.oracle(sc.twin_pods(hidden), recolour=recolour)
    sc.poison()
    fr = sc.render(r, hide=hs, tint=ts, tint_rgba=rgba)
    assert fr.visible == int((o["tiles"] > 0).sum())
    assert np.array_equal(bits(sc.image()), bits(o["rgba"]))
    proj, tiles = r.download_projected(n)
    assert not tiles[hidden].any() and np.array_equal(tiles, o["tiles"])
    r.destroy(); plain.destroy(); ts.destroy(); hs.destroy(); sc.release()


# ------------------------------------------------------------------------------------------------
# 7. plain case, 8. errors, 9. un-hiding
# ------------------------------------------------------------------------------------------------

def _render_sel_raw(gs, sc, r, fs, aux=None):
    return gs._L.gs_render_frame_sel(r._h, sc.stream._h, sc.buf._h, gs.C.byref(sc.gt), gs.C.byref(sc.mt), gs.C.byref(sc.cam),
                                     0, 0xFFFFFFFF, sc.img.device_ptr(), gs.C.byref(aux) if aux is not None else None,
                                     gs.C.byref(fs) if fs is not None else None)


def test_plain_case_is_the_aux_frame(gs, ob, device, stream):
    """two renderers in lock step (the same history, hence the same plan): r0 renders plain frames, r1 the variant"""
    n, W, H = 30_000, 333, 197
    sc = Scene(gs, ob, device, stream, 0, 0, n, W, H)
    ref = gs.Buffer(device, size=W * H * 16)
    r0, r1 = gs.Renderer(device), gs.Renderer(device)
    hs = gs.Selection(device, n)                    # empty: the same image through the mask path
    # (variant, launches beyond the plain frame's): no struct; a struct without selections; the empty selection, whose
    # slot mask is gathered once; the unchanged selection again: nothing more
    for variant, extra in [(None, 0), (gs.FrameSelection(), 0), ("hide", 1), ("hide", 0), ("hide", 0)]:
        f0 = r0.render(stream, sc.buf, sc.gt, sc.mt, sc.cam, ref.device_ptr())
        img0 = ref.download(stream, f32).reshape(H, W, 4)
        sc.poison()
        if variant == "hide":
            f1 = sc.render(r1, hide=hs)
        else:
            gs._check(_render_sel_raw(gs, sc, r1, variant))
            f1 = r1.wait_frame()
        assert f1.launches == f0.launches + extra, (variant, f1.launches, f0.launches)
        assert f1.pairs == f0.pairs and f1.visible == f0.visible
        assert np.array_equal(bits(sc.image()), bits(img0))
    ref.release(); r0.destroy(); r1.destroy(); hs.destroy(); sc.release()


def test_argument_errors_enqueue_nothing(gs, ob, device, stream):
    n, W, H = 5_000, 96, 64
    sc = Scene(gs, ob, device, stream, 0, 0, n, W, H)
    r = gs.Renderer(device)
    good, short = gs.Selection(device, n), gs.Selection(device, n - 1)
    sc.poison()
    bad = []
    fs = gs.FrameSelection(); fs.hide = good._h; fs.reserved[1] = 1; bad.append(fs)
    fs = gs.FrameSelection(); fs.reserved[0] = 7; bad.append(fs)
    fs = gs.FrameSelection(); fs.hide = short._h; bad.append(fs)
    fs = gs.FrameSelection(); fs.tint = short._h; fs.tint_rgba[:] = (1, 1, 1, 0.5); bad.append(fs)
    for rgba in [(np.nan, 0, 0, 0.5), (0, np.inf, 0, 0.5), (0, 0, 0, -0.1), (0, 0, 0, 1.5), (0, 0, 0, np.nan)]:
        fs = gs.FrameSelection(); fs.tint = good._h; fs.tint_rgba[:] = rgba; bad.append(fs)
    for fs in bad:
        with pytest.raises(gs.InvalidArgumentError):
            gs._check(_render_sel_raw(gs, sc, r, fs))
    stream.synchronize()
    assert np.isnan(sc.image()).all(), "a refused frame must enqueue nothing"
    with pytest.raises(gs.InvalidArgumentError):
        r.select_visible(stream, good, 0, 0, W, H)         # still no last frame
    r.destroy(); good.destroy(); short.destroy(); sc.release()


def test_unhiding_after_mostly_hidden_frames(gs, ob, device, stream):
    n, W, H = 60_000, 480, 270
    sc = Scene(gs, ob, device, stream, gs.SH_NONE, 0, n, W, H, first=5)
    plain = gs.Renderer(device)
    fp = sc.render(plain)
    want = sc.image()
    hidden = np.random.default_rng(11).random(n) < 0.95
    hs = sc.selection(hidden)
    r = gs.Renderer(device)
    for _ in range(3):
        fr = sc.render(r, hide=hs)
    assert fr.pairs < fp.pairs // 4
    hs.clear(stream)
    sc.poison()
    fr = sc.render(r, hide=hs, check=True)
    assert fr.flags == 0 and fr.pairs == fp.pairs and fr.visible == fp.visible
    assert np.array_equal(bits(sc.image()), bits(want))
    r.destroy(); plain.destroy(); hs.destroy(); sc.release()
