"""Contribution scores (gs_render_frame_contrib, gs_contributions_clear, gs_select_contribution).

Every field of a record is an integer reduction, so the records are defined bit for bit: they are compared, as raw 16-byte
rows, with the expectation that tests/contrib_np.py derives from the frozen oracle's blend."""
import os

import numpy as np
import pytest

import contrib_np as cn
import gpu_child
import helpers
from frames import frame_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PODS = [(0, 0), (3, 0)]          # (sh, cov): SH f32 + rot-scale (sh_deg = 0), SH-none + rot-scale
W, H = cn.SCENE_A_SIZE
N = 2500


class SceneA:
    """scene A on the device, with the oracle's sorted frame and the expectation of one camera / band / hide set"""

    def __init__(self, gs, ob, device, stream, sh, cov, mode=0, **cam_kw):
        self.gs, self.ob, self.device, self.sh, self.cov = gs, ob, device, sh, cov
        self.pod, self.pods, self.ogt, self.omt, self.ocam, self.gt, self.mt, self.cam = frame_setup(
            gs, ob, cn.scene_a(), *cn.SCENE_A_SIZE, sh, cov, mode=mode, **cam_kw)
        self.buf = gs.GaussiansBuffer.new_with_pods(device, self.pod, self.pods)
        self.order = self.buf.download_order(stream)
        self.img = gs.Buffer(device, data=np.full(H * W * 4, helpers.POISON))

    def oracle(self, band=None, hidden=None):
        """(frame, expectation, oracle image) of this camera"""
        ob = self.ob
        frame = cn.sorted_frame(ob, self.sh, self.cov, self.pods, self.ogt, self.omt, self.ocam, self.order, band=band, hidden=hidden)
        proj, tiles, skeys, sidx, ranges = frame
        exp = cn.expectation(ob, proj, tiles, skeys, sidx, ranges, self.ocam, self.ogt, band=band)
        rgba = ob.blend(proj, sidx, ranges, self.ocam, band=band, gt=self.ogt)
        return frame, exp, rgba

    def render(self, r, stream, contrib, **kw):
        fr = r.render(stream, self.buf, self.gt, self.mt, self.cam, self.img.device_ptr(), contributions=contrib, **kw)
        stream.synchronize()
        return fr

    def image(self, stream):
        return self.img.download(stream, np.float32).reshape(H, W, 4).copy()

    def release(self):
        self.img.release()
        self.buf.destroy()


def _same(got, want, what=""):
    bad = (cn.raw(got) != cn.raw(want)).any(axis=1)
    assert not bad.any(), "%s: %d records differ, first %d: got %s, want %s" % (
        what, int(bad.sum()), int(np.flatnonzero(bad)[0]), got[bad][:3], want[bad][:3])


def _arbitrary(n, seed):
    """nonzero records, a few with hits about to wrap"""
    rng = np.random.default_rng(seed)
    rec = cn.zero_records(n)
    rec["sum"] = rng.integers(1, 1 << 40, n, dtype=np.uint64)
    rec["hits"] = rng.integers(1, 1 << 20, n, dtype=np.uint32)
    rec["hits"][::97] = np.uint32(0xFFFFFFFE)
    rec["wmax"] = rng.uniform(1e-3, 0.6, n).astype(np.float32)
    return rec


@pytest.mark.parametrize("sh,cov", PODS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scene_a_records_exact(gs, ob, device, stream, mode, sh, cov):
    sc = SceneA(gs, ob, device, stream, sh, cov, mode)
    (proj, tiles, skeys, sidx, ranges), exp, o_rgba = sc.oracle()
    cn.assert_scene_a_conditions(ob, tiles, skeys, sidx, ranges, sc.ocam, sc.ogt, proj, sc.order, exp)
    r_plain, r = gs.Renderer(device), gs.Renderer(device)
    fr_plain = r_plain.render(stream, sc.buf, sc.gt, sc.mt, sc.cam, sc.img.device_ptr())
    plain = sc.image(stream)
    sc.img.write(stream, 0, np.full(H * W * 4, helpers.POISON))
    c = gs.Contributions.new(device, stream, N)
    fr = sc.render(r, stream, c)
    got = c.download(stream)
    rgba = sc.image(stream)
    print("visible %d pairs %d hits %d zero-hit visible %d" % (int((np.asarray(tiles) > 0).sum()), len(sidx), int(exp["hits"].sum()),
                                                              int(((np.asarray(tiles) > 0) & (exp["hits"] == 0)).sum())))
    _same(got, exp, "mode %d" % mode)
    zero = exp["hits"] == 0
    assert zero.any() and not cn.raw(got)[zero].any(), "culled and zero-hit records are 16 zero bytes"
    assert np.array_equal(helpers.bits(rgba), helpers.bits(plain)), "contribution frame colour != plain frame colour"
    assert np.array_equal(helpers.bits(rgba), helpers.bits(o_rgba)), "contribution frame colour != oracle"
    assert fr.launches == fr_plain.launches, "the accumulation rides in the blend launch"
    c.release(); r.destroy(); r_plain.destroy(); sc.release()


def test_accumulates_and_clear(gs, ob, device, stream):
    sc1 = SceneA(gs, ob, device, stream, 3, 0)
    sc2 = SceneA(gs, ob, device, stream, 3, 0, eye=(0.3, 0.1, 0.5), target=(0.2, 0.0, -1.0))
    _, exp1, _ = sc1.oracle()
    _, exp2, _ = sc2.oracle()
    assert (cn.raw(exp1) != cn.raw(exp2)).any()
    pre = _arbitrary(N, 1)
    guard = np.full(256, 0xA5, np.uint8)
    store = gs.Buffer(device, data=np.concatenate([pre.view(np.uint8), guard]))
    c = gs.Contributions(device, N, buffer=store)
    r = gs.Renderer(device)
    sc1.render(r, stream, c)
    sc2.render(r, stream, c)
    _same(c.download(stream), cn.combine(cn.combine(pre, exp1), exp2), "pre-fill (+) two frames")
    c.clear(stream)
    stream.synchronize()
    whole = store.download(stream, np.uint8)
    assert not whole[:16 * N].any() and np.array_equal(whole[16 * N:], guard), "clear zeroes exactly 16 n bytes"
    c.release(); r.destroy(); sc1.release(); sc2.release()


def test_bands_add_up_to_the_full_frame(gs, ob, device, stream):
    sc = SceneA(gs, ob, device, stream, 3, 0)
    _, exp, _ = sc.oracle()
    c = gs.Contributions.new(device, stream, N)
    r = gs.Renderer(device)
    sc.render(r, stream, c, band=(0, 2))
    sc.render(r, stream, c, band=(2, 4))
    _same(c.download(stream), exp, "two bands")
    c.release(); r.destroy(); sc.release()


def test_hidden_gaussians_contribute_nothing(gs, ob, device, stream):
    sc = SceneA(gs, ob, device, stream, 3, 0)
    hidden = np.arange(N) % 3 == 0
    _, exp, o_rgba = sc.oracle(hidden=hidden)
    assert not exp["hits"][hidden].any() and exp["hits"][~hidden].any()
    sel = gs.Selection(device, N)
    sel.upload(stream, hidden)
    pre = _arbitrary(N, 2)
    c = gs.Contributions(device, N, buffer=gs.Buffer(device, data=pre))
    r = gs.Renderer(device)
    sc.render(r, stream, c, hide=sel)
    got = c.download(stream)
    assert np.array_equal(cn.raw(got)[hidden], cn.raw(pre)[hidden]), "hidden records stay untouched"
    _same(got, cn.combine(pre, exp), "hide")
    assert np.array_equal(helpers.bits(sc.image(stream)), helpers.bits(o_rgba))
    c.release(); r.destroy(); sel.destroy(); sc.release()


def test_skipped_frame_leaves_the_records(gs, ob, device, stream):
    """far-then-near: the near frame outgrows the pair capacity and is skipped; its records stay untouched"""
    import synth
    g = synth.scene(60000, first=5)
    n = len(g)
    pod = gs.GaussianPod(gs.SH_NONE, gs.COV3D_ROT_SCALE)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod.from_gaussian(g))
    w, h = 960, 540
    gt, mt = gs.gaussian_transform_pod(sh_deg=0), gs.model_transform_pod()
    gt_big = gs.gaussian_transform_pod(size=4.0, sh_deg=0)
    far_cam = helpers.default_camera(gs, w, h, eye=(0.0, 0.0, 60.0), target=(0.0, 0.0, 0.0))
    near_cam = helpers.default_camera(gs, w, h)
    img = gs.Buffer(device, size=w * h * 16)
    ref_r, ref_c = gs.Renderer(device), gs.Contributions.new(device, stream, n)
    ref_r.render(stream, buf, gt_big, mt, near_cam, img.device_ptr(), contributions=ref_c)
    near = ref_c.download(stream).copy()
    assert near["hits"].any()
    r, c = gs.Renderer(device), gs.Contributions.new(device, stream, n)
    r.render(stream, buf, gt, mt, far_cam, img.device_ptr(), contributions=c)
    far = c.download(stream).copy()
    assert far["hits"].any()
    r.render(stream, buf, gt_big, mt, near_cam, img.device_ptr(), contributions=c, check=False)
    with pytest.raises(gs.PairCapacityError):
        r.wait_frame()
    assert np.array_equal(cn.raw(c.download(stream)), cn.raw(far)), "a skipped frame must leave the records untouched"
    r.render(stream, buf, gt_big, mt, near_cam, img.device_ptr(), contributions=c, check=False)
    assert r.wait_frame().flags == 0
    _same(c.download(stream), cn.combine(far, near), "the retried frame")
    for x in (c, ref_c, img):
        x.release()
    r.destroy(); ref_r.destroy(); buf.destroy()


def test_contribution_frames_take_one_round(gs, ob, device, stream):
    w, h = 640, 360
    g = helpers.deep_scene(200_000)
    n = len(g)
    pod = gs.GaussianPod(gs.SH_NONE, gs.COV3D_ROT_SCALE)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod.from_gaussian(g))
    gt, mt = gs.gaussian_transform_pod(1.0, 0, 0, False, 3.0), gs.model_transform_pod()
    cam = helpers.copy_camera(helpers.default_camera(ob, w, h), gs.Camera)
    img = gs.Buffer(device, size=w * h * 16)
    r1 = gs.Renderer(device)
    r1.set_rounds(0)
    c1 = gs.Contributions.new(device, stream, n)
    r1.render(stream, buf, gt, mt, cam, img.device_ptr(), contributions=c1)
    assert r1.sort_info().rounds == 1
    want_img = img.download(stream, np.uint8).copy()
    r2 = gs.Renderer(device)
    r2.set_rounds(1, 30_000)
    c2 = gs.Contributions.new(device, stream, n)
    for _ in range(2):      # (the second frame is partitioned)
        r2.render(stream, buf, gt, mt, cam, img.device_ptr())
        assert r2.sort_info().rounds == 2
    r2.render(stream, buf, gt, mt, cam, img.device_ptr(), contributions=c2)
    assert r2.sort_info().rounds == 1, "a contribution frame is planned as one round"
    assert np.array_equal(img.download(stream, np.uint8), want_img)
    r2.render(stream, buf, gt, mt, cam, img.device_ptr())
    assert r2.sort_info().rounds == 2, "the renderer's pin is unchanged"
    got, want = c2.download(stream), c1.download(stream)
    assert want["hits"].any()
    _same(got, want, "pinned to two rounds vs pinned to one")
    for x in (c1, c2, img):
        x.release()
    r1.destroy(); r2.destroy(); buf.destroy()


def test_two_renderers_two_streams_one_buffer(gs, ob, device, stream):
    sc = SceneA(gs, ob, device, stream, 3, 0)
    _, exp, _ = sc.oracle()
    s1, s2 = device.create_stream(), device.create_stream()
    r1, r2 = gs.Renderer(device), gs.Renderer(device)
    img2 = gs.Buffer(device, size=W * H * 16)
    c = gs.Contributions.new(device, stream, N)
    # the first frame of a renderer sizes its buffers (blocking): done here, then the records are cleared
    r1.render(s1, sc.buf, sc.gt, sc.mt, sc.cam, sc.img.device_ptr(), contributions=c)
    r2.render(s2, sc.buf, sc.gt, sc.mt, sc.cam, img2.device_ptr(), contributions=c)
    c.clear(stream)
    stream.synchronize()
    r1.render(s1, sc.buf, sc.gt, sc.mt, sc.cam, sc.img.device_ptr(), contributions=c, check=False)
    r2.render(s2, sc.buf, sc.gt, sc.mt, sc.cam, img2.device_ptr(), contributions=c, check=False)
    assert r1.wait_frame().flags == 0 and r2.wait_frame().flags == 0
    s1.synchronize(); s2.synchronize()
    got = c.download(stream)
    want = cn.combine(exp, exp)
    assert np.array_equal(want["wmax"], exp["wmax"]) and np.array_equal(want["sum"], 2 * exp["sum"])
    _same(got, want, "two frames on two streams")
    c.release(); img2.release(); r1.destroy(); r2.destroy(); s1.close(); s2.close(); sc.release()


@pytest.mark.parametrize("groups", [1, 2, 4, 8])
def test_blend_groups_switch(gs, ob, device, stream, groups, tmp_path):
    """GS3D_BLEND_GROUPS is read once per process: a child per setting, one after the other"""
    want = []
    for mode in (0, 1, 2):
        sc = SceneA(gs, ob, device, stream, 3, 0, mode)
        want.append(sc.oracle()[1])
        sc.release()
    out = str(tmp_path / "records.npy")
    gpu_child.run([os.path.join(ROOT, "tests", "contrib_child.py"), out], env={"GS3D_BLEND_GROUPS": str(groups)}, timeout=300,
                  label="GS3D_BLEND_GROUPS=%d" % groups, expect="contrib_child OK")
    got = np.load(out)
    for mode in (0, 1, 2):
        _same(got[mode], want[mode], "GS3D_BLEND_GROUPS=%d mode %d" % (groups, mode))


def _values(rec, kind):
    if kind == 0:
        return rec["sum"].astype(np.float32) * np.float32(2.0 ** -24)      # u64 -> f32 to nearest even, exact scale
    if kind == 1:
        return rec["hits"].astype(np.float32)
    return rec["wmax"]


def _apply(old, hit, op):
    return [hit, old | hit, old & hit, old & ~hit, old ^ hit][op]


def test_select_contribution(gs, ob, device, stream):
    sc = SceneA(gs, ob, device, stream, 3, 0)
    _, exp, _ = sc.oracle()
    c = gs.Contributions.new(device, stream, N)
    r = gs.Renderer(device)
    sc.render(r, stream, c)
    rec = c.download(stream).copy()
    _same(rec, exp, "scene A")
    sel = gs.Selection(device, N)
    old = np.random.default_rng(3).random(N) < 0.5
    inf = float("inf")
    hit_vals = rec["hits"][rec["hits"] > 0]
    bounds = {0: [(0.0, 1.0), (float(np.median(_values(rec, 0))), inf), (-inf, inf), (2.0, 1.0), (-inf, 0.0)],
              1: [(0.0, 0.0), (1.0, float(np.median(hit_vals))), (-inf, inf), (5.0, 4.0), (float(hit_vals.max()), inf)],
              2: [(0.0, 0.5), (0.5, inf), (-inf, inf), (0.9, 0.1), (0.99, 0.99)]}
    for kind in (gs.CONTRIB_SUM, gs.CONTRIB_HITS, gs.CONTRIB_MAX):
        v = _values(rec, kind)
        for lo, hi in bounds[kind]:
            hit = (np.float32(lo) <= v) & (v <= np.float32(hi))
            if lo > hi:
                assert not hit.any()
            for op in range(5):
                sel.upload(stream, old)
                c.select(stream, sel, kind, lo, hi, op)
                got = sel.download(stream)
                assert np.array_equal(got, _apply(old, hit, op)), (kind, lo, hi, op)
                assert N % 32 and not (int(sel.download_words(stream)[-1]) >> (N % 32)), "tail bits stay 0"
    c.select(stream, sel, gs.CONTRIB_HITS, 0.0, 0.0)
    assert np.array_equal(sel.download(stream), exp["hits"] == 0), "HITS in [0, 0]: the Gaussians no pixel blends"
    assert (exp["hits"] == 0).any() and (exp["hits"] != 0).any()
    sel.destroy(); c.release(); r.destroy(); sc.release()


def test_invalid_arguments_touch_nothing(gs, ob, device, stream):
    sc = SceneA(gs, ob, device, stream, 3, 0)
    L, C = gs._L, gs.C
    pre = _arbitrary(N + 1, 4)
    store = gs.Buffer(device, data=pre)
    small = gs.Buffer.from_raw(device, store.device_ptr(), 16 * N - 1)
    odd = gs.Buffer.from_raw(device, store.device_ptr() + 4, 16 * N)
    r = gs.Renderer(device)
    img0 = sc.img.download(stream, np.uint8).copy()
    bad = gs.InvalidArgumentError.code

    def frame(cbuf):
        return L.gs_render_frame_contrib(r._h, stream._h, sc.buf._h, C.byref(sc.gt), C.byref(sc.mt), C.byref(sc.cam), 0, 0xFFFFFFFF,
                                         C.c_void_p(sc.img.device_ptr()), None, cbuf._h if cbuf is not None else None)

    def untouched():
        stream.synchronize()
        assert np.array_equal(store.download(stream, np.uint8), pre.view(np.uint8))
        assert np.array_equal(sc.img.download(stream, np.uint8), img0)

    for cbuf in (small, odd):
        assert frame(cbuf) == bad
        untouched()
        with pytest.raises(gs.InvalidArgumentError):
            r.render(stream, sc.buf, sc.gt, sc.mt, sc.cam, sc.img.device_ptr(), contributions=cbuf)
        assert L.gs_contributions_clear(cbuf._h, stream._h, N) == bad
        untouched()
    sel = gs.Selection(device, N)
    sel.upload(stream, np.arange(N) % 2 == 0)
    words0 = sel.download_words(stream).copy()

    def select(cbuf=store, s=sel, kind=0, lo=0.0, hi=1.0, op=0):
        return L.gs_select_contribution(s._h, stream._h, cbuf._h if cbuf is not None else None, kind, lo, hi, op)

    longer = gs.Selection(device, N + 2)       # length mismatch: 16 (N + 2) bytes are more than the buffer holds
    for kw in (dict(cbuf=small), dict(cbuf=odd), dict(lo=float("nan")), dict(hi=float("nan")), dict(kind=3), dict(kind=0xFFFFFFFF),
               dict(op=5), dict(op=-1), dict(s=longer), dict(cbuf=None)):
        assert select(**kw) == bad, kw
        untouched()
        assert np.array_equal(sel.download_words(stream), words0), kw
    with pytest.raises(ValueError):
        gs.Contributions(device, N, buffer=store).select(stream, longer, gs.CONTRIB_SUM, 0.0, 1.0)
    assert select() == 0        # ... and the valid call goes through
    longer.destroy(); sel.destroy(); r.destroy(); small.release(); odd.release(); store.release(); sc.release()


def test_at_scale(gs, ob, device, stream):
    """the bench's 1 M scene at 1080p under the renderer's own plan: structural checks and the conservation witness"""
    import synth
    n, w, h = 1_000_000, 1920, 1080
    pod = gs.GaussianPod(gs.SH_NONE, gs.COV3D_ROT_SCALE)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod.from_gaussian(synth.scene(n)))
    gt, mt = gs.gaussian_transform_pod(sh_deg=0), gs.model_transform_pod()
    cam = gs.camera_look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0, 1, 0), float(np.deg2rad(60.0)), w, h, 0.1, 100.0)
    img = gs.Buffer(device, size=w * h * 16)
    c = gs.Contributions.new(device, stream, n)
    r = gs.Renderer(device)
    r.render(stream, buf, gt, mt, cam, img.device_ptr(), contributions=c)
    one = c.download(stream).copy()
    rgba = img.download(stream, np.float32).reshape(h, w, 4)
    _, tiles = r.download_projected(n)
    assert (tiles == 0).any() and not cn.raw(one)[tiles == 0].any(), "Gaussians that touch no tile have zero records"
    assert one["hits"].any() and one["wmax"].max() <= np.float32(0.99)      # alpha <= 0.99f (binary32), T <= 1
    # conservation: per pixel the weights sum to 1 - T.  Per contribution at most two binary32 roundings of relative
    # magnitude 2^-24 on values <= 1 (T (1 - alpha), alpha T) and one truncation below 2^-24, plus the final 1 - T:
    # within 2^-21 per contribution
    total = float(one["sum"].astype(np.float64).sum() * 2.0 ** -24)
    alpha = float(rgba[..., 3].astype(np.float64).sum())
    bound = float(one["hits"].astype(np.float64).sum()) * 2.0 ** -21
    print("conservation: sum of weights %.6f, sum of alpha %.6f, difference %.3e, bound %.3e" % (total, alpha, abs(total - alpha), bound))
    assert abs(total - alpha) <= bound
    r.render(stream, buf, gt, mt, cam, img.device_ptr(), contributions=c)
    two = c.download(stream)
    assert np.array_equal(two["sum"], 2 * one["sum"]) and np.array_equal(two["hits"], 2 * one["hits"])
    assert np.array_equal(helpers.bits(two["wmax"]), helpers.bits(one["wmax"]))
    c.release(); img.release(); r.destroy(); buf.destroy()
