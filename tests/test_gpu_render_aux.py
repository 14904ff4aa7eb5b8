"""Depth and pick planes (gs_render_frame_aux): written by the blend launch of the frame itself.
The colour must be the plain frame's and the oracle's bit for bit; the depth plane must be, bit for bit, the R channel
of the oracle's blend with every splat's r replaced by its view depth z' (g = b = 0, no background); the pick plane is
checked against the exact alpha relation, the tile lists and a float64 walk of every pixel's list."""
import hashlib

import numpy as np
import pytest

import helpers
import synth
from frames import frame_setup
from helpers import band_rows, bits, deep_scene
from planes import POISON_PICK, Planes, oracle_depth, pick_witness

pytestmark = pytest.mark.gpu

PODS = [(0, 0), (3, 0)]          # (sh, cov): SH3 f32 + rot-scale, SH-none + rot-scale


def _scene(gs, ob, sh, cov, n, W, H, mode=0, first=7, **cam_kw):
    return frame_setup(gs, ob, synth.scene(n, first=first), W, H, sh, cov, mode, sh_deg=3 if sh != gs.SH_NONE else 0, **cam_kw)


def _oracle(ob, sh, cov, pods, ogt, omt, ocam, order, band=None):
    proj, tiles = ob.preprocess(sh, cov, pods, ogt, omt, ocam, band=band)
    tiles_x, tiles_y = (ocam.width + 15) // 16, (ocam.height + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=ogt)
    return rgba, oracle_depth(ob, proj, sidx, ranges, ocam, ogt, band)


@pytest.mark.parametrize("sh,cov", PODS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_aux_colour_unchanged_and_depth_exact(gs, ob, device, stream, mode, sh, cov):
    W, H = 333, 197
    pod, pods, ogt, omt, ocam, gt, mt, cam = _scene(gs, ob, sh, cov, 30000, W, H, mode=mode)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    order = buf.download_order(stream)
    for band in (None, (3, 9)):
        o_rgba, o_depth = _oracle(ob, sh, cov, pods, ogt, omt, ocam, order, band)
        y0, y1 = band_rows(band, H)
        plain = gs.Buffer(device, size=W * H * 16)
        r_plain, r_aux = gs.Renderer(device), gs.Renderer(device)
        fr_plain = r_plain.render(stream, buf, gt, mt, cam, plain.device_ptr(), band=band)
        rgba_plain = plain.download(stream, np.float32).reshape(H, W, 4)
        pl = Planes(gs, device, W, H)
        fr_aux = pl.render(r_aux, stream, buf, gt, mt, cam, band=band)
        rgba, depth, pick = pl.get(stream)
        assert fr_aux.launches == fr_plain.launches, "the planes ride in the blend launch"
        assert np.array_equal(bits(rgba[y0:y1]), bits(rgba_plain[y0:y1])), "aux frame colour != plain frame colour"
        assert np.array_equal(bits(rgba[y0:y1]), bits(o_rgba[y0:y1])), "aux frame colour != oracle"
        bad = bits(depth[y0:y1]) != bits(o_depth[y0:y1])
        assert not bad.any(), "depth differs from the oracle at %d pixels, first %s: %s vs %s" % (
            bad.sum(), np.argwhere(bad)[0], depth[y0:y1][bad][:3], o_depth[y0:y1][bad][:3])
        # rows outside the band keep the poison
        outside = np.ones(H, bool)
        outside[y0:y1] = False
        assert np.isnan(depth[outside]).all() and (pick[outside] == POISON_PICK).all()
        # pick: exact relation to the alpha (1 - T is exact for T >= 0.5)
        assert np.array_equal(pick[y0:y1] != gs.PICK_NONE, rgba[y0:y1, :, 3] >= 0.5)
        # a pixel without contributors has depth 0
        assert (depth[y0:y1][rgba[y0:y1, :, 3] == 0.0] == 0.0).all()
        pl.release(); plain.release(); r_plain.destroy(); r_aux.destroy()
    buf.destroy()


def _check_pick_pairs(gs, r, pick, W, H, n):
    """every picked index is a visible Gaussian whose emitted pairs include the pixel's tile (single-round taps)"""
    proj, tiles = r.download_projected(n)
    _, sidx = r.download_sorted()
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    ranges = r.download_ranges(tiles_x * tiles_y)
    picked = pick != gs.PICK_NONE
    assert (pick[picked] < n).all()
    assert (tiles[pick[picked]] > 0).all(), "a picked Gaussian is not visible"
    pair_tile = np.repeat(np.arange(tiles_x * tiles_y), (ranges[:, 1] - ranges[:, 0]).astype(np.int64))
    have = set((pair_tile.astype(np.uint64) << np.uint64(32) | sidx.astype(np.uint64)).tolist())
    yy, xx = np.nonzero(picked)
    tile_of = (yy // 16) * tiles_x + xx // 16
    want = (tile_of.astype(np.uint64) << np.uint64(32)) | pick[yy, xx].astype(np.uint64)
    assert all(k in have for k in want.tolist()), "a picked Gaussian has no pair for the pixel's tile"
    return proj, sidx, ranges


@pytest.mark.parametrize("threshold", [0.5, 1.0 / 255.0])
def test_aux_pick_matches_a_float64_walk(gs, ob, device, stream, threshold):
    W, H = 333, 197
    sh, cov = 3, 0
    pod, pods, ogt, omt, ocam, gt, mt, cam = _scene(gs, ob, sh, cov, 30000, W, H)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    r = gs.Renderer(device)
    pl = Planes(gs, device, W, H)
    pl.render(r, stream, buf, gt, mt, cam, threshold=threshold)
    rgba, depth, pick = pl.get(stream)
    n = buf.len()
    proj, sidx, ranges = _check_pick_pairs(gs, r, pick, W, H, n)
    tiles_x = (W + 15) // 16
    picked = pick != gs.PICK_NONE
    # the float64 walk agrees wherever it is unambiguous
    tcut = np.float32(1.0) - np.float32(threshold)
    w_pick, amb = pick_witness(proj, sidx, ranges, W, H, tiles_x, float(tcut))
    assert amb.mean() <= 1e-3, "%.4f %% ambiguous pixels" % (100 * amb.mean())
    bad = (w_pick != pick.astype(np.uint64)) & ~amb
    assert not bad.any(), "pick differs from the float64 walk at %d pixels, first %s: %s vs %s" % (
        bad.sum(), np.argwhere(bad)[0], pick[bad][:3], w_pick[bad][:3])
    if threshold < 0.5:
        # the first contributor: a pixel with any alpha has a pick
        assert np.array_equal(picked, rgba[..., 3] > 0.0)
    pl.release(); r.destroy(); buf.destroy()


def test_aux_invalid_arguments(gs, ob, device, stream):
    W, H = 64, 48
    pod, pods, ogt, omt, ocam, gt, mt, cam = _scene(gs, ob, 3, 0, 2000, W, H)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    r = gs.Renderer(device)
    pl = Planes(gs, device, W, H)
    # (1e-9, 2^-25: 1 - t rounds to 1 in f32, a cut no step can cross)
    for t in (0.0, 1.0, -0.1, float("nan"), 1.5, 1e-9, 2.0 ** -25, float(np.finfo(np.float32).tiny)):
        with pytest.raises(gs.InvalidArgumentError):
            pl.render(r, stream, buf, gt, mt, cam, threshold=t)
    with pytest.raises(gs.InvalidArgumentError):      # misaligned plane
        r.render(stream, buf, gt, mt, cam, pl.img.device_ptr(), depth_device_ptr=pl.depth.device_ptr() + 2)
    with pytest.raises(gs.InvalidArgumentError):      # reserved must be 0
        aux = gs.AuxTargets(None, pl.pick.device_ptr(), 0.5, 1)
        gs._check(gs._capi.load().gs_render_frame_aux(r._h, stream._h, buf._h, gs.C.byref(gt), gs.C.byref(mt),
                                                      gs.C.byref(cam), 0, 0xFFFFFFFF, pl.img.device_ptr(),
                                                      gs.C.byref(aux)))
    # nothing was enqueued: the planes still hold the poison
    _, depth, pick = pl.get(stream)
    assert np.isnan(depth).all() and (pick == POISON_PICK).all()
    # one plane alone
    pl.render(r, stream, buf, gt, mt, cam)
    rgba, depth, pick = pl.get(stream)
    r2 = gs.Renderer(device)
    pl2 = Planes(gs, device, W, H)
    r2.render(stream, buf, gt, mt, cam, pl2.img.device_ptr(), pick_device_ptr=pl2.pick.device_ptr())
    rgba2, depth2, pick2 = pl2.get(stream)
    assert np.array_equal(pick2, pick) and np.isnan(depth2).all() and np.array_equal(bits(rgba2), bits(rgba))
    # the smallest thresholds that are accepted pick the first contributor, as 1/255 does
    firsts = []
    for t in (1.0 / 255.0, 2.0 ** -24, float(np.nextafter(np.float32(2.0 ** -25), np.float32(1.0)))):
        pl2.poison(stream)
        pl2.render(r2, stream, buf, gt, mt, cam, threshold=t)
        rgba2, _, pick2 = pl2.get(stream)
        assert np.array_equal(pick2 != gs.PICK_NONE, rgba2[..., 3] > 0.0), t
        firsts.append(pick2)
    assert all(np.array_equal(f, firsts[0]) for f in firsts)
    # a zero-initialised gs_aux_targets (no planes, threshold 0) is the plain frame
    pl2.poison(stream)
    gs._check(gs._capi.load().gs_render_frame_aux(r2._h, stream._h, buf._h, gs.C.byref(gt), gs.C.byref(mt), gs.C.byref(cam),
                                                  0, 0xFFFFFFFF, pl2.img.device_ptr(), gs.C.byref(gs.AuxTargets())))
    assert r2.wait_frame().flags == 0
    rgba2, depth2, pick2 = pl2.get(stream)
    assert np.array_equal(bits(rgba2), bits(rgba)) and np.isnan(depth2).all() and (pick2 == POISON_PICK).all()
    pl.release(); pl2.release(); r.destroy(); r2.destroy(); buf.destroy()


def test_aux_pick_is_a_caller_index(gs, ob, device, stream):
    """spatial order on / off, and a renderer in block-list mode (its per-slot arrays in list space): the same planes"""
    n, W, H = 90_000, 320, 192
    g = synth.scene(n, first=4242)
    pod = gs.GaussianPod(1, 0)
    pods = pod.from_gaussian(g)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    views = {"all": ((0, 0, 12), (0, 0, -14), 70.0), "corner": ((0, 0, 0), (13, 7, -3), 25.0)}
    cams = {k: gs.camera_look_at(e, t, (0, 1, 0), float(np.deg2rad(f)), W, H, 0.1, 100.0) for k, (e, t, f) in views.items()}
    res = {}
    for spatial in (True, False):
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
        buf.set_spatial_order(spatial)
        assert buf.spatial_order() == spatial
        r = gs.Renderer(device)
        pl = Planes(gs, device, W, H)
        # all -> corner (the test inside the preprocess kernel) -> corner (block list: the previous frame saw < n / 2)
        for k, name in enumerate(["all", "corner", "corner"]):
            pl.poison(stream)
            fr = pl.render(r, stream, buf, gt, mt, cams[name])
            planes = pl.get(stream)
            _check_pick_pairs(gs, r, planes[2], W, H, n)
            res[(spatial, k)] = (fr.launches, planes)
        pl.release(); r.destroy(); buf.destroy()
    assert res[(True, 2)][0] == res[(True, 1)][0] + 1, "the second corner frame should take the block list"
    for key in res:
        ref = res[(True, 0 if key[1] == 0 else 1)][1]
        for a, b in zip(res[key][1], ref):
            assert np.array_equal(bits(a), bits(b)), key
    assert (res[(True, 1)][1][2] != gs.PICK_NONE).any() and (res[(True, 0)][1][2] != gs.PICK_NONE).any()


def test_aux_two_rounds_equal_one_round(gs, ob, device, stream):
    W, H = 640, 360
    sh, cov = gs.SH_NONE, gs.COV3D_ROT_SCALE
    g = deep_scene(200_000)
    pod = gs.GaussianPod(sh, cov)
    pods = pod.from_gaussian(g)
    gt = gs.gaussian_transform_pod(1.0, 0, 0, False, 3.0)
    mt = gs.model_transform_pod()
    cam = helpers.copy_camera(helpers.default_camera(ob, W, H), gs.Camera)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    r = gs.Renderer(device)
    r.set_rounds(0)
    pl = Planes(gs, device, W, H)
    pl.render(r, stream, buf, gt, mt, cam)
    ref = pl.get(stream)
    assert r.sort_info().rounds == 1
    for band in (None, (4, 17)):
        y0, y1 = band_rows(band, H)
        for k in (5_000, 30_000, 120_000):
            r2 = gs.Renderer(device)
            r2.set_rounds(1, k)
            for frame in range(2):      # the second frame is partitioned
                pl.poison(stream)
                pl.render(r2, stream, buf, gt, mt, cam, band=band)
                assert r2.sort_info().rounds == 2
                rgba, depth, pick = pl.get(stream)
                ctx = (band, k, frame)
                assert np.array_equal(bits(rgba[y0:y1]), bits(ref[0][y0:y1])), ctx
                assert np.array_equal(bits(depth[y0:y1]), bits(ref[1][y0:y1])), ctx
                assert np.array_equal(pick[y0:y1], ref[2][y0:y1]), ctx
                if band is not None:
                    assert np.isnan(depth[:y0]).all() and (pick[y1:] == POISON_PICK).all(), ctx
            r2.destroy()
    pl.release(); r.destroy(); buf.destroy()


def test_aux_skipped_frame_leaves_the_planes(gs, ob, device, stream):
    """far-then-near: the near frame outgrows the pair capacity and is skipped; its planes stay untouched"""
    g = synth.scene(60000, first=5)
    pod = gs.GaussianPod(gs.SH_NONE, gs.COV3D_ROT_SCALE)
    pods = pod.from_gaussian(g)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    W, H = 960, 540
    gt, mt = gs.gaussian_transform_pod(sh_deg=0), gs.model_transform_pod()
    gt_big = gs.gaussian_transform_pod(size=4.0, sh_deg=0)
    far_cam = helpers.default_camera(gs, W, H, eye=(0.0, 0.0, 60.0), target=(0.0, 0.0, 0.0))
    near_cam = helpers.default_camera(gs, W, H)
    ref_r = gs.Renderer(device)
    ref = Planes(gs, device, W, H)
    ref.render(ref_r, stream, buf, gt_big, mt, near_cam)
    want = ref.get(stream)
    r = gs.Renderer(device)
    pl = Planes(gs, device, W, H)
    pl.render(r, stream, buf, gt, mt, far_cam)
    far = pl.get(stream)
    pl.render(r, stream, buf, gt_big, mt, near_cam, check=False)
    with pytest.raises(gs.PairCapacityError):
        r.wait_frame()
    got = pl.get(stream)
    for a, b in zip(got, far):
        assert np.array_equal(bits(a), bits(b)), "a skipped frame must leave the planes untouched"
    pl.render(r, stream, buf, gt_big, mt, near_cam, check=False)
    assert r.wait_frame().flags == 0
    got = pl.get(stream)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))
    pl.release(); ref.release(); r.destroy(); ref_r.destroy(); buf.destroy()


def test_aux_frame_ring(gs, ob, device, stream):
    """three frames in flight, each lane with its own planes: every lane's planes are the lone renderer's"""
    W, H = 480, 270
    g = synth.scene(200_000, first=11)
    pod = gs.GaussianPod(gs.SH_NONE, gs.COV3D_ROT_SCALE)
    pods = pod.from_gaussian(g)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    gt, mt = gs.gaussian_transform_pod(sh_deg=0), gs.model_transform_pod()
    cams = [helpers.default_camera(gs, W, H, eye=(0.2 * k, 0.0, 0.5 * k), target=(0.1 * k, 0.0, -5.0)) for k in range(6)]
    want = []
    for cam in cams:
        r = gs.Renderer(device)
        pl = Planes(gs, device, W, H)
        pl.render(r, stream, buf, gt, mt, cam)
        want.append(pl.get(stream))
        pl.release(); r.destroy()
    ring = gs.FrameRing(device, 3)
    lanes = [Planes(gs, device, W, H) for _ in range(3)]
    for rep in range(2):        # the first pass sizes every lane's buffers; the second runs with frames in flight
        got = []
        for k, cam in enumerate(cams):
            lane = k % 3
            if k >= 3:
                ring.streams[lane].synchronize()
                got.append(lanes[lane].get(ring.streams[lane]))
            ring.render(buf, gt, mt, cam, lanes[lane].img.device_ptr(), check=rep == 0,
                        depth_device_ptr=lanes[lane].depth.device_ptr(), pick_device_ptr=lanes[lane].pick.device_ptr())
        ring.synchronize()
        for lane in range(3):
            got.append(lanes[lane].get(ring.streams[lane]))
        ring.wait()
        for k, (a, b) in enumerate(zip(got, want)):
            for x, y in zip(a, b):
                assert np.array_equal(bits(x), bits(y)), (rep, k)
    for pl in lanes:
        pl.release()
    ring.close(); buf.destroy()


def test_aux_at_scale(gs, ob, device, stream):
    """1 M Gaussians at 1080p under the renderer's own policy: the aux colour is the plain frame's, the depth the oracle's"""
    n, W, H = 1_000_000, 1920, 1080
    sh, cov = gs.SH_NONE, gs.COV3D_ROT_SCALE
    g = synth.scene(n)
    pod = gs.GaussianPod(sh, cov)
    pods = pod.from_gaussian(g)
    ogt, omt = ob.gaussian_transform(sh_deg=0), ob.model_transform()
    ocam = helpers.default_camera(ob, W, H)
    gt, mt = gs.GaussianTransformPod.from_buffer_copy(bytes(ogt)), gs.ModelTransformPod.from_buffer_copy(bytes(omt))
    cam = helpers.copy_camera(ocam, gs.Camera)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    order = buf.download_order(stream)
    plain = gs.Buffer(device, size=W * H * 16)
    r_plain, r_aux = gs.Renderer(device), gs.Renderer(device)
    r_plain.render(stream, buf, gt, mt, cam, plain.device_ptr())
    pl = Planes(gs, device, W, H)
    pl.render(r_aux, stream, buf, gt, mt, cam)
    h_plain = hashlib.sha256(plain.download(stream, np.uint8).tobytes()).hexdigest()
    h_aux = hashlib.sha256(pl.img.download(stream, np.uint8).tobytes()).hexdigest()
    assert h_aux == h_plain
    _, depth, pick = pl.get(stream)
    o_rgba, o_depth = _oracle(ob, sh, cov, pods, ogt, omt, ocam, order)
    rgba = plain.download(stream, np.float32).reshape(H, W, 4)
    assert np.array_equal(bits(rgba), bits(o_rgba))
    assert np.array_equal(bits(depth), bits(o_depth))
    assert np.array_equal(pick != gs.PICK_NONE, rgba[..., 3] >= 0.5)
    pl.release(); plain.release(); r_plain.destroy(); r_aux.destroy(); buf.destroy()
