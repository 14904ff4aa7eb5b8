"""Frames the render tests share: the transforms and camera of a scene for oracle and product, one poisoned image rendered
and downloaded, and a whole frame compared stage by stage with the oracle."""
import numpy as np

import synth
from helpers import copy_camera, default_camera

RGBA_TOL = 1e-4  # BASELINE.json north_star: <= 1e-4 per channel


def frame_setup(gs, ob, g, W, H, sh, cov, mode=0, sh_deg=0, **cam_kw):
    """pods and the oracle's and the product's transforms and camera of a scene: the product's are the oracle's bytes"""
    pod = gs.GaussianPod(sh, cov)
    pods = pod.from_gaussian(g)
    ogt = ob.gaussian_transform(sh_deg=sh_deg, mode=mode)
    omt = ob.model_transform()
    ocam = default_camera(ob, W, H, **cam_kw)
    gt = gs.GaussianTransformPod.from_buffer_copy(bytes(ogt))
    mt = gs.ModelTransformPod.from_buffer_copy(bytes(omt))
    cam = copy_camera(ocam, gs.Camera)
    return pod, pods, ogt, omt, ocam, gt, mt, cam


def render_image(gs, device, stream, r, buf, gt, mt, cam, W, H, poison=np.float32(np.nan), **kw):
    """one frame into an image pre-filled with the poison (None: left as allocated); returns (rgba, the frame's result)"""
    img = gs.Buffer(device, size=H * W * 16) if poison is None else gs.Buffer(device, data=np.full(H * W * 4, np.float32(poison)))
    fr = r.render(stream, buf, gt, mt, cam, img.device_ptr(), **kw)
    stream.synchronize()
    out = img.download(stream, np.float32).reshape(H, W, 4).copy()
    img.release()
    return out, fr


def render_gpu(gs, device, stream, pod, pods, gt, mt, cam, band=None, renderer=None, sort_mode=None):
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    img = gs.Buffer(device, size=cam.height * cam.width * 16)
    r = renderer or gs.Renderer(device)
    if sort_mode is not None:
        r.set_sort_mode(*sort_mode)        # (depth, tile): 1 MSD-first, 0 LSD passes, -1 the renderer chooses
    r.render(stream, buf, gt, mt, cam, img.device_ptr(), band=band)
    stream.synchronize()
    rgba = img.download(stream, np.float32).reshape(cam.height, cam.width, 4)
    return r, buf, img, rgba


def mirror_order(ob, buf, stream, sh, cov, pods, fresh=True):
    """The buffer's mirror order, which the oracle needs for exact-depth ties.  For
    a freshly created buffer it must equal the oracle's own restatement of the spatial order."""
    order = buf.download_order(stream)
    assert np.array_equal(np.sort(order), np.arange(len(order), dtype=np.uint32)), "order is not a permutation"
    if fresh:
        exp = ob.spatial_order(sh, cov, pods) if buf.spatial_order() and len(order) > 1 else np.arange(
            len(order), dtype=np.uint32)
        assert np.array_equal(order, exp), "mirror order differs from the oracle's spatial order"
    return order


def oracle_stages(ob, sh, cov, pods, ogt, omt, ocam, band=None, order=None):
    proj, tiles = ob.preprocess(sh, cov, pods, ogt, omt, ocam, band=band)
    tiles_x = (ocam.width + 15) // 16
    tiles_y = (ocam.height + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=ogt)
    return proj, tiles, keys, idx, skeys, sidx, ranges, rgba


def compare_frame(gs, ob, device, stream, sh, cov, gaussians, W, H, gt_kw=None, mt_kw=None,
                   cam_kw=None, band=None, check_image_exact=True, sort_mode=None, info=None):
    gt_kw, mt_kw, cam_kw = gt_kw or {}, mt_kw or {}, cam_kw or {}
    pod = gs.GaussianPod(sh, cov)
    pods = pod.from_gaussian(gaussians)
    assert np.array_equal(pods, ob.pack(sh, cov, gaussians)), "product pack != oracle pack"
    ogt = ob.gaussian_transform(**gt_kw)
    omt = ob.model_transform(**mt_kw)
    ocam = default_camera(ob, W, H, **cam_kw)
    gt = gs.gaussian_transform_pod(gt_kw.get("size", 1.0), gt_kw.get("mode", 0), gt_kw.get("sh_deg", 3),
                                   gt_kw.get("no_sh0", False), gt_kw.get("max_std_dev", 3.0))
    mt = gs.model_transform_pod(mt_kw.get("pos", (0, 0, 0)), mt_kw.get("rot", (0, 0, 0, 1)),
                                mt_kw.get("scale", (1, 1, 1)))
    cam = copy_camera(ocam, gs.Camera)
    assert bytes(gt) == bytes(ogt) and bytes(mt) == bytes(omt)

    r, buf, img, rgba = render_gpu(gs, device, stream, pod, pods, gt, mt, cam, band, sort_mode=sort_mode)
    if info is not None:
        info.append(r.sort_info())
    order = mirror_order(ob, buf, stream, sh, cov, pods)
    o_proj, o_tiles, o_keys, o_idx, o_skeys, o_sidx, o_ranges, o_rgba = oracle_stages(
        ob, sh, cov, pods, ogt, omt, ocam, band, order=order)
    n = len(gaussians)
    st = r.stats()
    g_proj, g_tiles = r.download_projected(n)
    # --- preprocess ---
    bad = np.nonzero(g_tiles != o_tiles)[0]
    assert bad.size == 0, "tiles_touched differs at %d Gaussians, first %s: gpu %s oracle %s" % (
        bad.size, bad[:5], g_tiles[bad[:5]], o_tiles[bad[:5]])
    vis = o_tiles > 0
    gb = g_proj[vis].view(np.uint8).reshape(-1, 48)
    obb = o_proj[vis].view(np.uint8).reshape(-1, 48)
    badrec = np.nonzero((gb != obb).any(axis=1))[0]
    if badrec.size:
        i = badrec[0]
        raise AssertionError("projected record differs for %d of %d visible; first:\n gpu    %s\n oracle %s"
                             % (badrec.size, vis.sum(), g_proj[vis][i], o_proj[vis][i]))
    assert st.visible == int(vis.sum())
    assert st.pairs == len(o_keys)
    # --- keys + sort ---
    g_skeys, g_sidx = r.download_sorted()
    assert np.array_equal(g_skeys, o_skeys), "sorted keys differ"
    assert np.array_equal(g_sidx, o_sidx), "sorted indices differ"
    # --- ranges ---
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    g_ranges = r.download_ranges(tiles_x * tiles_y)
    assert np.array_equal(g_ranges, o_ranges), "tile ranges differ"
    # --- image ---
    b0, b1 = band if band is not None else (0, tiles_y)
    y0, y1 = b0 * 16, min(b1 * 16, H)
    diff = np.abs(rgba[y0:y1] - o_rgba[y0:y1])
    assert np.isfinite(rgba[y0:y1]).all()
    assert diff.max(initial=0.0) <= RGBA_TOL, "RGBA L-inf %g > %g (at %s)" % (
        diff.max(), RGBA_TOL, np.unravel_index(diff.argmax(), diff.shape))
    if check_image_exact:
        neq = (rgba[y0:y1].view(np.uint32) != o_rgba[y0:y1].view(np.uint32)).sum()
        assert neq == 0, "%d channel values differ in the last bits (max abs diff %g)" % (neq, diff.max())
    for h in (buf,):
        h.destroy()
    img.release()
    r.destroy()
    return st


class Scene:
    """a scene on the device with its image, its oracle frames and the oracle twin of a hidden selection"""

    def __init__(self, gs, ob, device, stream, sh, cov, n, W, H, mode=0, first=7, spatial=True, g=None, **cam_kw):
        self.gs, self.ob, self.device, self.stream = gs, ob, device, stream
        self.sh, self.cov, self.n, self.W, self.H = sh, cov, n, W, H
        self.g = synth.scene(n, first=first) if g is None else g
        self.pod, self.pods, self.ogt, self.omt, self.ocam, self.gt, self.mt, self.cam = frame_setup(
            gs, ob, self.g, W, H, sh, cov, mode, sh_deg=3 if sh != gs.SH_NONE else 0, **cam_kw)
        self.buf = gs.GaussiansBuffer.new_with_pods(device, self.pod, self.pods)
        if not spatial:
            self.buf.set_spatial_order(False)
        self.img = gs.Buffer(device, data=np.full(H * W * 4, np.float32(np.nan)))
        self.tiles_x, self.tiles_y = (W + 15) // 16, (H + 15) // 16

    def order(self):
        return self.buf.download_order(self.stream)

    def twin_pods(self, hidden):
        """the oracle twin: opacity byte (byte 15 of every record) of the hidden Gaussians := 0"""
        p = np.array(self.pods, dtype=np.uint8).reshape(self.n, -1).copy()
        p[np.asarray(hidden, bool), 15] = 0
        return p.reshape(-1)

    def oracle(self, pods, band=None, ocam=None, recolour=None):
        ob, ocam = self.ob, ocam or self.ocam
        proj, tiles = ob.preprocess(self.sh, self.cov, pods, self.ogt, self.omt, ocam, band=band)
        if recolour is not None:
            recolour(proj)
        keys, idx = ob.build_keys(proj, tiles, self.tiles_x, order=self.order())
        skeys, sidx = ob.sort_pairs(keys, idx)
        ranges = ob.tile_ranges(skeys, self.tiles_x * self.tiles_y)
        rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=self.ogt)
        return dict(proj=proj, tiles=np.asarray(tiles), keys=skeys, idx=sidx, ranges=ranges, rgba=rgba)

    def poison(self):
        self.img.write(self.stream, 0, np.full(self.H * self.W * 4, np.float32(np.nan)))
        self.stream.synchronize()

    def render(self, r, band=None, cam=None, **kw):
        fr = r.render(self.stream, self.buf, self.gt, self.mt, cam or self.cam, self.img.device_ptr(), band=band, **kw)
        self.stream.synchronize()
        return fr

    def image(self):
        return self.img.download(self.stream, np.float32).reshape(self.H, self.W, 4).copy()

    def selection(self, flags):
        s = self.gs.Selection(self.device, self.n)
        s.upload(self.stream, np.asarray(flags, bool))
        return s

    def release(self):
        self.img.release()
        self.buf.destroy()


def tint32(c, a, t):
    a, t = np.float32(a), np.float32(t)
    return (np.float32(1.0) - a) * c.astype(np.float32) + a * t
