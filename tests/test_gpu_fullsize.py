"""GPU parity at BASELINE.json's full sizes.  The oracle is too slow to run inside the GPU suite
at 10 M Gaussians, so these tests use (1) frame / scene hashes the oracle produced offline
(tests/golden/fullsize_v3.json, generators: tests/golden/make_golden_fullsize.py and _v3.py) — the HIP path is
specified bit-exact, so equal sha256 == equal frames — and (2) size-independent properties of the
intermediate results: sortedness and stability (in mirror order) of the (tile, depth) pairs, the pair multiset being
exactly the rect expansion of the projected records, tile ranges partitioning [0, D), idempotence,
band stitching, and the background identity out(bg) = out(0) + (1 - alpha) * bg."""
import hashlib
import json
import os

import numpy as np
import pytest

import helpers
from frames import render_image
from scenes import upload_synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# fullsize_v3.json: the frames of fullsize_v2.json (same hashes) with the visible / pair counts of rect version 4 (round 5:
# small rects lose the tiles their splat cannot reach); the older versions' counts ride along for the A/B switches
GOLD = json.load(open(os.path.join(HERE, "golden", "fullsize_v3.json")))
if os.environ.get("GS3D_RECT_V1") == "1":
    # the A/B switch of DESIGN.md §3.3: version 1 of the tile rect — same frames, the version-1 counts
    for _g in GOLD.values():
        _g["visible"], _g["pairs"] = _g["visible_rect_v1"], _g["pairs_rect_v1"]
elif os.environ.get("GS3D_TILE_MASKS") == "0":
    for _g in GOLD.values():
        _g["visible"], _g["pairs"] = _g["visible_rect_v3"], _g["pairs_rect_v3"]


def _check_intermediates(gs, r, g, cam, order):
    """properties of the sorted pairs / ranges / projected records that hold at any size"""
    n = g["n"]
    tiles_x, tiles_y = (cam.width + 15) // 16, (cam.height + 15) // 16
    num_tiles = tiles_x * tiles_y
    st = r.stats()
    keys, idx = r.download_sorted()
    D = len(keys)
    assert D == st.pairs == g["pairs"]
    # sortedness: keys non-decreasing; stability: equal keys keep ascending Gaussian index
    assert D < 2 or bool((keys[1:] >= keys[:-1]).all()), "keys not sorted"
    same = keys[1:] == keys[:-1]
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)      # mirror slot of every Gaussian
    assert bool((rank[idx[1:][same]] > rank[idx[:-1][same]]).all()), "equal keys not in stable (mirror) order"
    proj, tiles = r.download_projected(n)
    assert int((tiles > 0).sum()) == st.visible == g["visible"]
    assert int(tiles.sum(dtype=np.int64)) == D
    # key = (tile << 32) | depth bits of the Gaussian it points at
    tile_of = (keys >> np.uint64(32)).astype(np.int64)
    assert tile_of.max(initial=0) < num_tiles
    assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), proj["depth"][idx].view(np.uint32))
    assert bool((tiles[idx] > 0).all())
    # the pair multiset is exactly the rect expansion: per-Gaussian multiplicity == tiles_touched,
    # every pair's tile lies inside its Gaussian's rect
    assert np.array_equal(np.bincount(idx, minlength=n).astype(np.uint32), tiles)
    ty, tx = tile_of // tiles_x, tile_of % tiles_x
    p = proj[idx]     # rect in tile units, exclusive max
    assert bool(((tx >= p["tx0"]) & (tx < p["tx1"]) & (ty >= p["ty0"]) & (ty < p["ty1"])).all())
    area = (proj["tx1"].astype(np.int64) - proj["tx0"]) * (proj["ty1"].astype(np.int64) - proj["ty0"])
    # ... and is the whole rect, except for rects of at most 3 x 3 tiles, which may have lost tiles (rect version 4)
    w, h = proj["tx1"].astype(np.int64) - proj["tx0"], proj["ty1"].astype(np.int64) - proj["ty0"]
    small = (w <= 3) & (h <= 3)
    vis = tiles > 0
    assert np.array_equal(area[vis & ~small], tiles[vis & ~small].astype(np.int64))
    assert bool((tiles[vis & small] <= area[vis & small]).all())
    if os.environ.get("GS3D_TILE_MASKS") == "0" or os.environ.get("GS3D_RECT_V1") == "1":
        assert np.array_equal(area[vis], tiles[vis].astype(np.int64))
    # per-tile counts from the rects (difference array) == counts in the sorted keys == ranges
    counts = np.bincount(tile_of, minlength=num_tiles)
    ranges = r.download_ranges(num_tiles).reshape(num_tiles, 2).astype(np.int64)
    assert np.array_equal(ranges[:, 1] - ranges[:, 0], counts)
    nz = counts > 0
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert np.array_equal(ranges[nz, 0], starts[nz]), "ranges do not partition [0, D)"
    return keys, idx


@pytest.mark.parametrize("name", ["1m", "10m", "50m"])
def test_fullsize_frame_matches_oracle_hash(gs, device, stream, name):
    g = GOLD[name]
    pod, buf, scene_hash = upload_synth(gs, device, stream, g)
    assert scene_hash == g["scene_sha256"], "synthetic scene generator differs from the golden run (not a renderer issue)"
    spatial = buf.spatial_order()     # off only under GS3D_SPATIAL_ORDER=0
    if spatial:
        assert hashlib.sha256(buf.download_order(stream).tobytes()).hexdigest() == g["order_sha256"], \
            "spatial mirror order differs from the oracle's"
    frame_key = "frame_sha256" if spatial else "frame_sha256_index_order"
    cam = helpers.default_camera(gs, g["width"], g["height"])
    gt, mt = gs.gaussian_transform_pod(sh_deg=g["sh_deg"]), gs.model_transform_pod()
    r = gs.Renderer(device)
    rgba = render_image(gs, device, stream, r, buf, gt, mt, cam, cam.width, cam.height, poison=None)[0]
    st = r.stats()
    assert (st.visible, st.pairs) == (g["visible"], g["pairs"])
    assert np.isfinite(rgba).all()
    assert int((rgba[..., 3] > 0).sum()) == g["covered_pixels"]
    assert abs(float(rgba.astype(np.float64).sum()) - g["frame_sum"]) <= 1e-6 * g["frame_sum"]
    assert hashlib.sha256(rgba.tobytes()).hexdigest() == g[frame_key], "frame differs from the oracle's"
    if g["n"] <= 10_000_000:   # at 50 M the taps would move 175 M pairs through numpy: hashes, V, D and bands only
        _check_intermediates(gs, r, g, cam, buf.download_order(stream))
    # idempotence: same inputs, same bits (the pipeline has no order-dependent atomics in its results)
    again = render_image(gs, device, stream, r, buf, gt, mt, cam, cam.width, cam.height, poison=None)[0]
    assert np.array_equal(again.view(np.uint32), rgba.view(np.uint32))
    # band stitching at full size: 8 tile-row bands (the 8-GPU decomposition) == the full frame
    tiles_y = (g["height"] + 15) // 16
    edges = [tiles_y * k // 8 for k in range(9)]
    stitched = np.zeros_like(rgba)
    vis_sum = 0
    for b0, b1 in zip(edges[:-1], edges[1:]):
        part = render_image(gs, device, stream, r, buf, gt, mt, cam, cam.width, cam.height, poison=None, band=(b0, b1))[0]
        stitched[b0 * 16:min(b1 * 16, g["height"])] = part[b0 * 16:min(b1 * 16, g["height"])]
        vis_sum += r.stats().pairs
    assert hashlib.sha256(stitched.tobytes()).hexdigest() == g[frame_key]
    # bands emit every (tile, Gaussian) pair of the whole frame exactly once up to rect version 3; under version 4 a band
    # boundary changes which rects are 2..3 x 2..3 tiles (a 2 x 2 rect cut in two keeps all four tiles, a 4 x 3 one cut in
    # two may lose corners), so the sum moves by a fraction of a percent either way — the stitched image above does not
    if os.environ.get("GS3D_TILE_MASKS") == "0" or os.environ.get("GS3D_RECT_V1") == "1":
        assert vis_sum == g["pairs"], "bands must emit each (tile, Gaussian) pair exactly once"
    else:
        assert abs(vis_sum - g["pairs"]) <= 0.01 * g["pairs"], (vis_sum, g["pairs"])
    # the same buffer with the spatial order switched off: plain index order, the oracle's other hash
    buf.set_spatial_order(False)
    plain = render_image(gs, device, stream, r, buf, gt, mt, cam, cam.width, cam.height, poison=None)[0]
    assert np.array_equal(buf.download_order(stream), np.arange(g["n"], dtype=np.uint32))
    assert hashlib.sha256(plain.tobytes()).hexdigest() == g["frame_sha256_index_order"]
    r.destroy()
    buf.destroy()


def test_fullsize_4k_frame_matches_oracle_hash(gs, device, stream):
    g = GOLD["10m-4k"]
    pod, buf, scene_hash = upload_synth(gs, device, stream, g)
    assert scene_hash == g["scene_sha256"]
    cam = helpers.default_camera(gs, g["width"], g["height"])
    gt, mt = gs.gaussian_transform_pod(sh_deg=g["sh_deg"]), gs.model_transform_pod()
    r = gs.Renderer(device)
    rgba = render_image(gs, device, stream, r, buf, gt, mt, cam, cam.width, cam.height, poison=None)[0]
    st = r.stats()
    assert (st.visible, st.pairs) == (g["visible"], g["pairs"])
    assert hashlib.sha256(rgba.tobytes()).hexdigest() == g["frame_sha256" if buf.spatial_order() else
                                                             "frame_sha256_index_order"]
    r.destroy()
    buf.destroy()


class _HostTorch:
    """the two torch entry points parallel.assemble / allocate_gather use, on numpy arrays (the GPU
    suite must not initialise torch's own HIP runtime next to the product library's)"""
    float32 = np.float32

    @staticmethod
    def cat(rows, dim=0):
        return np.concatenate(rows, axis=dim)


class _DeviceGather:
    """device memory with the shape of parallel.allocate_gather's tensor"""

    def __init__(self, gs, device, plan, width):
        self.shape = (plan.world_size * plan.chunk_rows, width, 4)
        self.buf = gs.Buffer(device, size=self.shape[0] * width * 16)

    def data_ptr(self):
        return self.buf.device_ptr()

    def host(self, stream):
        return self.buf.download(stream, np.float32).reshape(self.shape)


def test_sharded_path_single_gpu_4k(gs, device, stream):
    """The 8-GPU decomposition of the 4K frame (BASELINE config 4), driven through the SAME code
    path bench.py uses for N > 1 — BandPlan, band_target_ptr into the gather buffer, assemble — with
    the 8 "ranks" played one after the other on this GPU (the all-gather is what is left out: every
    rank's chunk is simply already there).  Default floor(g R / G) bands and a cost-balanced plan
    must both reproduce the oracle's frame hash."""
    from importlib import import_module
    par = import_module("wgpu_3dgs_core_amd.parallel")
    g = GOLD["10m-4k"]
    pod, buf, scene_hash = upload_synth(gs, device, stream, g)
    assert scene_hash == g["scene_sha256"]
    W, H = g["width"], g["height"]
    cam = helpers.default_camera(gs, W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=g["sh_deg"]), gs.model_transform_pod()
    key = "frame_sha256" if buf.spatial_order() else "frame_sha256_index_order"
    r = gs.Renderer(device)
    plan = par.BandPlan(H, 8)
    assert [b - a for a, b in plan.bands] == [16, 17, 17, 17, 17, 17, 17, 17]
    row_pairs = np.zeros(plan.tiles_y)
    tiles_x = (W + 15) // 16
    for attempt in range(2):
        gbuf = _DeviceGather(gs, device, plan, W)
        pairs = 0
        for rank in range(8):
            r.render(stream, buf, gt, mt, cam, par.band_target_ptr(gbuf, plan, rank, W), band=plan.bands[rank])
            pairs += r.stats().pairs
            if attempt == 0:
                a, b = plan.bands[rank]
                rows = par.row_costs_from_ranges(r.download_ranges(tiles_x * plan.tiles_y), tiles_x, plan.tiles_y, fixed=0.0)
                row_pairs[a:b] = rows[a:b]
        img = par.assemble(_HostTorch, gbuf.host(stream), plan)
        gbuf.buf.release()
        assert img.shape == (H, W, 4)
        if os.environ.get("GS3D_TILE_MASKS") == "0" or os.environ.get("GS3D_RECT_V1") == "1":
            assert pairs == g["pairs"]
        else:      # (a band edge changes which rects are eligible for rect version 4's corner test)
            assert abs(pairs - g["pairs"]) <= 0.01 * g["pairs"], (pairs, g["pairs"])
        assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == g[key], \
            "sharded frame differs (plan %s)" % (plan.bands,)
        # second round: bands re-cut to equal pairs
        cost = lambda pl: max(row_pairs[a:b].sum() for a, b in pl.bands)
        new = plan.rebalanced(row_pairs + 64.0 * tiles_x)
        assert cost(new) <= cost(plan)
        plan = new
    r.destroy()
    buf.destroy()


def test_fullsize_background_identity(gs, device, stream):
    """out(bg).rgb = out(0).rgb + (1 - alpha) * bg, alpha independent of bg — at 1 M / 1080p."""
    g = GOLD["1m"]
    pod, buf, _ = upload_synth(gs, device, stream, g)
    gt, mt = gs.gaussian_transform_pod(sh_deg=g["sh_deg"]), gs.model_transform_pod()
    r = gs.Renderer(device)
    cam0 = helpers.default_camera(gs, g["width"], g["height"])
    cam1 = helpers.default_camera(gs, g["width"], g["height"])
    cam1.background[:] = [0.25, 0.5, 1.0]
    a = render_image(gs, device, stream, r, buf, gt, mt, cam0, cam0.width, cam0.height, poison=None)[0]
    b = render_image(gs, device, stream, r, buf, gt, mt, cam1, cam1.width, cam1.height, poison=None)[0]
    assert np.array_equal(a[..., 3].view(np.uint32), b[..., 3].view(np.uint32))
    t = 1.0 - a[..., 3].astype(np.float64)
    exp = a[..., :3].astype(np.float64) + t[..., None] * np.array([0.25, 0.5, 1.0])
    assert np.abs(b[..., :3] - exp).max() <= 2e-6
    r.destroy()
    buf.destroy()


@pytest.mark.skipif(not os.environ.get("GS3D_BIG_TEST"), reason="opt-in: GS3D_BIG_TEST=<millions of Gaussians> (minutes, tens of GB of HBM)")
def test_largest_scene_one_gpu(gs, ob, device, stream):
    """A scene several times BASELINE's largest on ONE GPU (GS3D_BIG_TEST=200: 200 M Gaussians, fp16 SH,
    28.8 GB of records + as much mirror + ~25 GB of frame scratch of the 288 GB): the oracle cannot blend
    that, but its preprocess can be run chunk by chunk while the scene is uploaded, so V and D are checked
    exactly; the image is checked by the size-independent properties (idempotence, two-band stitch ==
    whole frame, finite, covered).  Prints ms per frame."""
    import time
    import synth
    n = int(float(os.environ["GS3D_BIG_TEST"]) * 1_000_000)
    sh, cov, W, H = 1, 0, 1920, 1080
    pod = gs.GaussianPod(sh, cov)
    buf = gs.GaussiansBuffer.new_empty(device, pod, n)
    cam = helpers.default_camera(gs, W, H)
    ocam = helpers.default_camera(ob, W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    ogt, omt = ob.GaussianTransform.from_buffer_copy(bytes(gt)), ob.ModelTransform.from_buffer_copy(bytes(mt))
    vis = pairs = 0
    t0 = time.perf_counter()
    for first in range(0, n, 1_000_000):
        cnt = min(1_000_000, n - first)
        pods = pod.from_gaussian(synth.scene(cnt, first=first))
        buf.update_range_with_pod(stream, first, pods)
        _, tiles = ob.preprocess(sh, cov, pods, ogt, omt, ocam)
        vis += int((tiles > 0).sum())
        pairs += int(tiles.sum(dtype=np.int64))
    stream.synchronize()
    t_up = time.perf_counter() - t0
    assert pairs < 0xfffffff0, "pick a smaller scene: pair indices are 32-bit"
    r = gs.Renderer(device)
    t0 = time.perf_counter()
    rgba = render_image(gs, device, stream, r, buf, gt, mt, cam, cam.width, cam.height, poison=None)[0]      # includes the mirror / spatial-order build
    t_first = time.perf_counter() - t0
    st = r.stats()
    assert (st.visible, st.pairs) == (vis, pairs), (st.visible, vis, st.pairs, pairs)
    assert np.isfinite(rgba).all() and int((rgba[..., 3] > 0).sum()) > W * H // 2
    img = gs.Buffer(device, size=W * H * 16)
    for _ in range(2):
        r.render(stream, buf, gt, mt, cam, img.device_ptr())
    stream.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False)
    stream.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / 5
    again = img.download(stream, np.float32).reshape(H, W, 4)
    assert np.array_equal(again.view(np.uint32), rgba.view(np.uint32)), "not idempotent"
    tiles_y = (H + 15) // 16
    stitched = np.zeros_like(rgba)
    d_sum = 0
    for b0, b1 in ((0, tiles_y // 2), (tiles_y // 2, tiles_y)):
        part = render_image(gs, device, stream, r, buf, gt, mt, cam, cam.width, cam.height, poison=None, band=(b0, b1))[0]
        stitched[b0 * 16:min(b1 * 16, H)] = part[b0 * 16:min(b1 * 16, H)]
        d_sum += r.stats().pairs
    assert d_sum == pairs
    assert np.array_equal(stitched.view(np.uint32), rgba.view(np.uint32)), "two bands != whole frame"
    print("\nBIG %d M Gaussians (%d B records): upload+oracle counts %.1f s, first frame (mirror build) %.2f s, "
          "%.3f ms per frame = %.0f Msplats/s, V %d, D %d, frame sha256 %s" % (
              n // 1_000_000, pod.size, t_up, t_first, ms, n / ms / 1e3, vis, pairs, hashlib.sha256(rgba.tobytes()).hexdigest()[:16]))
    img.release()
    r.destroy()
    buf.destroy()
