"""The staging of k_blend_grouped in front of dead blocks, and its block threshold.  A block is dead when all its pixels are
parked: finished (T < 1e-4), outside the image, or finished in round 1 when round 2 resumes.  What the kernel stages for
such a block must not change a pixel, whether it enters the lists as null work (as now) or is left off them (measured and
not taken: NOTES.md Part VII).  The block threshold is pmin minus the rounding bound alone (cull_rounding_slack, no constant
0.1): a block may be dropped only if `power >= pmin` fails at every one of its pixels.  Every frame is compared bit for bit
(the uint32 view of every plane) with the oracle, for GS3D_BLEND_GROUPS = 4 (8x4 blocks) and 8 (4x4 blocks).

The switch is read once per process, so every setting renders all cases in one child process (this file, run as a script)
and leaves the frames in an .npz; the oracle's frames are computed once per case in the test process.  The scenes are built
as tests/test_gpu_blend_staging.py builds its scenes: isotropic Gaussians placed on chosen pixels, and the oracle's tile
ranges and `stopped` flags are asserted to say what the scene was built for before anything is compared.

  dead blocks   one 16 x 16 tile.  Nearest lie opaque splats on the centres of chosen 4x4 blocks, few enough to sit in
                batch 1 and enough to take all 16 pixels of those blocks below T < 1e-4 there (oracle: blend(...,
                stopped=True) on the range cut at 128 — exactly the chosen blocks are finished, no other).  Behind
                them 129, 130 or 257 large faint splats that reach every pixel: batches 2 and 3 stage them with the chosen
                blocks dead.  `one`: a single 4x4 block; `pair`: two side by side, one 8x4 block of G = 4; `wave0`: the
                eight blocks of pixel rows 0..7 (wave 1 still live); `allbut1`: fifteen of the sixteen.
  from the      `edge`: 22 x 19, partial tiles at the right and bottom edge, 6 and 3 pixels: blocks outside the image are
  start         dead from the first batch and one block column / row is cut.  `band`: the middle band of three with a block
                that dies in batch 1.  `rounds`: a two-round frame with the depth and pick planes, round 1 pinned to the
                nearest 2048 Gaussians (as tests/test_gpu_rounds.py pins it); it finishes one block in each of three
                tiles that stay open (asserted on the oracle's flags for the round-1 part of the ranges), so round 2
                resumes them with those blocks dead in its first batch.
  threshold     modes 0 and 1, a 7680 x 16 target, the block at x = 7608..7611 of the tile at x = 7600.  Splats approach
                the block from the left, from above and over its corner, and needles (axis ratio > 1000) pass it, each
                family as a scan of the centre offset that moves the block's maximum of `power` through at least
                [pmin - 0.12, pmin + 0.02] (asserted from the oracle's projection, in float64).  Asserted too: some
                splat whose block maximum is within 0.1 above pmin reaches alpha >= 1/255 on a pixel of the block whose
                final alpha is far from saturation — what a threshold that is too tight would lose."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gpu_child  # noqa: E402
import helpers  # noqa: E402

pytestmark = pytest.mark.gpu

SH, COV = 3, 0          # SH-none + rot-scale
ROUND1 = 2048           # the shortest round 1 the renderer takes
N_PAD = 4096            # Gaussians behind the camera: the renderer plans two rounds only for more than 4096
BEHIND = (129, 130, 257)
ALL16 = [(bx, by) for by in range(4) for bx in range(4)]
# name: (blocks that die in batch 1, opaque splats per block, their sigma in pixels)
DEAD_SETS = {
    "one": ([(1, 1)], 12, 2.0),
    "pair": ([(2, 2), (3, 2)], 12, 2.0),
    "wave0": ([b for b in ALL16 if b[1] < 2], 12, 2.0),
    "allbut1": ([b for b in ALL16 if b != (3, 3)], 8, 2.5),
}
THR_VFOV = 0.12         # degrees: a focal length of 7.6 k pixels, so that x = 7600 is an ordinary view direction
THR_BLOCK = (7608, 4)   # first pixel of the block the threshold scans aim at
ROUNDS_CLUSTER_TILES = (0, 5, 10)

# name: (kind, W, H, mode, band, vfov)
CASES = {}
for _s in DEAD_SETS:
    for _n in BEHIND:
        CASES["%s_%d" % (_s, _n)] = ("dead", 16, 16, 0, None, 60.0)
CASES["edge"] = ("edge", 22, 19, 0, None, 60.0)
CASES["band"] = ("band", 32, 48, 0, (1, 2), 60.0)
CASES["thr_m0"] = ("thr", 7680, 16, 0, None, THR_VFOV)
CASES["thr_m1"] = ("thr", 7680, 16, 1, None, THR_VFOV)
ROUNDS_CASE = ("rounds", 64, 48, 0, None, 60.0)


def _ob():
    from oracle import binding
    return binding


def _pack(splats, W, H, vfov):
    """splats: rows (px, py, sigma_px, z, r, g, b, opacity byte); pixel coordinates are continuous (pixel i spans i .. i + 1)"""
    import synth
    cam = helpers.default_camera(_ob(), W, H, vfov_deg=vfov)
    a = np.asarray(splats, dtype=np.float64).reshape(-1, 8)
    g = np.zeros(len(a), dtype=synth.GAUSSIAN_DTYPE)
    g["rot"][:] = (0.0, 0.0, 0.0, 1.0)
    g["pos"][:, 0] = (a[:, 0] - cam.cx) / cam.fx * a[:, 3]
    g["pos"][:, 1] = -(a[:, 1] - cam.cy) / cam.fy * a[:, 3]
    g["pos"][:, 2] = -a[:, 3]
    g["scale"][:] = np.abs(a[:, 2] * a[:, 3] / cam.fx)[:, None]
    g["color"][:] = a[:, 4:8].astype(np.uint8)
    return g


def _cluster(rng, ox, oy, blocks, per_block, sig, z0):
    """opaque splats on the centres of 4x4 blocks of the tile at (ox, oy), interleaved over the blocks"""
    out = []
    for k in range(per_block):
        for i, (bx, by) in enumerate(blocks):
            out.append((ox + 4 * bx + 2.0, oy + 4 * by + 2.0, sig, z0 + 0.001 * (k * len(blocks) + i),
                        rng.randint(256), rng.randint(256), rng.randint(256), 255))
    return out


def _big(rng, W, H, n, z0=3.0):
    """large faint splats that reach alpha >= 1/255 at every pixel"""
    return [(W / 2 + rng.uniform(-4, 4), H / 2 + rng.uniform(-4, 4), rng.uniform(40.0, 60.0), z0 + 0.002 * i,
             rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(3, 6)) for i in range(n)]


def _small(rng, ox, oy, n, z0, z1):
    """small splats (sigma half a pixel) in the middle 7 x 7 pixels of the tile at (ox, oy): pairs of that tile only"""
    zs = z0 + (z1 - z0) * rng.permutation(n) / max(n, 1)
    return [(ox + rng.uniform(4.5, 11.5), oy + rng.uniform(4.5, 11.5), 0.5, zs[i],
             rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(20, 50)) for i in range(n)]


def _rounds_small_counts():
    """per tile: small splats of round 1, and of round 2"""
    r1 = [30] * 12
    r2 = [129, 1, 64, 65, 128, 130, 0, 63, 127, 2, 257, 191]
    return r1, r2


def _needles(cam, offs, theta_deg, sigma_px, opacity, z=4.0):
    """needles through (7320, 5.5 - off): standard deviation sigma_px along a direction theta from the x axis and far below a
    pixel across (the +0.3 dilation sets the width: axis ratio sigma_px / 0.55)"""
    import synth
    g = np.zeros(len(offs), dtype=synth.GAUSSIAN_DTYPE)
    t = np.deg2rad(theta_deg) / 2
    g["rot"][:] = (0.0, 0.0, np.sin(t), np.cos(t))
    g["pos"][:, 0] = (7320.0 - cam.cx) / cam.fx * z
    g["pos"][:, 1] = -((5.5 - np.asarray(offs, dtype=np.float64)) - cam.cy) / cam.fy * z
    g["pos"][:, 2] = -z
    g["scale"][:] = (sigma_px * z / cam.fx, 1e-7, 1e-7)
    g["color"][:] = (200, 120, 40, opacity)
    return g


def _block_max(proj, bx0, by0):
    """float64 maximum of `power` over the 16 pixel centres of the 4x4 block at (bx0, by0), per projected Gaussian"""
    p = {k: proj[k].astype(np.float64) for k in ("mx", "my", "ca", "cb", "cc")}
    best = np.full(len(proj), -np.inf)
    for y in range(4):
        for x in range(4):
            dx, dy = p["mx"] - (bx0 + x + 0.5), p["my"] - (by0 + y + 0.5)
            best = np.maximum(best, p["ca"] * dx * dx + p["cb"] * dx * dy + p["cc"] * dy * dy)
    return best


def _pmin(proj, mode):
    if mode == 1:
        return np.full(len(proj), -4.5)
    return np.maximum(-np.log(255.0 * proj["opacity"].astype(np.float64)) - 1e-3, -5.6)


_THR = {}


def _thr_families(mode):
    """the scans of a threshold case: list of (name, Gaussians), offsets chosen from a probe run of the oracle's projection so
    that the block maximum minus pmin runs from above +0.04 to below -0.14; cached per mode"""
    if mode in _THR:
        return _THR[mode]
    ob = _ob()
    W, H = 7680, 16
    cam = helpers.default_camera(ob, W, H, vfov_deg=THR_VFOV)
    ogt, omt = ob.gaussian_transform(sh_deg=0, mode=mode), ob.model_transform()
    bx0, by0 = THR_BLOCK
    op = 255 if mode == 0 else 3      # Ellipse: alpha is flat inside the ellipse, so a faint one (the pixels must stay live)

    def iso(dirx, diry, ax, ay):
        # centre = (ax, ay) - off * (dirx, diry): (ax, ay) is a pixel centre of the block's facing edge or corner
        return lambda offs: _pack([(ax - o * dirx, ay - o * diry, 1.0, 4.0, 90, 200, 160, op) for o in offs], W, H, THR_VFOV)
    fams = {
        "left": (iso(1.0, 0.0, bx0 + 0.5, by0 + 1.5), (2.0, 5.0)),
        "above": (iso(0.0, 1.0, bx0 + 1.5, by0 + 0.5), (2.0, 4.4)),
        "corner": (iso(0.7071, 0.7071, bx0 + 0.5, by0 + 0.5), (2.0, 5.0)),
        "needle": (lambda offs: _needles(cam, offs, -20.0, 800.0, op), None),
    }
    out = []
    for name, (make, span) in fams.items():
        if span is None:
            # the needle's line passes the block's nearest pixel centre at some offset: walk up from there
            probe = np.linspace(-120.0, 120.0, 2401)
            g = make(probe)
            proj, _ = ob.preprocess(SH, COV, ob.pack(SH, COV, g), ogt, omt, cam)
            rel = _block_max(proj, bx0, by0) - _pmin(proj, mode)
            peak = int(np.argmax(rel))
            assert rel[peak] > 0.5, "the needle never crosses the block"
            probe, rel = probe[peak:], rel[peak:]
        else:
            probe = np.linspace(span[0], span[1], 601)
            g = make(probe)
            proj, _ = ob.preprocess(SH, COV, ob.pack(SH, COV, g), ogt, omt, cam)
            rel = _block_max(proj, bx0, by0) - _pmin(proj, mode)
        # rel falls with the offset: the stretch from +0.04 down to -0.14
        hi = probe[np.nonzero(rel > 0.04)[0][-1]]
        lo = probe[np.nonzero(rel < -0.14)[0][0]]
        assert hi < lo, (name, hi, lo)
        out.append((name, make(np.linspace(hi, lo, 64 if span else 128))))
    _THR[mode] = out
    return out


def _gaussians(name, case):
    """the built scene; also what it was built for (checked against the oracle in _check_scene)"""
    kind, W, H, mode, band, vfov = case
    rng = np.random.RandomState(sum(map(ord, name)))
    if kind == "dead":
        set_name, n = name.rsplit("_", 1)
        blocks, per, sig = DEAD_SETS[set_name]
        return _pack(_cluster(rng, 0, 0, blocks, per, sig, 2.0) + _big(rng, W, H, int(n)), W, H, vfov)
    if kind == "edge":
        return _pack(_big(rng, W, H, 140) + _small(rng, 0, 0, 20, 4.0, 5.0), W, H, vfov)
    if kind == "band":
        return _pack(_cluster(rng, 0, 16, [(1, 1)], 24, 1.5, 2.0) + _big(rng, W, H, 129), W, H, vfov)
    if kind == "thr":
        return np.concatenate([g for _, g in _thr_families(mode)])
    assert kind == "rounds"
    r1, r2 = _rounds_small_counts()
    s = []
    for t in ROUNDS_CLUSTER_TILES:
        s += _cluster(rng, 16 * (t % 4), 16 * (t // 4), [(1 + t % 2, 1 + (t // 4) % 2)], 24, 1.5, 2.0 + 0.03 * t)
    s += _big(rng, W, H, 128)
    for t in range(12):
        s += _small(rng, 16 * (t % 4), 16 * (t // 4), r1[t], 4.0, 5.0)
    s += _small(rng, 16, 16, ROUND1 - len(s), 5.0, 5.5)           # tile 5 fills round 1 up
    assert len(s) == ROUND1
    for t in range(12):
        s += _small(rng, 16 * (t % 4), 16 * (t // 4), r2[t], 7.0, 8.5)
    s += [(rng.uniform(0, W), rng.uniform(0, H), 2.0, -(1.0 + 0.001 * i), 255, 255, 255, 255) for i in range(N_PAD)]
    return _pack(s, W, H, vfov)


def _child(out):
    """renders every case under this process's switches"""
    with gpu_child.child_rig() as (gs, _, dev, st):
        from planes import Planes
        res = {}
        cases = dict(CASES)
        cases["rounds"] = ROUNDS_CASE
        for name, case in cases.items():
            kind, W, H, mode, band, vfov = case
            pod = gs.GaussianPod(SH, COV)
            pods = pod.from_gaussian(_gaussians(name, case))
            gt = gs.gaussian_transform_pod(1.0, mode, 0, False, 3.0)
            mt = gs.model_transform_pod((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))
            cam = helpers.default_camera(gs, W, H, vfov_deg=vfov)
            buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pods)
            r = gs.Renderer(dev)
            if kind != "rounds":
                img = gs.Buffer(dev, data=np.full(H * W * 4, helpers.POISON))
                r.render(st, buf, gt, mt, cam, img.device_ptr(), band=band)
                st.synchronize()
                res[name + "/rgba"] = img.download(st, np.float32).reshape(H, W, 4).copy()
                img.release()
            else:
                r.set_rounds(1, ROUND1)
                pl = Planes(gs, dev, W, H)
                for frame in range(2):       # the second frame of a two-round renderer is partitioned
                    pl.poison(st)
                    pl.render(r, st, buf, gt, mt, cam, band=band)
                    si = r.sort_info()
                    rgba, depth, pick = pl.get(st)
                    res["%s/f%d/rgba" % (name, frame)] = rgba
                    res["%s/f%d/depth" % (name, frame)] = depth
                    res["%s/f%d/pick" % (name, frame)] = pick
                    res["%s/f%d/info" % (name, frame)] = np.array([si.rounds, si.round1, si.tiles_done], dtype=np.int64)
                pl.release()
            r.destroy()
            buf.destroy()
        np.savez(out, **res)


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """groups -> the child's planes; every child runs once, on first use"""
    tmp = tmp_path_factory.mktemp("blend_dead_blocks")
    cache = {}

    def get(groups):
        if groups not in cache:
            out = os.path.join(str(tmp), "g%d.npz" % groups)
            gpu_child.run([os.path.abspath(__file__), out], env={"GS3D_BLEND_GROUPS": str(groups)}, timeout=300,
                          label="GS3D_BLEND_GROUPS=%d" % groups)
            cache[groups] = gpu_child.load_npz(out)
        return cache[groups]
    return get


_ORACLE = {}


def _oracle(ob, name, case):
    """the oracle's planes of a case and its lists; computed once per case"""
    if name in _ORACLE:
        return _ORACLE[name]
    from planes import oracle_depth
    kind, W, H, mode, band, vfov = case
    pods = ob.pack(SH, COV, _gaussians(name, case))
    ogt, omt = ob.gaussian_transform(sh_deg=0, mode=mode), ob.model_transform()
    ocam = helpers.default_camera(ob, W, H, vfov_deg=vfov)
    order = ob.spatial_order(SH, COV, pods)      # a fresh buffer's mirror order
    proj, tiles = ob.preprocess(SH, COV, pods, ogt, omt, ocam, band=band)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=ogt)
    _ORACLE[name] = dict(rgba=rgba, proj=proj, sidx=sidx, ranges=ranges, tiles_x=tiles_x, tiles_y=tiles_y, ocam=ocam, ogt=ogt,
                         depth=lambda: oracle_depth(ob, proj, sidx, ranges, ocam, ogt, band))
    return _ORACLE[name]


def _finished_blocks(ob, o, cut, band=None):
    """4x4 blocks all of whose 16 pixels left their list through the transmittance test within the first cut[t] entries of
    tile t's range: bool [H / 4, W / 4] (the image sizes used with it are multiples of 4)"""
    r = o["ranges"].copy()
    r[:, 1] = r[:, 0] + np.minimum(r[:, 1] - r[:, 0], np.asarray(cut, dtype=np.uint32))
    _, st = ob.blend(o["proj"], o["sidx"], r, o["ocam"], band=band, gt=o["ogt"], stopped=True)
    H, W = st.shape
    return (st > 0).reshape(H // 4, 4, W // 4, 4).all(axis=(1, 3))


def _check_scene(ob, name, case, o):
    """the oracle's lists and flags are the ones the scene was built for"""
    kind, W, H, mode, band, vfov = case
    lens = (o["ranges"][:, 1] - o["ranges"][:, 0]).astype(np.int64)
    if kind == "dead":
        set_name, n = name.rsplit("_", 1)
        blocks, per, sig = DEAD_SETS[set_name]
        front = per * len(blocks)
        assert front <= 128 and lens[0] == front + int(n), lens
        assert o["proj"]["opacity"][o["sidx"][:front]].min() >= 0.99           # the opaque splats lie nearest
        fin = _finished_blocks(ob, o, [128])
        want = np.zeros((4, 4), bool)
        for bx, by in blocks:
            want[by, bx] = True
        assert np.array_equal(fin, want), "blocks finished in batch 1:\n%s\nbuilt for:\n%s" % (fin, want)
    elif kind == "edge":
        assert list(lens) == [160, 140, 140, 140], lens
    elif kind == "band":
        assert lens[2] == 24 + 129 and lens[3] == 129, lens
        fin = _finished_blocks(ob, o, [128] * 6, band=band)
        assert fin[4 + 1, 1] and fin[4:8].sum() == 1, fin[4:8]
    elif kind == "thr":
        bx0, by0 = THR_BLOCK
        fams = _thr_families(mode)
        at, witnessed = 0, False
        final_alpha = o["rgba"][by0:by0 + 4, bx0:bx0 + 4, 3]
        assert final_alpha.max() < 0.9, "the block's pixels saturate: later splats would not show"
        for fname, g in fams:
            proj = o["proj"][at:at + len(g)]
            at += len(g)
            rel = _block_max(proj, bx0, by0) - _pmin(proj, mode)
            assert rel.max() >= 0.02 and rel.min() <= -0.12, (fname, rel.min(), rel.max())
            assert np.abs(np.diff(np.sort(rel))).max() <= 0.02, fname      # a scan, not two clusters
            op = proj["opacity"].astype(np.float64)
            alpha = op * np.exp(rel + _pmin(proj, mode)) if mode == 0 else op
            witnessed |= bool(((rel >= 0.0) & (rel <= 0.1) & (alpha >= 1.0 / 255.0)).any())
            if fname == "needle":
                assert _axis_ratio(proj).min() >= 1.0e3
        assert at == len(o["proj"])
        assert witnessed, "no splat within 0.1 above pmin reaches alpha >= 1/255 on the block"
    else:
        r1, r2 = _rounds_small_counts()
        first = o["sidx"] < ROUND1                       # Gaussians 0 .. 2047 are the nearest 2048: round 1
        cut = []
        for t in range(12):
            s, e = int(o["ranges"][t, 0]), int(o["ranges"][t, 1])
            n1 = int(first[s:e].sum())
            assert first[s:s + n1].all()
            cut.append(n1)
            want1 = 128 + r1[t] + (24 if t in ROUNDS_CLUSTER_TILES else 0) + (ROUND1 - 128 - 72 - 360 if t == 5 else 0)
            assert n1 == want1 and e - s - n1 == r2[t], (t, n1, want1, e - s - n1)
        fin = _finished_blocks(ob, o, cut)
        for t in ROUNDS_CLUSTER_TILES:
            tx, ty = t % 4, t // 4
            f = fin[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4]
            assert f[1 + ty % 2, 1 + t % 2] and not f.all(), (t, f)       # round 1 finishes the block, not the tile
            assert r2[t] > 0


def _axis_ratio(proj):
    """sqrt of the conic's eigenvalue ratio: long over short standard deviation"""
    a, b, c = (-2.0 * proj["ca"].astype(np.float64), -proj["cb"].astype(np.float64), -2.0 * proj["cc"].astype(np.float64))
    mid, rad = 0.5 * (a + c), np.sqrt(0.25 * (a - c) ** 2 + b * b)
    return np.sqrt((mid + rad) / (mid - rad))


@pytest.mark.parametrize("name", list(CASES))
def test_dead_blocks_equal_the_oracle(ob, frames, name):
    case = CASES[name]
    kind, W, H, mode, band, vfov = case
    o = _oracle(ob, name, case)
    _check_scene(ob, name, case, o)
    y0, y1 = helpers.band_rows(band, H)
    for groups in (8, 4):
        got = frames(groups)[name + "/rgba"]
        assert np.array_equal(helpers.bits(got[y0:y1]), helpers.bits(o["rgba"][y0:y1])), "groups %d != oracle" % groups
        if band is not None:      # rows outside the band keep the poison
            assert np.all(got[:y0] == helpers.POISON) and np.all(got[y1:] == helpers.POISON)
    assert (o["rgba"][y0:y1, :, 3] > 0.0).any()


def test_round_two_resumes_with_dead_blocks(ob, gs, frames):
    from planes import pick_witness
    name, case = "rounds", ROUNDS_CASE
    kind, W, H, mode, band, vfov = case
    o = _oracle(ob, name, case)
    _check_scene(ob, name, case, o)
    o_depth = o["depth"]()
    w_pick, amb = pick_witness(o["proj"], o["sidx"], o["ranges"], W, H, o["tiles_x"], 0.5)
    assert amb.mean() <= 1e-2
    for frame in range(2):
        k = "%s/f%d/" % (name, frame)
        for groups in (8, 4):
            f = frames(groups)
            rounds, round1, done = [int(x) for x in f[k + "info"]]
            assert rounds == 2 and round1 == ROUND1
            assert done < 12 - len(ROUNDS_CLUSTER_TILES) + 1, "round 1 finished a tile it was built to leave open"
            ctx = "groups %d, frame %d" % (groups, frame)
            assert np.array_equal(helpers.bits(f[k + "rgba"]), helpers.bits(o["rgba"])), "colour != oracle: " + ctx
            assert np.array_equal(helpers.bits(f[k + "depth"]), helpers.bits(o_depth)), "depth != oracle: " + ctx
            assert np.array_equal(f[k + "pick"] != gs.PICK_NONE, f[k + "rgba"][..., 3] >= 0.5), ctx
            bad = (w_pick != f[k + "pick"].astype(np.uint64)) & ~amb
            assert not bad.any(), "pick != the float64 walk of the oracle's lists at %d pixels: %s" % (bad.sum(), ctx)


if __name__ == "__main__":
    _child(sys.argv[1])
