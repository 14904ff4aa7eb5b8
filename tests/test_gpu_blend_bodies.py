"""The two forms of k_blend_grouped's trip loop (csrc/gs_render_kernels.h, NOTES.md Part XVII).  A wave runs a batch in the
BRANCH-FREE form — no any-lane test, T alternating between two register pairs, the exact step count: trip / 4 trips of four
steps and 0..3 single steps — while at least BLEND_FREE_MIN_LIVE of its 128 pixels are live at the top of the batch, and in
the BRANCHY form otherwise.  GS3D_BLEND_FREE_BODY pins the choice (0 branchy, 1 branch-free) and is read once per process.

Every frame is compared bit for bit (the uint32 view of every plane) with the oracle, three ways: under the rule in the test
process (the renderer's own choice of blocks: G = 8, and G = 4 on the rounds of the two-round frame), and pinned branchy and
pinned branch-free in one child process each (this file, run as a script); the pinned runs also go under
GS3D_BLEND_GROUPS = 4 and = 2.  Instantiations that carry the branchy form alone (the planes, two rounds, contribution
frames below G = 8) must pass with the switch set all the same.  The oracle's frames are computed once per case, and what a
scene was built for is asserted on the oracle's ranges, `stopped` flags and image before anything is compared.  The scenes
are built as tests/test_gpu_blend_trips.py builds its scenes: isotropic Gaussians placed on chosen pixels of images of one
to six tiles.

  full_n        one tile, n large faint splats that reach alpha >= 1/255 at every pixel (asserted in float64), so every block
                list holds n entries: n = 1 .. 9 and 125 .. 133.  A remainder of 0, 1, 2 and 3 steps behind zero, one and
                thirty-one trips; 128: the read ahead of the last step leaves the row; 129 .. 133: a second batch of 1 .. 5.
  uneven        one large splat in every list and 127 tiny ones centred in the 4x4 block (1, 1): one list of a wave is full
                while its neighbours hold one entry and idle on the null record.
  last_block    128 tiny splats centred in block (3, 3), the tile's last list, nothing else: the read ahead of the last step
                runs into the pad behind the lists.  Asserted on the oracle's image: only that block's pixels are coloured.
  finish_a      a = 4 .. 7 large faint splats, then six opaque ones whose mean is the centre of pixel (5, 5), then twenty
                brighter large ones.  That pixel reaches T < 1e-4 at the second opaque splat, list position a + 1 = 5, 6, 7,
                8: each of the four steps of a trip (asserted with the oracle's `stopped` flags on ranges cut at a + 1 and
                a + 2); the splats behind must not touch it.
  finrem_k      k = 0, 1, 2: the pixel reaches T < 1e-4 in step k of a three-step remainder.  Batch 1 holds 7 entries for
                the lists of wave 0 (the tile's upper half) — 3 + k faint splats and 4 - k opaque ones on pixel (5, 5), which
                leaves at position 4 + k — and 121 tiny splats in block (3, 3), which reach no pixel of wave 0 (asserted);
                the twenty brighter splats are the second batch.
  boundary_d    d = -1, 0, +1: 2 s tiny opaque splats on the centres of the first s pixels of the tile's upper half finish
                exactly those in batch 1 (each at its second splat), faint large splats fill the batch, and 130 more cover
                the tile behind it: wave 0 enters batch 2 with BLEND_FREE_MIN_LIVE + d live pixels (asserted on the `stopped`
                flags of the range cut at 128).  Under the rule, d = -1 runs batch 1 branch-free and batch 2 branchy.
  ellipse,      modes 1 and 2 on a 32 x 16 image; `partial`: an image of 6 x 3 pixels; `band`: the middle band of three;
  point, ...    `rounds`: a two-round frame with the depth and pick planes, round 1 pinned to the nearest 2048 Gaussians, lists
                of 5, 129 and 2 left for round 2; `contrib`: a contribution frame."""
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
MIN_LIVE = 73           # gs::BLEND_FREE_MIN_LIVE
FULL_N = tuple(range(1, 10)) + tuple(range(125, 134))
FINISH_A = (4, 5, 6, 7)
FINREM_K = (0, 1, 2)
BOUNDARY_D = (-1, 0, 1)
FINISH_PIXEL = (5, 5)
ROUNDS_R1 = (683, 683, 682)
ROUNDS_R2 = (5, 129, 2)
# the runs: name -> environment of the process (None: the test process itself, under the rule)
RUNS = {"rule": None}
for _g in (8, 4, 2):
    for _b in (0, 1):
        RUNS["g%d_body%d" % (_g, _b)] = dict({"GS3D_BLEND_FREE_BODY": str(_b)}, **({} if _g == 8 else {"GS3D_BLEND_GROUPS": str(_g)}))

# name: (kind, W, H, mode, band)
CASES = {}
for _n in FULL_N:
    CASES["full_%d" % _n] = ("full", 16, 16, 0, None)
CASES["uneven"] = ("uneven", 16, 16, 0, None)
CASES["last_block"] = ("last_block", 16, 16, 0, None)
for _a in FINISH_A:
    CASES["finish_%d" % _a] = ("finish", 16, 16, 0, None)
for _k in FINREM_K:
    CASES["finrem_%d" % _k] = ("finrem", 16, 16, 0, None)
for _d in BOUNDARY_D:
    CASES["boundary_%d" % _d] = ("boundary", 16, 16, 0, None)
CASES["ellipse"] = ("modes", 32, 16, 1, None)
CASES["point"] = ("modes", 32, 16, 2, None)
CASES["partial"] = ("partial", 6, 3, 0, None)
CASES["band"] = ("band", 32, 48, 0, (1, 2))
CASES["contrib"] = ("contrib", 32, 16, 0, None)
CASES["rounds"] = ("rounds", 48, 16, 0, None)
assert sum(ROUNDS_R1) == ROUND1


def _ob():
    from oracle import binding
    return binding


def _pack(splats, W, H):
    """splats: rows (px, py, sigma_px, z, r, g, b, opacity byte); pixel coordinates are continuous (pixel i spans i .. i + 1)"""
    import synth
    cam = helpers.default_camera(_ob(), W, H)
    a = np.asarray(splats, dtype=np.float64).reshape(-1, 8)
    g = np.zeros(len(a), dtype=synth.GAUSSIAN_DTYPE)
    g["rot"][:] = (0.0, 0.0, 0.0, 1.0)
    g["pos"][:, 0] = (a[:, 0] - cam.cx) / cam.fx * a[:, 3]
    g["pos"][:, 1] = -(a[:, 1] - cam.cy) / cam.fy * a[:, 3]
    g["pos"][:, 2] = -a[:, 3]
    g["scale"][:] = np.abs(a[:, 2] * a[:, 3] / cam.fx)[:, None]
    g["color"][:] = a[:, 4:8].astype(np.uint8)
    return g


def _big(rng, W, H, n, z0=3.0, bytes_=(3, 6)):
    """large faint splats that reach alpha >= 1/255 at every pixel"""
    return [(W / 2 + rng.uniform(-4, 4), H / 2 + rng.uniform(-4, 4), rng.uniform(40.0, 60.0), z0 + 0.002 * i,
             rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(*bytes_)) for i in range(n)]


def _small(rng, ox, oy, n, z0, z1):
    """small splats (sigma half a pixel) in the middle 7 x 7 pixels of the tile at (ox, oy): pairs of that tile only"""
    zs = z0 + (z1 - z0) * rng.permutation(n) / max(n, 1)
    return [(ox + rng.uniform(4.5, 11.5), oy + rng.uniform(4.5, 11.5), 0.5, zs[i],
             rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(20, 50)) for i in range(n)]


def _tiny(rng, cx, cy, n, z0=4.0):
    """faint splats of half a pixel within 0.3 pixels of (cx, cy), the centre of a 4x4 block: they reach alpha >= 1/255 within
    1.5 pixels of their mean, inside the block"""
    return [(cx + rng.uniform(-0.3, 0.3), cy + rng.uniform(-0.3, 0.3), 0.5, z0 + 0.002 * i,
             rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(4, 8)) for i in range(n)]


def _mid(rng, W, H, n):
    """splats of a few pixels all over the image, faint to half opaque"""
    return [(rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1.0, 5.0), 3.0 + 0.01 * i,
             rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(3, 128)) for i in range(n)]


def _opaque(rng, px, py, n, z0, sigma=2.0):
    """n opaque splats whose mean is the centre of pixel (px, py)"""
    return [(px + 0.5, py + 0.5, sigma, z0 + 0.001 * i, rng.randint(256), rng.randint(256), rng.randint(256), 255) for i in range(n)]


def boundary_stopped(name):
    """how many pixels of the tile's upper half the boundary case finishes in batch 1"""
    return 128 - (MIN_LIVE + int(name.split("_")[1]))


_SCENES = {}


def scene(name):
    """the Gaussians of a case (built once per process)"""
    if name in _SCENES:
        return _SCENES[name]
    kind, W, H, mode, band = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    if kind == "full":
        s = _big(rng, W, H, int(name.split("_")[1]))
    elif kind == "uneven":
        s = _big(rng, W, H, 1) + _tiny(rng, 6.0, 6.0, 127)
    elif kind == "last_block":
        s = _tiny(rng, 14.0, 14.0, 128)
    elif kind == "finish":
        a = int(name.split("_")[1])
        px, py = FINISH_PIXEL
        s = _big(rng, W, H, a, z0=2.0) + _opaque(rng, px, py, 6, 3.0) + _big(rng, W, H, 20, z0=4.0, bytes_=(20, 40))
    elif kind == "finrem":
        k = int(name.split("_")[1])
        px, py = FINISH_PIXEL
        s = _big(rng, W, H, 3 + k, z0=2.0) + _opaque(rng, px, py, 4 - k, 3.0) + _tiny(rng, 14.0, 14.0, 121, z0=3.5)
        s += _big(rng, W, H, 20, z0=4.0, bytes_=(20, 40))
    elif kind == "boundary":
        n = boundary_stopped(name)
        assert 2 * n <= 128
        s = []
        for i in range(n):       # two opaque splats of a quarter pixel on the pixel's centre: T = 0.01 behind the first
            s += _opaque(rng, i % 16, i // 16, 2, 2.0 + 0.004 * i, sigma=0.25)
        s += _big(rng, W, H, 128 - 2 * n, z0=3.0) + _big(rng, W, H, 130, z0=4.0, bytes_=(20, 40))
    elif kind == "modes":
        s = _mid(rng, W, H, 150)
    elif kind == "partial":
        s = _big(rng, W, H, 140)
    elif kind == "band":
        s = _big(rng, W, H, 131) + _small(rng, 16, 16, 7, 4.0, 5.0)
    elif kind == "contrib":
        s = _big(rng, W, H, 5) + _small(rng, 0, 0, 140, 4.0, 5.0) + _small(rng, 16, 0, 3, 4.0, 5.0)
    else:
        assert kind == "rounds"
        s = []
        for t in range(3):
            s += _small(rng, 16 * t, 0, ROUNDS_R1[t], 4.0, 5.0)
        for t in range(3):
            s += _small(rng, 16 * t, 0, ROUNDS_R2[t], 7.0, 8.5)
        s += [(rng.uniform(0, W), rng.uniform(0, H), 2.0, -(1.0 + 0.001 * i), 255, 255, 255, 255) for i in range(N_PAD)]
    _SCENES[name] = _pack(s, W, H)
    return _SCENES[name]


def render_all(gs, dev, st):
    """every case under this process's switches: name/plane -> array"""
    from planes import Planes
    res = {}
    pod = gs.GaussianPod(SH, COV)
    mt = gs.model_transform_pod((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))
    for name, (kind, W, H, mode, band) in CASES.items():
        gt = gs.gaussian_transform_pod(1.0, mode, 0, False, 3.0)
        cam = helpers.default_camera(gs, W, H)
        buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pod.from_gaussian(scene(name)))
        r = gs.Renderer(dev)
        if kind == "rounds":
            r.set_rounds(1, ROUND1)
            pl = Planes(gs, dev, W, H)
            for frame in range(2):       # the second frame of a two-round renderer is partitioned
                pl.poison(st)
                pl.render(r, st, buf, gt, mt, cam)
                si = r.sort_info()
                res["%s/f%d/rgba" % (name, frame)], res["%s/f%d/depth" % (name, frame)], res["%s/f%d/pick" % (name, frame)] = pl.get(st)
                res["%s/f%d/info" % (name, frame)] = np.array([si.rounds, si.round1], dtype=np.int64)
            pl.release()
        else:
            img = gs.Buffer(dev, data=np.full(H * W * 4, helpers.POISON))
            c = gs.Contributions.new(dev, st, len(scene(name))) if kind == "contrib" else None
            if c is not None:
                r.render(st, buf, gt, mt, cam, img.device_ptr(), contributions=c)
            else:
                r.render(st, buf, gt, mt, cam, img.device_ptr(), band=band)
            st.synchronize()
            res[name + "/rgba"] = img.download(st, np.float32).reshape(H, W, 4).copy()
            if c is not None:
                res[name + "/records"] = c.download(st).view(np.uint8).copy()
                c.release()
            img.release()
        r.destroy()
        buf.destroy()
    return res


def _child(out):
    with gpu_child.child_rig() as (gs, _, dev, st):
        np.savez(out, **render_all(gs, dev, st))


@pytest.fixture(scope="module")
def frames(gs, device, tmp_path_factory):
    """run -> the planes of every case: `rule` is this process, the pinned ones are children; each runs once, on first use"""
    tmp = tmp_path_factory.mktemp("blend_bodies")
    cache = {}

    def get(run):
        if run not in cache:
            if RUNS[run] is None:
                assert "GS3D_BLEND_GROUPS" not in os.environ and "GS3D_BLEND_FREE_BODY" not in os.environ
                st = device.create_stream()
                try:
                    cache[run] = render_all(gs, device, st)
                finally:
                    st.synchronize()
                    st.close()
            else:
                out = os.path.join(str(tmp), run + ".npz")
                gpu_child.run([os.path.abspath(__file__), out], env=RUNS[run], unset=("GS3D_BLEND_GROUPS", "GS3D_BLEND_FREE_BODY"),
                              timeout=300, label=" ".join("%s=%s" % kv for kv in sorted(RUNS[run].items())))
                cache[run] = gpu_child.load_npz(out)
        return cache[run]
    return get


_ORACLE = {}


def oracle(name):
    """the oracle's frame of a case and its lists; computed once per case"""
    if name in _ORACLE:
        return _ORACLE[name]
    ob = _ob()
    kind, W, H, mode, band = CASES[name]
    pods = ob.pack(SH, COV, scene(name))
    ogt, omt = ob.gaussian_transform(sh_deg=0, mode=mode), ob.model_transform()
    ocam = helpers.default_camera(ob, W, H)
    order = ob.spatial_order(SH, COV, pods)      # a fresh buffer's mirror order
    proj, tiles = ob.preprocess(SH, COV, pods, ogt, omt, ocam, band=band)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=ogt)
    _ORACLE[name] = dict(rgba=rgba, proj=proj, tiles=tiles, skeys=skeys, sidx=sidx, ranges=ranges, ocam=ocam, ogt=ogt,
                         tiles_x=tiles_x)
    return _ORACLE[name]


def _alpha64(proj, W, H):
    """float64 alpha of every projected Gaussian at every pixel centre: [n, H, W]"""
    p = {k: proj[k].astype(np.float64)[:, None, None] for k in ("mx", "my", "ca", "cb", "cc", "opacity")}
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    dx, dy = p["mx"] - px[None], p["my"] - py[None]
    return p["opacity"] * np.exp(p["ca"] * dx * dx + p["cb"] * dx * dy + p["cc"] * dy * dy)


def _stopped(o, cut):
    """the oracle's `stopped` flags with every tile's range cut to its first `cut` entries"""
    r = o["ranges"].copy()
    r[:, 1] = r[:, 0] + np.minimum(r[:, 1] - r[:, 0], np.uint32(cut))
    return _ob().blend(o["proj"], o["sidx"], r, o["ocam"], gt=o["ogt"], stopped=True)[1] > 0


def _check_scene(name, o):
    """the oracle's lists, flags and image are the ones the scene was built for"""
    kind, W, H, mode, band = CASES[name]
    lens = (o["ranges"][:, 1] - o["ranges"][:, 0]).astype(np.int64)
    a = o["rgba"][..., 3]
    if kind == "full":
        n = int(name.split("_")[1])
        assert list(lens) == [n], lens
        assert _alpha64(o["proj"], W, H).min() >= 1.5 / 255.0, "a splat misses a pixel: not every block list holds n entries"
    elif kind == "uneven":
        assert list(lens) == [128], lens
        al = _alpha64(o["proj"], W, H)
        assert al[0].min() >= 1.5 / 255.0
        inside = np.zeros((H, W), bool)
        inside[4:8, 4:8] = True
        assert (al[1:][:, ~inside] < 0.5 / 255.0).all(), "a tiny splat reaches a pixel outside its block"
        assert (al[1:][:, 4:8, 4:8].max(axis=(1, 2)) >= 1.5 / 255.0).all(), "a tiny splat enters no list"
    elif kind == "last_block":
        assert list(lens) == [128], lens
        lit = a > 0.0
        assert lit[12:16, 12:16].any() and not lit[:12].any() and not lit[:, :12].any(), "colour outside block (3, 3)"
    elif kind == "finish":
        n = int(name.split("_")[1])
        px, py = FINISH_PIXEL
        assert list(lens) == [n + 6 + 20], lens
        assert o["proj"]["opacity"][o["sidx"][n:n + 6]].min() >= 0.99 and o["proj"]["opacity"][o["sidx"][:n]].max() < 0.1
        # list positions 0 .. n - 1 are the faint splats, n and n + 1 the first two opaque ones: the pixel leaves at n + 1
        assert not _stopped(o, n + 1)[py, px] and _stopped(o, n + 2)[py, px]
        assert not _stopped(o, n + 2).all(), "the whole tile finishes with the pixel"
    elif kind == "finrem":
        k = int(name.split("_")[1])
        px, py = FINISH_PIXEL
        assert list(lens) == [7 + 121 + 20], lens
        op = o["proj"]["opacity"][o["sidx"]]
        assert op[:3 + k].max() < 0.1 and op[3 + k:7].min() >= 0.99 and op[7:].max() < 0.2
        # wave 0's lists of batch 1: the block of the pixel holds the first seven entries, and the 121 behind them reach no
        # pixel of the upper half: seven steps, one trip and a remainder of three; the pixel leaves at position 4 + k
        al = _alpha64(o["proj"], W, H)[o["sidx"]]
        assert (al[:7, 4:8, 4:8].max(axis=(1, 2)) >= 1.5 / 255.0).all()
        assert (al[7:128, :8, :] < 0.5 / 255.0).all(), "a tiny splat reaches the upper half"
        assert (al[128:].min(axis=(1, 2)) >= 1.5 / 255.0).all()
        assert not _stopped(o, 4 + k)[py, px] and _stopped(o, 5 + k)[py, px]
        assert not _stopped(o, 128)[:8].all(), "the whole half finishes with the pixel"
    elif kind == "boundary":
        n = boundary_stopped(name)
        assert list(lens) == [128 + 130], lens
        want = np.zeros((H, W), bool)
        want.reshape(-1)[:n] = True
        st = _stopped(o, 128)
        assert np.array_equal(st, want), "batch 1 finishes other pixels than the first %d" % n
        assert 128 - int(st[:8].sum()) == MIN_LIVE + int(name.split("_")[1])
        assert not _stopped(o, 1).any()
    elif kind == "modes":
        assert lens.min() >= 20, lens
    elif kind == "partial":
        assert list(lens) == [140], lens
    elif kind == "band":
        assert list(lens) == [0, 0, 131, 131 + 7, 0, 0], lens
    elif kind == "contrib":
        assert list(lens) == [145, 8], lens
    else:
        first = o["sidx"] < ROUND1                       # Gaussians 0 .. 2047 are the nearest 2048: round 1
        for t in range(3):
            s, e = int(o["ranges"][t, 0]), int(o["ranges"][t, 1])
            n1 = int(first[s:e].sum())
            assert first[s:s + n1].all() and n1 == ROUNDS_R1[t] and e - s - n1 == ROUNDS_R2[t], (t, n1, e - s)
        assert int((o["tiles"] > 0).sum()) == ROUND1 + sum(ROUNDS_R2)
        # round 1 leaves every tile open: its splats lie in the tile's middle, the rim stays untouched
        assert not _stopped(o, max(ROUNDS_R1)).reshape(1, 16, 3, 16).all(axis=(1, 3)).any()
    assert (a > 0.0).any()


def _same(got, want, what):
    assert np.array_equal(helpers.bits(got), helpers.bits(want)), what


def test_the_constant_is_the_kernels():
    """MIN_LIVE mirrors gs::BLEND_FREE_MIN_LIVE: the boundary scenes are built around it"""
    import re
    text = open(os.path.join(ROOT, "wgpu-3dgs-core_amd", "csrc", "gs_render_kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t BLEND_FREE_MIN_LIVE = (\d+);", text).group(1)) == MIN_LIVE


@pytest.mark.parametrize("name", [n for n in CASES if n != "rounds"])
def test_frames_equal_the_oracle(frames, name):
    kind, W, H, mode, band = CASES[name]
    o = oracle(name)
    _check_scene(name, o)
    y0, y1 = helpers.band_rows(band, H)
    exp = None
    if kind == "contrib":
        import contrib_np as cn
        exp = cn.expectation(_ob(), o["proj"], o["tiles"], o["skeys"], o["sidx"], o["ranges"], o["ocam"], o["ogt"])
        assert (exp["hits"] > 0).any()
    for run in RUNS:
        f = frames(run)
        got = f[name + "/rgba"]
        _same(got[y0:y1], o["rgba"][y0:y1], "%s: %s != oracle" % (name, run))
        if band is not None:      # rows outside the band keep the poison
            assert np.all(got[:y0] == helpers.POISON) and np.all(got[y1:] == helpers.POISON)
        if exp is not None:
            rec = f[name + "/records"].view(cn.CONTRIBUTION_DTYPE)
            assert np.array_equal(cn.raw(rec), cn.raw(exp)), "contribution records != oracle: %s" % run


def test_two_rounds_with_the_depth_and_pick_planes(gs, frames):
    from planes import oracle_depth
    name = "rounds"
    o = oracle(name)
    _check_scene(name, o)
    depth = oracle_depth(_ob(), o["proj"], o["sidx"], o["ranges"], o["ocam"], o["ogt"])
    for run in RUNS:       # (rule and the G = 8 pins: two-round frames take G = 4)
        f = frames(run)
        for frame in range(2):
            k = "%s/f%d/" % (name, frame)
            rounds, round1 = [int(x) for x in f[k + "info"]]
            assert rounds == 2 and round1 == ROUND1
            ctx = "%s, frame %d" % (run, frame)
            _same(f[k + "rgba"], o["rgba"], "colour != oracle: " + ctx)
            _same(f[k + "depth"], depth, "depth != oracle: " + ctx)
            assert np.array_equal(f[k + "pick"] != gs.PICK_NONE, f[k + "rgba"][..., 3] >= 0.5), ctx


if __name__ == "__main__":
    _child(sys.argv[1])
