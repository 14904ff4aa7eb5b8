"""The staging part of k_blend_grouped: a wave whose 64 lanes hold no splat skips its block tests and
its list build, and the G = 8 lists are written through a select on the ballot with a dump halfword for the non-members.
Every frame is compared bit for bit (the uint32 view of every plane) with the oracle, for GS3D_BLEND_GROUPS = 4 and 8.

The switch is read once per process, so every setting renders its cases in a child process (this file, run as a script),
one child at a time, and leaves the frames in an .npz; the oracle's frames are computed once per case in the test process.

The scenes are built, not generated: isotropic Gaussians placed on chosen pixels so that chosen tiles receive exactly n
(tile, Gaussian) pairs — the oracle's tile ranges are asserted to say so before anything is compared.

  counts   tiles 0..10 of a 4 x 3 tile image receive n = 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257 small splats:
           either side of every staging-wave (64) and batch (128) boundary.  A small splat has a standard deviation of
           half a pixel and sits in the middle 7 x 7 pixels of its tile, so that its radius square stays inside the tile in
           every display mode; some of them reach pixels of a single 4x4 block only (asserted).
  full     128 splats that reach alpha >= 1/255 at EVERY pixel of the image (asserted) lie nearest: the first batch of
           every tile is those 128, both staging waves are full and each of the 16 lists reaches the batch length — the
           last entry of the last list sits next to the dump halfword.  Behind them tile t receives k small splats, k =
           1, 30, 63, 64, 65, 0, 127, 128, 129, 2, 64, 65: a second batch that holds splats for wave 0 only (k <= 64;
           stale counts or stale list entries of wave 1 would replay the first batch's), its mirror with 65 (wave 1
           stages a single splat), and third batches of 1.

Both scenes are rendered at 64 x 48 in the three display modes and at 56 x 40 (partial tiles on both edges: the last
tile column is 8 pixels wide, the last tile row 8 pixels high); `full` also as the middle band of three, and as a
two-round frame (gs_renderer_set_rounds pinned through the API, round 1 = the nearest 200 Gaussians, so that round 2
resumes tiles) with the depth and pick planes.  A round 1 is at least 2048 Gaussians long and the renderer plans two
rounds only for more than 4096 Gaussians (gsp::plan_rounds), so that frame's scene, `full_rounds`, carries more: behind
the splats of `full` 1182 small ones in tile 5, which fill round 1 up to 2048; behind those the n small splats per tile of
`counts`, which are round 2 — every resumed tile stages a list of one of the lengths above; and 4096 Gaussians behind
the camera, which add no pair."""
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

SH, COV = 3, 0          # SH-none + rot-scale (gs.SH_NONE, gs.COV3D_ROT_SCALE)
N_COUNTS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 0)       # small splats of tile t, scene "counts"
N_BIG = 128
ROUND1 = 2048           # the shortest round 1 the renderer takes
N_FILL = ROUND1 - N_BIG - 738      # "full_rounds": small splats of tile 5 that fill round 1 (738 = sum(K_FULL))
N_PAD = 4096            # "full_rounds": Gaussians behind the camera
K_FULL = (1, 30, 63, 64, 65, 0, 127, 128, 129, 2, 64, 65)                # small splats of tile t behind the 128, scene "full"
assert sum(K_FULL) == 738

# name: (scene, W, H, mode, band)
PLAIN = {
    "counts64_m0": ("counts", 64, 48, 0, None),
    "counts64_m1": ("counts", 64, 48, 1, None),
    "counts64_m2": ("counts", 64, 48, 2, None),
    "counts56_m0": ("counts", 56, 40, 0, None),
    "full64_m0": ("full", 64, 48, 0, None),
    "full64_m1": ("full", 64, 48, 1, None),
    "full64_m2": ("full", 64, 48, 2, None),
    "full56_m0": ("full", 56, 40, 0, None),
    "full64_band": ("full", 64, 48, 0, (1, 2)),       # 3 tile rows in three bands: (0, 1), (1, 2), (2, 3)
}
ROUNDS = {"full64_rounds": ("full_rounds", 64, 48, 0, None)}


def _small_counts(scene):
    """small splats of every tile: one count per depth layer, the nearest layer first"""
    if scene == "counts":
        return [[k] for k in N_COUNTS]
    if scene == "full":
        return [[k] for k in K_FULL]
    return [[K_FULL[t], N_FILL if t == 5 else 0, N_COUNTS[t]] for t in range(12)]
SETS = {"plain": PLAIN, "rounds": ROUNDS}


def _gaussians(scene, W, H):
    """the built scene; Gaussian i of the array is NOT the i-th in depth (the small splats' depths are shuffled)"""
    import synth
    cam = helpers.default_camera(__import__("oracle.binding", fromlist=["binding"]), W, H)
    rng = np.random.RandomState(1234 + W)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    assert tiles_x * tiles_y == 12
    small = _small_counts(scene)
    px, py, sig, z, col = [], [], [], [], []
    if scene != "counts":
        for i in range(N_BIG):
            px.append(W / 2 + rng.uniform(-8, 8))
            py.append(H / 2 + rng.uniform(-8, 8))
            sig.append(rng.uniform(40.0, 60.0))
            z.append(3.0 + 0.002 * i)
            col.append((rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(3, 6)))
    for layer in range(len(small[0])):      # a layer lies behind the one before: depths 4 .. 5.5, 5.5 .. 7, 7 .. 8.5
        depth_rank = rng.permutation(sum(c[layer] for c in small))
        j = 0
        for t in range(12):
            tx, ty = t % tiles_x, t // tiles_x
            # the middle 7 x 7 pixels of the tile, cut to what the image shows of it
            x_hi = min(11.5, W - tx * 16 - 1.5)
            y_hi = min(11.5, H - ty * 16 - 1.5)
            for _ in range(small[t][layer]):
                if rng.randint(4) == 0:      # on the centre of an inner 4x4 block: its pixels only
                    px.append(tx * 16 + (6.0 if x_hi < 10.0 else rng.choice([6.0, 10.0])))
                    py.append(ty * 16 + (6.0 if y_hi < 10.0 else rng.choice([6.0, 10.0])))
                else:
                    px.append(tx * 16 + rng.uniform(4.5, x_hi))
                    py.append(ty * 16 + rng.uniform(4.5, y_hi))
                sig.append(0.5)
                z.append(4.0 + 1.5 * layer + 0.001 * depth_rank[j])
                col.append((rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(20, 50)))
                j += 1
    if scene == "full_rounds":
        for i in range(N_PAD):
            px.append(rng.uniform(0, W))
            py.append(rng.uniform(0, H))
            sig.append(2.0)
            z.append(-(1.0 + 0.001 * i))      # z > 0 in camera space is behind the camera
            col.append((255, 255, 255, 255))
    n = len(px)
    px, py, sig, z = [np.asarray(a, dtype=np.float64) for a in (px, py, sig, z)]
    g = np.zeros(n, dtype=synth.GAUSSIAN_DTYPE)
    g["rot"][:] = (0.0, 0.0, 0.0, 1.0)
    g["pos"][:, 0] = (px - cam.cx) / cam.fx * z
    g["pos"][:, 1] = -(py - cam.cy) / cam.fy * z
    g["pos"][:, 2] = -z
    g["scale"][:] = np.abs(sig * z / cam.fx)[:, None]
    g["color"][:] = np.asarray(col, dtype=np.uint8)
    return g


def _child(set_name, out):
    """renders every case of the set under this process's switches"""
    with gpu_child.child_rig() as (gs, _, dev, st):
        from planes import Planes
        res = {}
        for name, (scene, W, H, mode, band) in SETS[set_name].items():
            pod = gs.GaussianPod(SH, COV)
            pods = pod.from_gaussian(_gaussians(scene, W, H))
            gt = gs.gaussian_transform_pod(1.0, mode, 0, False, 3.0)
            mt = gs.model_transform_pod((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))
            cam = helpers.default_camera(gs, W, H)
            buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pods)
            r = gs.Renderer(dev)
            if set_name == "plain":
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


def _run_child(tmp, groups, set_name):
    out = os.path.join(str(tmp), "g%d_%s.npz" % (groups, set_name))
    gpu_child.run([os.path.abspath(__file__), set_name, out], env={"GS3D_BLEND_GROUPS": str(groups)}, timeout=300,
                  label="GS3D_BLEND_GROUPS=%d %s" % (groups, set_name))
    return gpu_child.load_npz(out)


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """(groups, set) -> the child's planes; every child runs once, on first use"""
    tmp = tmp_path_factory.mktemp("blend_staging")
    cache = {}

    def get(groups, set_name):
        if (groups, set_name) not in cache:
            cache[(groups, set_name)] = _run_child(tmp, groups, set_name)
        return cache[(groups, set_name)]
    return get


_ORACLE = {}


def _oracle(ob, name, case):
    """the oracle's planes of a case and what its lists look like; computed once per case"""
    if name in _ORACLE:
        return _ORACLE[name]
    from planes import oracle_depth
    scene, W, H, mode, band = case
    pods = ob.pack(SH, COV, _gaussians(scene, W, H))
    ogt, omt = ob.gaussian_transform(sh_deg=0, mode=mode), ob.model_transform()
    ocam = helpers.default_camera(ob, W, H)
    order = ob.spatial_order(SH, COV, pods)      # a fresh buffer's mirror order (tests/frames.py: mirror_order)
    proj, tiles = ob.preprocess(SH, COV, pods, ogt, omt, ocam, band=band)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=ogt)
    _ORACLE[name] = dict(rgba=rgba, proj=proj, sidx=sidx, ranges=ranges, tiles_x=tiles_x, tiles_y=tiles_y,
                         depth=lambda: oracle_depth(ob, proj, sidx, ranges, ocam, ogt, band))
    return _ORACLE[name]


def _alpha(o, g, xs, ys):
    """opacity x exp(power) of projected Gaussian g at the pixel centres xs x ys (float64)"""
    p = {k: float(o["proj"][k][g]) for k in ("mx", "my", "ca", "cb", "cc", "opacity")}
    dx, dy = np.meshgrid(p["mx"] - (xs + 0.5), p["my"] - (ys + 0.5))
    return p["opacity"] * np.exp(p["ca"] * dx * dx + p["cb"] * dx * dy + p["cc"] * dy * dy)


def _check_scene(o, case):
    """the oracle's lists are the ones the scene was built for"""
    scene, W, H, mode, band = case
    lens = (o["ranges"][:, 1] - o["ranges"][:, 0]).astype(np.int64)
    rows = range(o["tiles_y"]) if band is None else range(band[0], band[1])
    n_front = 0 if scene == "counts" else N_BIG
    small = [sum(c) for c in _small_counts(scene)]
    for t in range(12):
        if t // o["tiles_x"] not in rows:
            continue
        assert lens[t] == n_front + small[t], "tile %d receives %d pairs, built for %d" % (t, lens[t], n_front + small[t])
        s = int(o["ranges"][t, 0])
        if scene != "counts":      # the first batch is the 128 large splats: opacity bytes 3..5, the small ones' are 20..49
            assert o["proj"]["opacity"][o["sidx"][s:s + N_BIG]].max() < 6.0 / 255.0
            assert lens[t] == N_BIG or o["proj"]["opacity"][o["sidx"][s + N_BIG:s + lens[t]]].min() > 19.0 / 255.0
    if mode != 0:
        return
    if scene != "counts":
        # the first 128 entries of tile 0 reach alpha >= 1/255 at every pixel of the image: every list of every tile
        # holds all of them
        s = int(o["ranges"][0, 0])
        for g in o["sidx"][s:s + N_BIG]:
            assert _alpha(o, int(g), np.arange(W), np.arange(H)).min() >= 1.01 / 255.0
    else:
        # some small splat of tile 4 (127 of them) reaches alpha >= 1/255 at pixels of one 4x4 block only
        s, e = int(o["ranges"][4, 0]), int(o["ranges"][4, 1])
        tx, ty = 4 % o["tiles_x"], 4 // o["tiles_x"]
        blocks = []
        for g in o["sidx"][s:e]:
            a = _alpha(o, int(g), tx * 16 + np.arange(16), ty * 16 + np.arange(16)) >= 1.0 / 255.0
            blocks.append(int(a.reshape(4, 4, 4, 4).any(axis=(1, 3)).sum()))
        assert min(blocks) == 1 and max(blocks) > 1, (min(blocks), max(blocks))


@pytest.mark.parametrize("name", list(PLAIN))
def test_staging_equals_the_oracle(ob, frames, name):
    case = PLAIN[name]
    scene, W, H, mode, band = case
    o = _oracle(ob, name, case)
    _check_scene(o, case)
    y0, y1 = helpers.band_rows(band, H)
    for groups in (4, 8):
        got = frames(groups, "plain")[name + "/rgba"]
        assert np.array_equal(helpers.bits(got[y0:y1]), helpers.bits(o["rgba"][y0:y1])), "groups %d != oracle" % groups
        if band is not None:      # rows outside the band keep the poison
            assert np.all(got[:y0] == helpers.POISON) and np.all(got[y1:] == helpers.POISON)
    # the frame is not a trivial one: the splats show
    assert (o["rgba"][y0:y1, :, 3] > 0.0).any()


def test_staging_two_rounds_with_aux_planes(ob, gs, frames):
    name, case = "full64_rounds", ROUNDS["full64_rounds"]
    scene, W, H, mode, band = case
    o = _oracle(ob, name, case)
    _check_scene(o, case)
    o_depth = o["depth"]()
    f4, f8 = frames(4, "rounds"), frames(8, "rounds")
    for frame in range(2):
        k = "%s/f%d/" % (name, frame)
        for groups, f in ((4, f4), (8, f8)):
            rounds, round1, done = [int(x) for x in f[k + "info"]]
            assert rounds == 2 and round1 == ROUND1
            assert done < 12, "round 1 finished every tile: round 2 resumes nothing"
            ctx = "groups %d, frame %d" % (groups, frame)
            assert np.array_equal(helpers.bits(f[k + "rgba"]), helpers.bits(o["rgba"])), "colour != oracle: " + ctx
            assert np.array_equal(helpers.bits(f[k + "depth"]), helpers.bits(o_depth)), "depth != oracle: " + ctx
            # the pick's exact relation to the alpha (1 - T is exact for T >= 0.5, tests/test_gpu_render_aux.py)
            assert np.array_equal(f[k + "pick"] != gs.PICK_NONE, f[k + "rgba"][..., 3] >= 0.5), ctx
        assert np.array_equal(f8[k + "pick"], f4[k + "pick"]), "pick: groups 8 != groups 4 (frame %d)" % frame


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
