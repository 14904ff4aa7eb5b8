"""GS3D_BLEND_GROUPS=8 — k_blend_grouped<MODE, 8>: 4x4 pixel blocks, eight lane groups per wave, sixteen lists per tile
 — against GS3D_BLEND_GROUPS=4 and against the oracle, bit for bit (the uint32 view of every plane).

The switch is read once per process, so every setting renders its cases in a child process (this file, run as a
script), one child at a time, and leaves the frames in an .npz the tests compare; the oracle's frames are computed once
per case in the test process.  Shapes are the small ones at which this kernel can go wrong:

  100x70   partial tiles on both edges, out-of-image lanes inside 4x4 blocks, a last tile row of 6 pixel rows;
           splat, ellipse and point mode; and the middle band of three
  48x32    6 tiles: at most 256 tiles, a tile sort of one pass; as generated, and dense (every opacity 0.99: pixels
           and whole blocks finish mid-list — `remaining`, the DEAD parking, s_alive)
  256x256  tile lists longer than two staging batches of 128 (the camera stands back far enough to see the whole
           scene: from the origin the longest list of 50 000 Gaussians is 238), two rounds pinned by GS3D_ROUNDS=1 with
           a GS3D_ROUND1 short enough that round 2 resumes tiles, with the depth and pick planes

On "finishes mid-list": a pixel's blend stops BEFORE the step that would take T below 1e-4 (oracle and kernel alike), so
no final T is below 1e-4; what the dense case asserts on the oracle's side is that the float64 walk of the oracle's
own sorted lists finds a step with T (1 - alpha) < 0.9e-4, a margin f32 rounding cannot cross, at a pixel whose final T
in the oracle's image is the T before that step."""
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
ROUND1 = 4096

# name: (W, H, N, first, mode, band, dense)
PLAIN = {
    "c100_m0": (100, 70, 20000, 0, 0, None, False),
    "c100_m1": (100, 70, 20000, 0, 1, None, False),
    "c100_m2": (100, 70, 20000, 0, 2, None, False),
    "c100_band": (100, 70, 20000, 0, 0, (2, 4), False),      # 5 tile rows in three bands: (0, 2), (2, 4), (4, 5)
    "c48": (48, 32, 3000, 0, 0, None, False),
    "c48_dense": (48, 32, 3000, 0, 0, None, True),
}
ROUNDS = {"c256": (256, 256, 50000, 0, 0, None, False)}
CAMERA = {"c256": dict(eye=(0, 0, 12), target=(0, 0, -14), vfov_deg=70.0)}      # every other case: helpers.default_camera's
SETS = {"plain": (PLAIN, {}), "rounds": (ROUNDS, {"GS3D_ROUNDS": "1", "GS3D_ROUND1": str(ROUND1)})}


def _gaussians(case):
    import synth
    W, H, n, first, mode, band, dense = case
    g = synth.scene(n, first=first)
    if dense:
        g["color"][:, 3] = 253            # 253 / 255 = 0.992: alpha = min(0.99, ...) reaches its cap at every centre
    return g


def _child(set_name, out):
    """renders every case of the set under this process's switches"""
    with gpu_child.child_rig() as (gs, _, dev, st):
        from planes import Planes
        cases = SETS[set_name][0]
        res = {}
        for name, case in cases.items():
            W, H, n, first, mode, band, dense = case
            pod = gs.GaussianPod(SH, COV)
            pods = pod.from_gaussian(_gaussians(case))
            gt = gs.gaussian_transform_pod(1.0, mode, 0, False, 3.0)
            mt = gs.model_transform_pod((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))
            cam = helpers.default_camera(gs, W, H, **CAMERA.get(name, {}))
            buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pods)
            r = gs.Renderer(dev)
            if set_name == "plain":
                img = gs.Buffer(dev, data=np.full(H * W * 4, np.float32(-7.0)))
                r.render(st, buf, gt, mt, cam, img.device_ptr(), band=band)
                st.synchronize()
                res[name + "/rgba"] = img.download(st, np.float32).reshape(H, W, 4).copy()
                img.release()
            else:
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
    gpu_child.run([os.path.abspath(__file__), set_name, out], env=dict(SETS[set_name][1], GS3D_BLEND_GROUPS=str(groups)),
                  timeout=300, label="GS3D_BLEND_GROUPS=%d %s" % (groups, set_name))
    return gpu_child.load_npz(out)


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """(groups, set) -> the child's planes; every child runs once, on first use"""
    tmp = tmp_path_factory.mktemp("blend_groups8")
    cache = {}

    def get(groups, set_name):
        if (groups, set_name) not in cache:
            cache[(groups, set_name)] = _run_child(tmp, groups, set_name)
        return cache[(groups, set_name)]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _oracle(ob, case, name=None):
    """the oracle's colour and depth planes of a case, and what its lists looked like"""
    from planes import oracle_depth
    W, H, n, first, mode, band, dense = case
    pods = ob.pack(SH, COV, _gaussians(case))
    ogt, omt = ob.gaussian_transform(sh_deg=0, mode=mode), ob.model_transform()
    ocam = helpers.default_camera(ob, W, H, **CAMERA.get(name, {}))
    order = ob.spatial_order(SH, COV, pods)      # a fresh buffer's mirror order (tests/frames.py: mirror_order)
    proj, tiles = ob.preprocess(SH, COV, pods, ogt, omt, ocam, band=band)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    keys, idx = ob.build_keys(proj, tiles, tiles_x, order=order)
    skeys, sidx = ob.sort_pairs(keys, idx)
    ranges = ob.tile_ranges(skeys, tiles_x * tiles_y)
    rgba = ob.blend(proj, sidx, ranges, ocam, band=band, gt=ogt)
    return dict(rgba=rgba, proj=proj, sidx=sidx, ranges=ranges, ocam=ocam, ogt=ogt, tiles_x=tiles_x,
                depth=lambda: oracle_depth(ob, proj, sidx, ranges, ocam, ogt, band))


def _pixels_finishing_mid_list(o, W, H):
    """float64 walk of the oracle's lists (splat mode): pixels with a step T (1 - alpha) < 0.9e-4 whose final T in the
    oracle's image is the T before that step"""
    p = {k: o["proj"][k].astype(np.float64) for k in ("mx", "my", "ca", "cb", "cc", "opacity")}
    final_T = 1.0 - o["rgba"][..., 3].astype(np.float64)
    count = 0
    for t in range(o["ranges"].shape[0]):
        s, e = int(o["ranges"][t, 0]), int(o["ranges"][t, 1])
        tx, ty = t % o["tiles_x"], t // o["tiles_x"]
        xs, ys = np.arange(tx * 16, min(tx * 16 + 16, W)), np.arange(ty * 16, min(ty * 16 + 16, H))
        px, py = [a.ravel() for a in np.meshgrid(xs + 0.5, ys + 0.5)]
        T = np.ones(px.shape)
        live = np.ones(px.shape, bool)
        stopped = np.zeros(px.shape, bool)
        for j in range(s, e):
            g = int(o["sidx"][j])
            dx, dy = p["mx"][g] - px, p["my"][g] - py
            power = p["ca"][g] * dx * dx + p["cb"][g] * dx * dy + p["cc"][g] * dy * dy
            alpha = np.minimum(0.99, p["opacity"][g] * np.exp(power))
            act = live & (power <= 0.0) & (alpha >= 1.0 / 255.0)
            Tn = T * (1.0 - alpha)
            fin = act & (Tn < 1e-4)
            stopped |= fin & (Tn < 0.9e-4)
            T = np.where(act & ~fin, Tn, T)
            live &= ~fin
        got = final_T[py.astype(int), px.astype(int)]
        count += int((stopped & (np.abs(got - T) <= 1e-6)).sum())
    return count


@pytest.mark.parametrize("name", list(PLAIN))
def test_groups8_equals_groups4_and_the_oracle(ob, frames, name):
    case = PLAIN[name]
    W, H, n, first, mode, band, dense = case
    o = _oracle(ob, case)
    y0, y1 = (0, H) if band is None else (band[0] * 16, min(band[1] * 16, H))
    if dense:
        assert _pixels_finishing_mid_list(o, W, H) >= 1, "no pixel of the dense scene finishes before its list ends"
    assert (o["ranges"][:, 1] > o["ranges"][:, 0]).any()
    g4, g8 = frames(4, "plain")[name + "/rgba"], frames(8, "plain")[name + "/rgba"]
    assert np.array_equal(_bits(g8[y0:y1]), _bits(g4[y0:y1])), "groups 8 != groups 4"
    assert np.array_equal(_bits(g8[y0:y1]), _bits(o["rgba"][y0:y1])), "groups 8 != oracle"
    assert np.array_equal(_bits(g4[y0:y1]), _bits(o["rgba"][y0:y1])), "groups 4 != oracle"
    if band is not None:      # rows outside the band keep the poison
        assert np.all(g8[:y0] == np.float32(-7.0)) and np.all(g8[y1:] == np.float32(-7.0))


def test_groups8_two_rounds_with_aux_planes(ob, gs, frames):
    name, case = "c256", ROUNDS["c256"]
    W, H = case[0], case[1]
    o = _oracle(ob, case, name)
    lens = (o["ranges"][:, 1] - o["ranges"][:, 0]).astype(np.int64)
    assert lens.max() > 2 * 128, "no tile list exceeds two staging batches (%d)" % lens.max()
    o_depth = o["depth"]()
    f4, f8 = frames(4, "rounds"), frames(8, "rounds")
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    for frame in range(2):
        k = "%s/f%d/" % (name, frame)
        for f in (f4, f8):
            rounds, round1, done = [int(x) for x in f[k + "info"]]
            assert rounds == 2 and round1 == ROUND1
            assert done < tiles, "round 1 finished every tile: round 2 resumes nothing"
        assert np.array_equal(_bits(f8[k + "rgba"]), _bits(f4[k + "rgba"])), "colour: groups 8 != groups 4 (frame %d)" % frame
        assert np.array_equal(_bits(f8[k + "depth"]), _bits(f4[k + "depth"])), "depth: groups 8 != groups 4 (frame %d)" % frame
        assert np.array_equal(f8[k + "pick"], f4[k + "pick"]), "pick: groups 8 != groups 4 (frame %d)" % frame
        assert np.array_equal(_bits(f8[k + "rgba"]), _bits(o["rgba"])), "colour: groups 8 != oracle (frame %d)" % frame
        assert np.array_equal(_bits(f8[k + "depth"]), _bits(o_depth)), "depth: groups 8 != oracle (frame %d)" % frame
        # the pick's exact relation to the alpha (1 - T is exact for T >= 0.5, tests/test_gpu_render_aux.py)
        assert np.array_equal(f8[k + "pick"] != gs.PICK_NONE, f8[k + "rgba"][..., 3] >= 0.5)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
