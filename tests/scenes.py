"""The inputs several test modules share: the layout lists, the hostile scene and its packed records, the export scene and the
selection mask sets.  Everything cached here is read-only; a test that wants to change an array copies it first."""
import hashlib
import importlib.util
import os

import numpy as np

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

ALL_LAYOUTS = [(s, c) for s in range(4) for c in range(3)]
# f32 SH + rot-scale, f16 SH + f16 cov, snorm8 + f32 cov, no SH + rot-scale
FOUR_LAYOUTS = [(0, 0), (1, 2), (2, 1), (3, 0)]
N = 5003          # no multiple of 32, 64 or 1024: four full 1024-blocks and a partial one


def hostile_scene(n, seed=3):
    """SH beyond [-1, 1] (beyond the snorm8 range too), NaN and Inf in position, SH and scale at rows 5..10"""
    g = synth.scene(n, first=seed)
    rng = np.random.default_rng(seed)
    g["color"] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    g["sh"] = rng.uniform(-1.2, 1.2, (n, 45)).astype(f32)
    if n > 10:
        g["pos"][5] = np.nan
        g["pos"][6, 1] = np.inf
        g["pos"][7] = (-np.inf, 1.0, np.nan)
        g["sh"][8, 3] = np.nan
        g["sh"][9, 4] = np.inf
        g["scale"][10] = (np.inf, 1.0, 0.0)
    return g


_PACKED = {}


def packed_pods(gs, sh, cov, n=N, seed=3, keep_hostile=False):
    """hostile_scene(n, seed) packed for one layout, as flat bytes: computed once per key, read-only.  keep_hostile: a scene
    shorter than 11 rows is the tail of an 11-row one, so it keeps some of the NaN and Inf rows"""
    key = (sh, cov, n, seed, keep_hostile)
    if key not in _PACKED:
        short = keep_hostile and n < 11
        if ("g", n, seed, short) not in _PACKED:
            _PACKED[("g", n, seed, short)] = hostile_scene(11, seed)[11 - n:] if short else hostile_scene(n, seed)
        p = np.asarray(gs.GaussianPod(sh, cov).from_gaussian(_PACKED[("g", n, seed, short)])) if n else np.zeros(0, np.uint8)
        p.setflags(write=False)
        _PACKED[key] = p
    return _PACKED[key]


def pod_rows(gs, sh, cov, n=N, seed=3):
    """packed_pods(..., keep_hostile=True) as n rows of bytes"""
    return packed_pods(gs, sh, cov, n, seed, keep_hostile=True).reshape(n, -1)


_EXPORT = {}


def golden_export():
    """tests/golden/make_golden_export.py as a module, loaded once"""
    if "module" not in _EXPORT:
        spec = importlib.util.spec_from_file_location("make_golden_export", os.path.join(ROOT, "tests", "golden", "make_golden_export.py"))
        _EXPORT["module"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_EXPORT["module"])
    return _EXPORT["module"]


def export_scene(n):
    """the scene of tests/golden/make_golden_export.py (hostile records at the wave, workgroup and block edges): once per n,
    read-only"""
    if n not in _EXPORT:
        g = golden_export().scene(n)
        g.setflags(write=False)
        _EXPORT[n] = g
    return _EXPORT[n]


def history_masks(n=N):
    """(name, mask or None) of the snapshot, statistics and neighbour tests"""
    rng = np.random.default_rng(1)
    last = np.zeros(n, bool)
    last[n - 1] = True
    tail = np.zeros(n, bool)
    tail[4992:n] = True
    but_block = np.ones(n, bool)
    but_block[1024:2048] = False
    first = np.zeros(n, bool)
    first[0] = True
    return [("random30", rng.random(n) < 0.3), ("none", np.zeros(n, bool)), ("all", None), ("last", last), ("tail", tail),
            ("all-but-block-1", but_block), ("first", first)]


def export_selections(n):
    """(name, mask or None, invert) of the export tests"""
    rng = np.random.default_rng(1000 + n)
    per_wave = np.zeros(n, bool)
    per_wave[(np.arange(0, n, 64) + rng.integers(0, 64, len(range(0, n, 64)))).clip(max=n - 1)] = True
    last = np.zeros(n, bool)
    last[-1] = True
    random30 = rng.random(n) < 0.3
    return [("none", None, False), ("empty", np.zeros(n, bool), False), ("full", np.ones(n, bool), False),
            ("inverted", random30, True), ("one-per-wave", per_wave, False), ("every-second", np.arange(n) % 2 == 0, False),
            ("random30", random30, False), ("last", last, False)]


def deflate_selections(n):
    """(name, mask or None, invert) of the fast SPZ export's round trip"""
    rng = np.random.default_rng(2000 + n)
    random30 = rng.random(n) < 0.3
    return [("none", None, False), ("empty", np.zeros(n, bool), False), ("random30", random30, False), ("inverted", random30, True)]


def upload_synth(gs, device, stream, g, step=1_000_000):
    """the synthetic scene of a golden record g (n, sh, cov) uploaded in steps; returns (pod, buffer, sha256 of the records)"""
    pod = gs.GaussianPod(g["sh"], g["cov"])
    buf = gs.GaussiansBuffer.new_empty(device, pod, g["n"])
    h = hashlib.sha256()
    for first in range(0, g["n"], step):
        cnt = min(step, g["n"] - first)
        pods = pod.from_gaussian(synth.scene(cnt, first=first))
        h.update(pods.tobytes())
        buf.update_range_with_pod(stream, first, pods)
    stream.synchronize()
    return pod, buf, h.hexdigest()


def synthetic_ply(n, seed=5):
    """PlyGaussianPod records with trained-scene statistics (log-scales around -4, logit opacities,
    unnormalised wxyz quaternions, f_dc / f_rest), plus hostile values in the first records."""
    import wgpu_3dgs_core_amd as gs
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=gs.PLY_GAUSSIAN_DTYPE)
    p["pos"] = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    p["normal"] = rng.standard_normal((n, 3)).astype(np.float32)
    p["color"] = (rng.standard_normal((n, 3)) * 1.2).astype(np.float32)
    p["sh"] = (rng.standard_normal((n, 45)) * 0.1).astype(np.float32)
    p["alpha"] = (rng.standard_normal(n) * 4.0).astype(np.float32)
    p["scale"] = (rng.standard_normal((n, 3)) * 1.5 - 4.0).astype(np.float32)
    p["rot"] = rng.standard_normal((n, 4)).astype(np.float32)
    hostile = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 88.72283, 88.72284, 89.0, -103.97207, -103.97208, -104.5,
                        -87.4, -95.0, -100.0, -103.28, 1e-30, -1e-30, 50.0, -50.0, 1e30, -1e30], dtype=np.float32)
    k = min(n, len(hostile))
    p["scale"][:k, 0] = hostile[:k]
    p["alpha"][:k] = hostile[:k]
    p["color"][:k, 1] = hostile[:k]
    if n > 30:
        p["rot"][25] = 0.0            # zero quaternion: 0 / 0 -> NaN on both sides
        p["rot"][26] = (np.inf, 1, 2, 3)
        p["rot"][27] = 1e-30          # squares underflow
    return p
