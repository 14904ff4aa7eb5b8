"""Neighbour counts and select by neighbourhood, the parts that need no device: the header declares the
entry points with their notes and in their place, the ctypes layer binds them, the Rust file and the C++ mirror name them,
the Python layer refuses wrong arguments before any library call, and the numpy restatement of tests/neighbors_np.py
agrees with a plain Python loop and is symmetric."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import neighbors_np
from scenes import hostile_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["gs_gaussians_buffer_neighbor_counts", "gs_select_neighbors"]
TITLE = "Neighbour counts and select by neighbourhood"
f32 = np.float32


def test_header_declares_the_neighbor_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
        assert getattr(lib, name).restype == gs._capi.SIGNATURES[name][0]
    assert text.count(TITLE) == 1
    stats_title = "Attribute statistics, histograms and select by attribute range"
    assert text.index(stats_title) < text.index("gs_select_attribute(") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    for name in ENTRIES:
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.11" in comment, name
    sig = gs._capi.SIGNATURES
    assert sig["gs_gaussians_buffer_neighbor_counts"][1][4:6] == [C.c_float, C.c_uint32]
    assert sig["gs_select_neighbors"][1][5:9] == [C.c_float, C.c_uint32, C.c_uint32, C.c_int32]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**3.11 " in design and all(name in design for name in ENTRIES)


def test_rust_and_cpp_name_the_neighbor_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ENTRIES:
        assert "pub fn %s(" % name in rs, name
        assert name in hpp, name
    assert "void neighbor_counts(" in hpp and "void select_neighbors(" in hpp


def _stand_in(cls, **attrs):
    """a handle-less object: nothing it is given to may reach the library"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_neighbor_arguments_are_checked_without_a_device(gs):
    buf = _stand_in(gs.GaussiansBuffer, pod=gs.GaussianPod(0, 0), device=None)
    sel = _stand_in(gs.Selection)
    for bad in (-1.0, float("nan"), float("inf"), 1e20, -0.5):          # 1e20 squared is not finite in binary32
        with pytest.raises(ValueError):
            buf.neighbor_counts(None, bad)
        with pytest.raises(ValueError):
            sel.select_neighbors(None, buf, bad)
    for bad in ("1", None, True, (1.0,)):
        with pytest.raises(TypeError):
            buf.neighbor_counts(None, bad)
        with pytest.raises(TypeError):
            sel.select_neighbors(None, buf, bad)
    for bad in (0, -1, 2 ** 32):
        with pytest.raises(ValueError):
            buf.neighbor_counts(None, 1.0, cap=bad)
    for bad in (1.5, "8", None, True):
        with pytest.raises(TypeError):
            buf.neighbor_counts(None, 1.0, cap=bad)
    with pytest.raises(TypeError):
        buf.neighbor_counts(None, 1.0, among=np.zeros(4, bool))
    with pytest.raises(TypeError):
        buf.neighbor_counts(None, 1.0, model_transform=(0, 0, 0))
    with pytest.raises(TypeError):
        buf.neighbor_counts(None, 1.0, out=np.zeros(4, np.uint32))
    with pytest.raises(TypeError):
        sel.select_neighbors(None, sel, 1.0)
    with pytest.raises(TypeError):
        sel.select_neighbors(None, buf, 1.0, among="all")
    with pytest.raises(TypeError):
        sel.select_neighbors(None, buf, 1.0, model_transform="identity")
    for name in ("min_count", "max_count"):
        for bad in (-1, 2 ** 32):
            with pytest.raises(ValueError):
                sel.select_neighbors(None, buf, 1.0, **{name: bad})
        for bad in (1.0, "3", None, False):
            with pytest.raises(TypeError):
                sel.select_neighbors(None, buf, 1.0, **{name: bad})
    with pytest.raises(ValueError):
        sel.select_neighbors(None, buf, 1.0, op="nand")
    p = inspect.signature(gs.GaussiansBuffer.neighbor_counts).parameters
    assert list(p)[1:] == ["stream", "radius", "cap", "among", "model_transform", "out"]
    assert p["cap"].default == 0xFFFFFFFF and p["among"].default is None and p["model_transform"].default is None and p["out"].default is None
    p = inspect.signature(gs.Selection.select_neighbors).parameters
    assert list(p)[1:] == ["stream", "gaussians", "radius", "min_count", "max_count", "among", "model_transform", "op"]
    assert p["min_count"].default == 0 and p["max_count"].default == 0xFFFFFFFF and p["op"].default == gs.SEL_SET


def test_null_arguments_are_errors_of_the_c_abi(gs):
    """no device is touched"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    assert lib.gs_gaussians_buffer_neighbor_counts(None, None, None, None, 1.0, 16, None) == bad
    assert lib.gs_select_neighbors(None, None, None, None, None, 1.0, 0, 3, 0) == bad


# ---- the restatement against a plain loop ------------------------------------------------------------------------------

def _loop_counts(pw, among, r):
    rr = f32(r) * f32(r)
    n = len(pw)
    pt = [bool(among[i]) and all(np.isfinite(pw[i])) for i in range(n)]
    out = [0] * n
    for i in range(n):
        if not pt[i]:
            continue
        for j in range(n):
            if j == i or not pt[j]:
                continue
            dx, dy, dz = pw[i][0] - pw[j][0], pw[i][1] - pw[j][1], pw[i][2] - pw[j][2]
            if (dx * dx + dy * dy) + dz * dz <= rr:
                out[i] += 1
    return out


def test_restatement_matches_a_plain_loop():
    rng = np.random.default_rng(5)
    n = 50
    pw = rng.uniform(-1, 1, (n, 3)).astype(f32)
    pw[3] = pw[4] = pw[9]                       # duplicates
    pw[10] = pw[11] + np.array([0.25, 0, 0], f32)
    pw[20, 1] = np.nan
    pw[21, 0] = np.inf
    among = rng.random(n) < 0.8
    among[[3, 4, 9]] = True
    for r in (0.0, 0.25, 0.5, 3.0):
        for m in (None, among):
            got = neighbors_np.counts(pw, r, m)
            want = _loop_counts([[f32(v) for v in p] for p in pw], np.ones(n, bool) if m is None else m, r)
            assert got.tolist() == want, (r, m is None)
            assert got[20] == 0 and got[21] == 0
    assert neighbors_np.counts(pw, 0.0)[[3, 4, 9]].tolist() == [2, 2, 2]
    assert neighbors_np.counts(pw, 3.0).max() == n - 3                 # everything finite but itself
    c = neighbors_np.counts(pw, 0.5, among)
    pt = neighbors_np.points(pw, among)
    assert not pt[20] and not pt[21] and (c[~pt] == 0).all()
    assert np.array_equal(neighbors_np.in_count_range(c, pt, 0, 2 ** 32 - 1), pt)
    assert not neighbors_np.in_count_range(c, pt, 3, 2).any()
    assert neighbors_np.capped(c, 2).max() == 2 and neighbors_np.capped(c, 2).dtype == np.uint32


def test_restatement_is_symmetric():
    """the number of (i, j) pairs is the number of (j, i) pairs: sum of counts = twice the unordered pairs, and the count
    of a chunked run equals that of a run in one block (n > CHUNK)"""
    rng = np.random.default_rng(6)
    n = 2 * neighbors_np.CHUNK + 37
    pw = rng.uniform(-1, 1, (n, 3)).astype(f32)
    r = 0.2
    c = neighbors_np.counts(pw, r)
    d = pw[:, None, :] - pw[None, :, :]
    near = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= f32(r) * f32(r)
    assert np.array_equal(near, near.T)
    np.fill_diagonal(near, False)
    assert np.array_equal(c, near.sum(axis=1)) and c.sum() == 2 * np.triu(near).sum()


def test_positions_are_those_of_the_stats_restatement(gs):
    import stats_np
    pod = gs.GaussianPod(1, 2)
    rows = np.asarray(pod.from_gaussian(hostile_scene(40))).reshape(40, pod.size)
    mt = dict(pos=(0.5, -0.25, 1.5), rot=(0.0, 0.0, 0.0, 1.0), scale=(1.25, 0.75, 2.0))
    pw = neighbors_np.positions(rows, **mt)
    want = stats_np.attributes(1, 2, rows, **mt)[:, :3]
    assert np.array_equal(pw.view(np.uint32) | (np.isnan(pw) * np.uint32(0x7FFFFFFF)),
                          want.view(np.uint32) | (np.isnan(want) * np.uint32(0x7FFFFFFF)))
    assert not neighbors_np.points(pw)[5:8].any()
