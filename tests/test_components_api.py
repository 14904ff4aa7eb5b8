"""Connected components and the selects by cluster, the parts that need no device: the header declares
the entry points with their notes and in their place, the ctypes layer binds them, the Rust file and the C++ mirror name
them, the Python layer refuses wrong arguments before any library call, and the numpy restatement of
tests/components_np.py agrees with a plain Python flood fill."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import components_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["gs_gaussians_buffer_components", "gs_select_components", "gs_select_connected"]
TITLE = "Clusters: connected components within a radius, select by cluster size"
f32 = np.float32


def test_header_declares_the_components_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
        assert getattr(lib, name).restype == gs._capi.SIGNATURES[name][0]
    assert text.count(TITLE) == 1
    gzip_title = "Fast gzip members"
    assert text.count(gzip_title) == 1
    assert text.index(gzip_title) < text.index("gs_gaussians_buffer_export_spz_fast(") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    for name in ENTRIES:
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.16" in comment, name
    assert "#define GS_COMPONENT_NONE 0xFFFFFFFFu" in section
    struct = section[section.index("typedef struct gs_components_info"):section.index("} gs_components_info;")]
    assert re.findall(r"uint32_t\s+(\w+);", struct) == list(components_np.INFO_FIELDS)
    sig = gs._capi.SIGNATURES
    vp = C.c_void_p
    assert sig["gs_gaussians_buffer_components"][1] == [vp, vp, vp, vp, C.c_float, vp, vp, vp]
    assert sig["gs_select_components"][1][5:9] == [C.c_float, C.c_uint32, C.c_uint32, C.c_int32]
    assert sig["gs_select_connected"][1][5:8] == [C.c_float, vp, C.c_int32]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**3.16 " in design and all(name in design for name in ENTRIES)
    assert gs.COMPONENT_NONE == 0xFFFFFFFF == components_np.NONE
    assert gs.COMPONENTS_INFO_DTYPE.itemsize == 16 and gs.COMPONENTS_INFO_DTYPE.names == components_np.INFO_FIELDS


def test_rust_and_cpp_name_the_components_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ENTRIES:
        assert "pub fn %s(" % name in rs, name
        assert name in hpp, name
    assert "pub struct gs_components_info" in rs
    assert "void components(" in hpp and "void select_components(" in hpp and "void select_connected(" in hpp


def _stand_in(cls, **attrs):
    """a handle-less object: nothing it is given to may reach the library"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_component_arguments_are_checked_without_a_device(gs):
    buf = _stand_in(gs.GaussiansBuffer, pod=gs.GaussianPod(0, 0), device=None)
    sel = _stand_in(gs.Selection)
    for bad in (-1.0, float("nan"), float("inf"), 1e20, -0.5):          # 1e20 squared is not finite in binary32
        with pytest.raises(ValueError):
            buf.components(None, bad)
        with pytest.raises(ValueError):
            sel.select_components(None, buf, bad)
        with pytest.raises(ValueError):
            sel.select_connected(None, buf, bad, sel)
    for bad in ("1", None, True, (1.0,)):
        with pytest.raises(TypeError):
            buf.components(None, bad)
        with pytest.raises(TypeError):
            sel.select_components(None, buf, bad)
        with pytest.raises(TypeError):
            sel.select_connected(None, buf, bad, sel)
    with pytest.raises(TypeError):
        buf.components(None, 1.0, among=np.zeros(4, bool))
    with pytest.raises(TypeError):
        buf.components(None, 1.0, model_transform=(0, 0, 0))
    for name in ("labels_out", "sizes_out", "info_out"):
        with pytest.raises(TypeError):
            buf.components(None, 1.0, **{name: np.zeros(4, np.uint32)})
    for call in (lambda **kw: sel.select_components(None, buf, 1.0, **kw), lambda **kw: sel.select_connected(None, buf, 1.0, sel, **kw)):
        with pytest.raises(TypeError):
            call(among="all")
        with pytest.raises(TypeError):
            call(model_transform="identity")
        with pytest.raises(ValueError):
            call(op="nand")
    with pytest.raises(TypeError):
        sel.select_components(None, sel, 1.0)
    with pytest.raises(TypeError):
        sel.select_connected(None, sel, 1.0, sel)
    for bad in (None, np.zeros(4, bool), 3, buf):
        with pytest.raises(TypeError):
            sel.select_connected(None, buf, 1.0, bad)
    for name in ("min_size", "max_size"):
        for bad in (-1, 2 ** 32):
            with pytest.raises(ValueError):
                sel.select_components(None, buf, 1.0, **{name: bad})
        for bad in (1.0, "3", None, False):
            with pytest.raises(TypeError):
                sel.select_components(None, buf, 1.0, **{name: bad})
    p = inspect.signature(gs.GaussiansBuffer.components).parameters
    assert list(p)[1:] == ["stream", "radius", "among", "model_transform", "labels_out", "sizes_out", "info_out"]
    assert all(p[k].default is None for k in list(p)[3:])
    p = inspect.signature(gs.Selection.select_components).parameters
    assert list(p)[1:] == ["stream", "gaussians", "radius", "min_size", "max_size", "among", "model_transform", "op"]
    assert p["min_size"].default == 1 and p["max_size"].default == 0xFFFFFFFF and p["op"].default == gs.SEL_SET
    p = inspect.signature(gs.Selection.select_connected).parameters
    assert list(p)[1:] == ["stream", "gaussians", "radius", "seeds", "among", "model_transform", "op"]
    assert p["among"].default is None and p["model_transform"].default is None and p["op"].default == gs.SEL_SET


def test_null_arguments_are_errors_of_the_c_abi(gs):
    """no device is touched"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    assert lib.gs_gaussians_buffer_components(None, None, None, None, 1.0, None, None, None) == bad
    assert lib.gs_select_components(None, None, None, None, None, 1.0, 1, 3, 0) == bad
    assert lib.gs_select_connected(None, None, None, None, None, 1.0, None, 0) == bad


# ---- the restatement against a plain flood fill --------------------------------------------------------------------------

def _flood(pw, among, r):
    rr = f32(r) * f32(r)
    n = len(pw)
    pt = [bool(among[i]) and all(np.isfinite(pw[i])) for i in range(n)]

    def near(i, j):
        dx, dy, dz = pw[i][0] - pw[j][0], pw[i][1] - pw[j][1], pw[i][2] - pw[j][2]
        return (dx * dx + dy * dy) + dz * dz <= rr

    label, size = [components_np.NONE] * n, [0] * n
    for i in range(n):
        if not pt[i] or label[i] != components_np.NONE:
            continue
        members, stack = [i], [i]
        label[i] = i
        while stack:
            a = stack.pop()
            for b in range(n):
                if pt[b] and b != a and label[b] == components_np.NONE and near(a, b):
                    label[b] = i
                    members.append(b)
                    stack.append(b)
        for m in members:
            size[m] = len(members)
    return label, size


def test_restatement_matches_a_flood_fill():
    rng = np.random.default_rng(5)
    n = 50
    pw = rng.uniform(-1, 1, (n, 3)).astype(f32)
    pw[3] = pw[4] = pw[9]                       # duplicates
    pw[10] = pw[11] + np.array([0.25, 0, 0], f32)      # a pair at exactly r = 0.25
    assert f32(pw[10, 0] - pw[11, 0]) == f32(0.25)
    pw[20, 1] = np.nan
    pw[21, 0] = np.inf
    among = rng.random(n) < 0.8
    among[[3, 4, 9]] = True
    seen = set()
    for r in (0.0, 0.25, 0.5, 3.0):
        for m in (None, among):
            L, S, info = components_np.components(pw, r, m)
            mask = np.ones(n, bool) if m is None else m
            want_l, want_s = _flood([[f32(v) for v in p] for p in pw], mask, r)
            assert L.tolist() == want_l and S.tolist() == want_s, (r, m is None)
            assert L.dtype == np.uint32 and S.dtype == np.uint32
            assert L[20] == L[21] == components_np.NONE and S[20] == S[21] == 0
            roots = [i for i in range(n) if want_l[i] == i]
            big = max(want_s)
            assert components_np.info_tuple(info) == (sum(s > 0 for s in want_s), len(roots), big,
                                                      min(i for i in roots if want_s[i] == big))
            assert int(S[L == np.arange(n)].sum()) == info["points"]                # the sizes sum to the point count
            seen.add(info["components"])
            for lo, hi in ((1, 1), (0, components_np.UINT32_MAX), (2, 3), (5, 4), (0, 0)):
                want = [want_l[i] != components_np.NONE and lo <= want_s[i] <= hi for i in range(n)]
                assert components_np.in_size_range(S, lo, hi).tolist() == want
            seeds = np.zeros(n, bool)
            seeds[[4, 20, 30]] = True
            hit = {want_l[j] for j in (4, 20, 30) if want_l[j] != components_np.NONE}
            assert components_np.connected(L, seeds).tolist() == [want_l[i] != components_np.NONE and want_l[i] in hit for i in range(n)]
            assert not components_np.connected(L, np.zeros(n, bool)).any()
    L0, S0, _ = components_np.components(pw, 0.0)
    assert L0[[3, 4, 9]].tolist() == [3, 3, 3] and S0[[3, 4, 9]].tolist() == [3, 3, 3]
    two = np.array([[0.5, 0, 0], [0.75, 0, 0]], f32)                  # a distance of exactly r counts
    assert components_np.components(two, 0.25)[0].tolist() == [0, 0]
    assert components_np.components(two, float(np.nextafter(f32(0.25), f32(0))))[0].tolist() == [0, 1]
    assert components_np.components(pw, 3.0)[2]["components"] == 1 and len(seen) > 2
    _, _, none = components_np.components(pw[:0], 1.0)
    assert components_np.info_tuple(none) == (0, 0, 0, components_np.NONE)
    _, _, none = components_np.components(pw, 1.0, np.zeros(n, bool))
    assert components_np.info_tuple(none) == (0, 0, 0, components_np.NONE)


def test_restatement_sizes_sum_to_the_points():
    """a long chain needs many rounds of propagation: n points on a line one radius apart are one component, and none just
    below the radius"""
    n = 700
    rng = np.random.default_rng(2)
    x = (np.arange(n, dtype=f32) * f32(0.25))[rng.permutation(n)]
    pw = np.stack([x, np.zeros(n, f32), np.zeros(n, f32)], axis=1)
    L, S, info = components_np.components(pw, 0.25)
    assert (L == 0).all() and (S == n).all() and components_np.info_tuple(info) == (n, 1, n, 0)
    L, S, info = components_np.components(pw, float(np.nextafter(f32(0.25), f32(0))))
    assert np.array_equal(L, np.arange(n)) and (S == 1).all() and components_np.info_tuple(info) == (n, n, 1, 0)
    pw2 = rng.uniform(-1, 1, (600, 3)).astype(f32)
    for r in (0.05, 0.15, 0.3):
        L, S, info = components_np.components(pw2, r)
        assert int(S[L == np.arange(600)].sum()) == 600 == info["points"]
        assert info["components"] == len(np.unique(L)) and info["largest"] == S.max()
