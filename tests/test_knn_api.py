"""k nearest neighbours, the parts that need no device: the header declares the three entry points with
their notes and in their place, the ctypes layer binds them, the Rust file and the C++ mirror name them, the Python layer
refuses wrong arguments before any library call, and the restatement of tests/knn_np.py agrees with a plain loop and with
the properties of its own definition."""
import ctypes as C
import inspect
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import knn_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("gs_gaussians_buffer_knn", "gs_select_knn", "gs_knn_summary")
TITLE = "Nearest neighbours: k-NN distances, select by them, their summary"
f32, u32 = np.float32, np.uint32


def test_header_declares_the_knn_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    vp, i32, c_u32, c_f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    want = {"gs_gaussians_buffer_knn": (i32, [vp, vp, vp, vp, vp, c_u32, c_f32, vp, vp]),
            "gs_select_knn": (i32, [vp, vp, vp, c_u32, c_u32, c_f32, c_f32, i32]),
            "gs_knn_summary": (i32, [vp, vp, C.c_uint64, c_u32, c_u32, vp])}
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, text)
        assert hasattr(lib, entry), "the symbol is exported"
        assert gs._capi.SIGNATURES[entry] == want[entry]
        assert getattr(lib, entry).argtypes == want[entry][1] and getattr(lib, entry).restype == i32
    assert text.count(TITLE) == 1
    simplify = "Simplify: merge the Gaussians of each grid cell into one"
    assert text.index(simplify) < text.index("gs_gaussians_buffer_create_simplified(") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    # every comment of the section cites the design section and says that the reference has no such item
    comments = re.findall(r"/\*.*?\*/", section, flags=re.S)
    blocks = [c for c in comments if len(c) > 120]
    assert len(blocks) >= 5
    for c in blocks:
        assert "DESIGN.md 3.18" in c and "no reference item" in c, c[:80]
    for entry in ENTRIES:
        assert section.count(entry + "(") == 1
    assert "#define GS_KNN_NONE 0xFFFFFFFFu" in section and "GS_KNN_KTH_DIST2 = 0, GS_KNN_MEAN_DIST = 1" in section
    assert "typedef struct gs_knn_summary_result" in section
    # the summary record: 40 bytes, the layout of the header
    rec = gs._capi.KnnSummaryRecord
    assert C.sizeof(rec) == 40 and [(n, getattr(rec, n).offset) for n, _ in rec._fields_] == [
        ("points", 0), ("complete", 8), ("min", 16), ("max", 20), ("sum", 24), ("sum_sq", 32)]
    assert (gs.KNN_NONE, gs.KNN_MAX_K, gs.KNN_KTH_DIST2, gs.KNN_MEAN_DIST) == (0xFFFFFFFF, 16, 0, 1)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**3.18 " in design and all(e in design for e in ENTRIES)
    assert "gs_knn.hip" in design and "gs_knn.hip" in open(os.path.join(ROOT, "README.md")).read()
    assert '"gs_knn.hip"' in open(os.path.join(ROOT, "wgpu-3dgs-core_amd", "build.py")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "knn_device_code.txt"))


def test_rust_and_cpp_name_the_knn_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for entry in ENTRIES:
        assert "pub fn %s(" % entry in rs and entry + "(" in hpp
    decl = rs[rs.index("pub fn gs_gaussians_buffer_knn("):].split(";", 1)[0]
    assert "queries: *const gs_selection" in decl and "k: u32, radius: f32" in decl and "index_out: *mut gs_buffer" in decl
    decl = rs[rs.index("pub fn gs_knn_summary("):].split(";", 1)[0]
    assert "n: u64" in decl and "out: *mut gs_knn_summary_result" in decl
    assert "pub struct gs_knn_summary_result {" in rs and "pub sum_sq: f64," in rs
    assert "pub const GS_KNN_MEAN_DIST: u32 = 1;" in rs
    assert "void knn(Stream &s, uint32_t k, float radius" in hpp and "void select_knn(Stream &s" in hpp
    assert "inline gs_knn_summary_result knn_summary(Stream &s" in hpp


def _stand_in(cls, **attrs):
    """a handle-less object: nothing it is given to may reach the library"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_knn_arguments_are_checked_without_a_device(gs):
    buf = _stand_in(gs.GaussiansBuffer, pod=gs.GaussianPod(0, 0), device=None)
    sel, plane = _stand_in(gs.Selection, device=None), _stand_in(gs.Buffer, device=None)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            buf.knn(None, bad, 1.0)
        with pytest.raises(ValueError):
            buf.knn_auto(None, bad)
        with pytest.raises(ValueError):
            sel.select_knn(None, plane, bad, 0, 0.0, 1.0)
        with pytest.raises(ValueError):
            gs.knn_summary(None, plane, 4, bad)
        with pytest.raises(ValueError):
            sel.select_statistical_outliers(None, buf, k=bad)
    for bad in ("3", None, True, 3.0):
        with pytest.raises(TypeError):
            buf.knn(None, bad, 1.0)
        with pytest.raises(TypeError):
            sel.select_knn(None, plane, bad, 0, 0.0, 1.0)
    for bad in (-1.0, float("nan"), float("inf"), 1e20):          # 1e20 squared is not finite in binary32
        with pytest.raises(ValueError):
            buf.knn(None, 3, bad)
    with pytest.raises(TypeError):
        buf.knn(None, 3, "1")
    for kw in (dict(among=np.zeros(4, bool)), dict(queries=np.zeros(4, bool)), dict(model_transform=(0, 0, 0)),
               dict(dist2_out=np.zeros(12, f32)), dict(index_out=np.zeros(12, u32)), dict(indices=1)):
        with pytest.raises(TypeError):
            buf.knn(None, 3, 1.0, **kw)
    with pytest.raises(TypeError):
        buf.knn_auto(None, 3)                                      # knn_auto counts on the stream: it needs one
    # select_knn: the plane, the statistic, the bounds, the op
    with pytest.raises(TypeError):
        sel.select_knn(None, np.zeros(12, f32), 3, 0, 0.0, 1.0)
    for bad in (2, -1, "median", None, True):
        with pytest.raises(ValueError):
            sel.select_knn(None, plane, 3, bad, 0.0, 1.0)
    for lo, hi in ((float("nan"), 1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            sel.select_knn(None, plane, 3, 0, lo, hi)
    with pytest.raises(TypeError):
        sel.select_knn(None, plane, 3, 0, "0", 1.0)
    with pytest.raises(ValueError):
        sel.select_knn(None, plane, 3, 0, 0.0, 1.0, op="nand")
    # knn_summary
    with pytest.raises(TypeError):
        gs.knn_summary(None, np.zeros(12, f32), 4, 3)
    with pytest.raises(TypeError):
        gs.knn_summary(None, plane, 4.0, 3)
    with pytest.raises(ValueError):
        gs.knn_summary(None, plane, -1, 3)
    with pytest.raises(ValueError):
        gs.knn_summary(None, plane, 4, 3, "median")
    # select_statistical_outliers
    with pytest.raises(TypeError):
        sel.select_statistical_outliers(None, plane)
    with pytest.raises(TypeError):
        sel.select_statistical_outliers(None, buf, sigma="2")
    with pytest.raises(ValueError):
        sel.select_statistical_outliers(None, buf, sigma=float("nan"))
    assert gs.knn_kind("MEAN_DIST") == gs.KNN_MEAN_DIST and gs.knn_kind(0) == gs.KNN_KTH_DIST2
    p = inspect.signature(gs.GaussiansBuffer.knn).parameters
    assert list(p)[1:] == ["stream", "k", "radius", "among", "queries", "model_transform", "dist2_out", "index_out", "indices"]
    assert all(p[n].default is None for n in list(p)[4:9]) and p["indices"].default is False
    p = inspect.signature(gs.GaussiansBuffer.knn_auto).parameters
    assert list(p)[1:] == ["stream", "k", "among", "model_transform", "radius0", "max_passes"] and p["max_passes"].default == 24
    p = inspect.signature(gs.Selection.select_statistical_outliers).parameters
    assert list(p)[1:5] == ["stream", "gaussians", "k", "sigma"] and (p["k"].default, p["sigma"].default) == (8, 2.0)
    assert "gs_gaussians_buffer_knn" in gs.GaussiansBuffer.knn.__doc__ and "gs_select_knn" in gs.Selection.select_knn.__doc__
    assert "gs_knn_summary" in gs.knn_summary.__doc__
    s = gs.KnnSummary(points=4, complete=2, min=f32(1), max=f32(3), sum=4.0, sum_sq=10.0)
    assert s.mean == 2.0 and s.std == 1.0
    assert math.isnan(gs.KnnSummary(points=0, complete=0, min=f32(np.inf), max=f32(-np.inf), sum=0.0, sum_sq=0.0).mean)


def test_null_arguments_are_errors_of_the_c_abi(gs):
    """no device is touched"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    out = gs._capi.KnnSummaryRecord()
    out.points = 7
    assert lib.gs_gaussians_buffer_knn(None, None, None, None, None, 3, 1.0, None, None) == bad
    assert lib.gs_select_knn(None, None, None, 3, 0, 0.0, 1.0, 0) == bad
    assert lib.gs_knn_summary(None, None, 4, 3, 0, C.byref(out)) == bad and out.points == 7


# ---- the restatement against a plain loop and against its own definition -------------------------------------------------

def _r(x):
    """x rounded to binary32, as a Python float"""
    return struct.unpack("f", struct.pack("f", x))[0]


def _bits(x):
    return struct.unpack("I", struct.pack("f", x))[0]


def _loop_rows(p, k, radius, among):
    """the definition as a plain Python loop; every operation rounded to binary32 by a round trip through 4 bytes"""
    n = len(p)
    rr = _r(_r(radius) * _r(radius))
    pt = [bool(among[i]) and all(math.isfinite(c) for c in p[i]) for i in range(n)]
    d2_rows, ix_rows = [], []
    for i in range(n):
        if not pt[i]:
            d2_rows.append([float("nan")] * k)
            ix_rows.append([knn_np.NONE] * k)
            continue
        cand = []
        for j in range(n):
            if j == i or not pt[j]:
                continue
            d = [_r(float(p[i][a]) - float(p[j][a])) for a in range(3)]
            d2 = _r(_r(_r(d[0] * d[0]) + _r(d[1] * d[1])) + _r(d[2] * d[2]))
            if d2 <= rr:
                cand.append((_bits(d2), j, d2))
        cand.sort()
        cand = cand[:k]
        d2_rows.append([c[2] for c in cand] + [float("inf")] * (k - len(cand)))
        ix_rows.append([c[1] for c in cand] + [knn_np.NONE] * (k - len(cand)))
    return np.array(d2_rows, f32).reshape(n, k), np.array(ix_rows, u32).reshape(n, k)


def _forty():
    rng = np.random.default_rng(40)
    p = rng.uniform(-1, 1, (40, 3)).astype(f32)
    p[10:14] = p[3]                          # duplicates: ties at distance 0
    p[21] = f32([5, 5, 5])                   # and an exact tie at a distance, away from the others
    p[20] = f32([5.25, 5, 5])
    p[22] = f32([4.75, 5, 5])
    p[7, 1] = np.nan
    p[8, 0] = np.inf
    among = np.ones(40, bool)
    among[[2, 30]] = False
    return p, among


def test_restatement_equals_a_plain_loop():
    p, among = _forty()
    for k in (1, 3, 16):
        for radius in (0.0, 0.25, 0.6, 5.0):
            d2, ix = knn_np.rows(p, k, radius, among)
            ld2, lix = _loop_rows(p, k, radius, among)
            assert np.array_equal(d2.view(u32), ld2.view(u32)) and np.array_equal(ix, lix), (k, radius)
            pt, complete = knn_np.row_kinds(d2)
            assert np.array_equal(pt, knn_np.points(p, among)) and not pt[[2, 7, 8, 30]].any()
            # the statistics, by the same plain arithmetic
            kth, mean = knn_np.statistic(d2, knn_np.KTH_DIST2), knn_np.statistic(d2, knn_np.MEAN_DIST)
            for i in range(40):
                if not pt[i]:
                    assert np.isnan(kth[i]) and np.isnan(mean[i])
                elif not complete[i]:
                    assert kth[i] == np.inf and mean[i] == np.inf
                else:
                    s = _r(math.sqrt(float(d2[i, 0])))
                    for t in range(1, k):
                        s = _r(s + _r(math.sqrt(float(d2[i, t]))))
                    assert _bits(kth[i]) == _bits(float(d2[i, k - 1])) and _bits(mean[i]) == _bits(_r(s / k))
    d2, ix = knn_np.rows(p, 3, 0.0, among)
    assert np.array_equal(ix[3], [10, 11, 12]) and np.array_equal(ix[12], [3, 10, 11]) and (d2[3].view(u32) == 0).all()
    d2, ix = knn_np.rows(p, 2, 0.25, among)
    assert np.array_equal(ix[21], [20, 22]) and d2[21, 0] == d2[21, 1]      # the tie goes to the smaller caller index


def test_a_complete_row_does_not_change_when_the_radius_doubles():
    p, among = _forty()
    for k in (1, 3, 8):
        radius = 0.3
        d2, ix = knn_np.rows(p, k, radius, among)
        seen = 0
        while radius < 8.0:
            radius *= 2.0
            e2, jx = knn_np.rows(p, k, radius, among)
            _, complete = knn_np.row_kinds(d2)
            seen += int(complete.sum())
            assert np.array_equal(d2[complete].view(u32), e2[complete].view(u32)) and np.array_equal(ix[complete], jx[complete])
            # an incomplete row only grows: its entries stay a prefix
            held = np.isfinite(d2)
            assert np.array_equal(d2[held].view(u32), e2[held].view(u32)) and np.array_equal(ix[held], jx[held])
            d2, ix = e2, jx
        assert seen > 0 and knn_np.row_kinds(d2)[1].sum() == knn_np.points(p, among).sum()
    # ... and the row of k is the first k entries of the row of 16
    d16, i16 = knn_np.rows(p, 16, 0.6, among)
    for k in (1, 3, 8):
        d2, ix = knn_np.rows(p, k, 0.6, among)
        assert np.array_equal(d2.view(u32), d16[:, :k].view(u32)) and np.array_equal(ix, i16[:, :k])


def test_summary_and_range_of_the_restatement():
    p, among = _forty()
    d2, _ = knn_np.rows(p, 3, 0.6, among)
    pt, complete = knn_np.row_kinds(d2)
    assert 0 < complete.sum() < pt.sum() == 36
    for kind in (knn_np.KTH_DIST2, knn_np.MEAN_DIST):
        v = knn_np.statistic(d2, kind)
        s = knn_np.summary(d2, kind)
        assert (s["points"], s["complete"]) == (36, int(complete.sum()))
        assert s["min"] == v[complete].min() and s["max"] == v[complete].max()
        assert s["sum"] == pytest.approx(float(v[complete].astype(np.float64).sum()), rel=1e-15)
        inf = float("inf")
        assert np.array_equal(knn_np.in_range(d2, kind, inf, inf), pt & ~complete)
        assert np.array_equal(knn_np.in_range(d2, kind, -inf, inf), pt)
        assert not knn_np.in_range(d2, kind, 1.0, 0.5).any()
    none = knn_np.summary(d2[~complete & pt], knn_np.KTH_DIST2)
    assert none["complete"] == 0 and none["min"] == np.inf and none["max"] == -np.inf and none["sum"] == 0.0
