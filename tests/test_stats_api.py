"""Attribute statistics, histograms and select by attribute range, the parts that need no device: the
header declares the entry points with their notes, the ctypes layer binds them with structs of the header's size, the Rust
file and the C++ mirror name them, the Python layer refuses wrong arguments before any library call, and the numpy
restatement of tests/stats_np.py agrees with a plain Python loop and with np.histogram."""
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

import cpp_test
import edit_np
import stats_np
from scenes import ALL_LAYOUTS, hostile_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["gs_gaussians_buffer_stats", "gs_gaussians_buffer_histogram", "gs_select_attribute"]
TITLE = "Attribute statistics, histograms and select by attribute range"
ATTRS = ["GS_ATTR_X", "GS_ATTR_Y", "GS_ATTR_Z", "GS_ATTR_RED", "GS_ATTR_GREEN", "GS_ATTR_BLUE", "GS_ATTR_OPACITY",
         "GS_ATTR_SIZE2", "GS_ATTR_DIST2", "GS_ATTR_COUNT"]
f32 = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "gs3d.h")).read()


def test_header_declares_the_stats_api(gs):
    text = _header()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
        assert getattr(lib, name).restype == gs._capi.SIGNATURES[name][0]
    assert text.count(TITLE) == 1
    assert text.index("Snapshots of the selected records, concatenation") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    for name in ENTRIES + ["gs_attribute_desc {", "gs_attribute_stats {", "gs_stats {"]:
        key = name + "(" if name in ENTRIES else name
        comment = section[:section.index(key)].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.10" in comment, name
    for k, name in enumerate(ATTRS):
        assert re.search(r"%s\s*=\s*%d\b" % (name, k), text), name
        assert getattr(gs, name[3:]) == k
    assert gs.ATTR_NAMES == [a[8:].lower() for a in ATTRS[:9]]
    sig = gs._capi.SIGNATURES
    assert sig["gs_gaussians_buffer_histogram"][1][4:7] == [C.c_float, C.c_float, C.c_uint32]
    assert sig["gs_select_attribute"][1][4:7] == [C.c_float, C.c_float, C.c_int32]


def test_rust_and_cpp_name_the_stats_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ENTRIES + ATTRS + ["pub struct gs_attribute_desc", "pub struct gs_attribute_stats", "pub struct gs_stats"]:
        assert name in rs, name
    assert "pub r#ref: [f32; 3]" in rs and "pub attr: [gs_attribute_stats; 9]" in rs      # `ref` is a Rust keyword
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ENTRIES + ["gs_stats stats(", "histogram(", "select_attribute("]:
        assert name in hpp, name


def test_structs_match_the_header(gs, tmp_path):
    d, a, st = gs._capi.AttributeDesc, gs._capi.AttributeStats, gs._capi.Stats
    assert [f[0] for f in d._fields_] == ["attr", "model_transform", "ref", "reserved"]
    assert (d.attr.offset, d.model_transform.offset, d.ref.offset, d.reserved.offset, C.sizeof(d)) == (0, 8, 16, 28, 40)
    assert (a.finite.offset, a.min.offset, a.max.offset, a.sum.offset, C.sizeof(a)) == (0, 8, 12, 16, 24)
    assert (st.count.offset, st.attr.offset, C.sizeof(st)) == (0, 8, 8 + 9 * 24)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gs3d.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(gs_attribute_desc), offsetof(gs_attribute_desc, model_transform), offsetof(gs_attribute_desc, ref), "
                   "offsetof(gs_attribute_desc, reserved), sizeof(gs_attribute_stats), offsetof(gs_attribute_stats, min), "
                   "offsetof(gs_attribute_stats, max), offsetof(gs_attribute_stats, sum), sizeof(gs_stats), offsetof(gs_stats, attr), "
                   "(int)GS_ATTR_COUNT); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(d), d.model_transform.offset, d.ref.offset, d.reserved.offset, C.sizeof(a), a.min.offset, a.max.offset,
                   a.sum.offset, C.sizeof(st), st.attr.offset, 9]


def _stand_in(cls, **attrs):
    """a handle-less object: nothing it is given to may reach the library"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_stats_arguments_are_checked_without_a_device(gs):
    buf = _stand_in(gs.GaussiansBuffer, pod=gs.GaussianPod(0, 0), device=None)
    sel = _stand_in(gs.Selection)
    with pytest.raises(TypeError):
        buf.stats(None, np.zeros(4, bool))
    with pytest.raises(TypeError):
        buf.stats(None, None, model_transform=(0, 0, 0))
    with pytest.raises(ValueError):
        buf.stats(None, None, ref=(0, 0))
    with pytest.raises(TypeError):
        buf.histogram(None, gs.ATTR_X, 0, 1, 16, selection="all")
    for bad in ("w", 9, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            buf.histogram(None, bad, 0, 1, 16)
    for bad in (0, 4097, -3):
        with pytest.raises(ValueError):
            buf.histogram(None, gs.ATTR_X, 0, 1, bad)
    for bad in (1.5, "8", None, True):
        with pytest.raises(TypeError):
            buf.histogram(None, gs.ATTR_X, 0, 1, bad)
    with pytest.raises(ValueError):
        buf.histogram(None, "dist2", 0, 1, 16, ref=(0, np.inf, 0))
    with pytest.raises(TypeError):
        sel.select_attribute(None, sel, gs.ATTR_X, 0, 1)
    with pytest.raises(ValueError):
        sel.select_attribute(None, buf, "size", 0, 1)
    with pytest.raises(ValueError):
        sel.select_attribute(None, buf, gs.ATTR_X, float("nan"), 1)
    with pytest.raises(ValueError):
        sel.select_attribute(None, buf, gs.ATTR_X, 0, float("nan"))
    with pytest.raises(ValueError):
        sel.select_attribute(None, buf, gs.ATTR_X, 0, 1, op="nand")
    with pytest.raises(ValueError):
        sel.select_attribute(None, buf, gs.ATTR_DIST2, 0, 1, ref=(np.nan, 0, 0))
    with pytest.raises(TypeError):
        sel.select_attribute(None, buf, gs.ATTR_X, 0, 1, model_transform="identity")
    # a non-finite ref is looked at only for DIST2
    d = gs.attribute_desc("opacity", None, (np.inf, 0, 0))
    assert d.attr == gs.ATTR_OPACITY and not d.model_transform and list(d.reserved) == [0, 0]
    mt = gs.model_transform_pod(pos=(1, 2, 3))
    d = gs.attribute_desc(gs.ATTR_DIST2, mt, (1, 2, 3))
    assert list(d.ref) == [1.0, 2.0, 3.0] and list(d.model_transform.contents.pos) == [1.0, 2.0, 3.0]
    assert inspect.signature(gs.GaussiansBuffer.stats).parameters["selection"].default is None
    assert inspect.signature(gs.GaussiansBuffer.stats).parameters["model_transform"].default is None
    assert inspect.signature(gs.GaussiansBuffer.histogram).parameters["selection"].default is None
    assert inspect.signature(gs.Selection.select_attribute).parameters["op"].default == gs.SEL_SET
    st = gs.GaussianStats(count=2, finite=np.array([2, 2, 0] + [0] * 6, np.uint64), min=np.zeros(9, f32), max=np.ones(9, f32),
                          sum=np.array([3.0, -1.0, 0.0] + [0.0] * 6))
    c = st.centroid
    assert c[0] == 1.5 and c[1] == -0.5 and np.isnan(c[2])
    assert np.array_equal(st.bounds[0], np.zeros(3, f32)) and np.array_equal(st.bounds[1], np.ones(3, f32))


def test_null_arguments_are_errors_of_the_c_abi(gs):
    """no device is touched"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    out = gs._capi.Stats()
    out.count = 77
    assert lib.gs_gaussians_buffer_stats(None, None, None, None, None, C.byref(out)) == bad and out.count == 77
    counts = (C.c_uint64 * 8)(*([5] * 8))
    d = gs.attribute_desc(gs.ATTR_X)
    assert lib.gs_gaussians_buffer_histogram(None, None, None, C.byref(d), 0.0, 1.0, 1, counts) == bad and list(counts) == [5] * 8
    assert lib.gs_select_attribute(None, None, None, C.byref(d), 0.0, 1.0, 0) == bad


# ---- the restatement against a plain loop ------------------------------------------------------------------------------

MT = dict(pos=(0.5, -0.25, 1.5), rot=tuple((np.array([0.3, -0.5, 0.2, 0.7]) / np.linalg.norm([0.3, -0.5, 0.2, 0.7])).astype(f32)),
          scale=(1.25, 0.75, 2.0))
REF = (0.25, -0.5, -3.0)


def _loop_attributes(sh, cov, rec):
    """one record (bytes) -> nine np.float32, scalar arithmetic in the order of DESIGN.md §3.10"""
    x, y, z = [f32(v) for v in struct.unpack_from("<3f", rec, 0)]
    qx, qy, qz, qw = [f32(v) for v in MT["rot"]]
    sx, sy, sz = [f32(v) for v in MT["scale"]]
    one = f32(1.0)
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz, yy, yz, zz, wx, wy, wz = qx * x2, qx * y2, qx * z2, qy * y2, qy * z2, qz * z2, qw * x2, qw * y2, qw * z2
    col = [[(one - (yy + zz)) * sx, (xy + wz) * sx, (xz - wy) * sx],
           [(xy - wz) * sy, (one - (xx + zz)) * sy, (yz + wx) * sy],
           [(xz + wy) * sz, (yz - wx) * sz, (one - (xx + yy)) * sz]]
    pw = [((col[0][r] * x + col[1][r] * y) + col[2][r] * z) + f32(MT["pos"][r]) for r in range(3)]
    rgba = [f32(b) / f32(255.0) for b in rec[12:16]]
    c0 = 16 + edit_np.SH_BYTES[sh]
    if cov == 0:
        rx, ry, rz, rw, ax, ay, az = [f32(v) for v in struct.unpack_from("<7f", rec, c0)]
        x2, y2, z2 = rx + rx, ry + ry, rz + rz
        xx, xy, xz, yy, yz, zz, wx, wy, wz = rx * x2, rx * y2, rx * z2, ry * y2, ry * z2, rz * z2, rw * x2, rw * y2, rw * z2
        m0 = [(one - (yy + zz)) * ax, (xy + wz) * ax, (xz - wy) * ax]
        m1 = [(xy - wz) * ay, (one - (xx + zz)) * ay, (yz + wx) * ay]
        m2 = [(xz + wy) * az, (yz - wx) * az, (one - (xx + yy)) * az]
        s = [(m0[k] * m0[k] + m1[k] * m1[k]) + m2[k] * m2[k] for k in range(3)]
    elif cov == 1:
        c6 = struct.unpack_from("<6f", rec, c0)
        s = [f32(c6[0]), f32(c6[3]), f32(c6[5])]
    else:
        c6 = struct.unpack_from("<6e", rec, c0)
        s = [f32(c6[0]), f32(c6[3]), f32(c6[5])]
    d = [pw[k] - f32(REF[k]) for k in range(3)]
    return pw + rgba + [(s[0] + s[1]) + s[2], (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]]


def _key(v):
    u = struct.unpack("<I", struct.pack("<f", float(v)))[0]
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else u | 0x80000000


@pytest.mark.parametrize("sh,cov", ALL_LAYOUTS)
def test_restatement_matches_a_plain_loop(gs, sh, cov):
    n = 100
    pod = gs.GaussianPod(sh, cov)
    assert pod.size == edit_np.pod_bytes(sh, cov)
    rows = np.asarray(pod.from_gaussian(hostile_scene(n))).reshape(n, pod.size)
    got = stats_np.attributes(sh, cov, rows, ref=REF, **MT)
    with np.errstate(all="ignore"):
        want = np.array([_loop_attributes(sh, cov, rows[i].tobytes()) for i in range(n)], f32)
    assert np.array_equal(got.view(np.uint32) | (np.isnan(got) * np.uint32(0x7FFFFFFF)),
                          want.view(np.uint32) | (np.isnan(want) * np.uint32(0x7FFFFFFF)))       # bit-equal; any NaN = any NaN
    assert np.isnan(got[5, :3]).all() and not np.isfinite(got[6, :3]).any() and np.isnan(got[7, :3]).all()      # the planted rows
    mask = np.random.default_rng(2).random(n) < 0.5
    st = stats_np.stats(got, mask)
    assert st["count"] == int(mask.sum())
    for k in range(9):
        vals = [want[i, k] for i in range(n) if mask[i] and math.isfinite(want[i, k])]
        assert st["finite"][k] == len(vals)
        lo, hi = min(vals, key=_key), max(vals, key=_key)
        assert st["min"][k].tobytes() == f32(lo).tobytes() and st["max"][k].tobytes() == f32(hi).tobytes()
        assert st["sum"][k] == math.fsum(float(v) for v in vals)
    # slots and range membership, value by value
    for k, lo, hi, bins in ((stats_np.X, -2.0, 3.0, 7), (stats_np.OPACITY, 0.0, 1.0, 256), (stats_np.DIST2, 1.0, 40.0, 1)):
        slots = stats_np.histogram_slots(got[:, k], lo, hi, bins)
        scale = f32(bins) / (f32(hi) - f32(lo))
        for i in range(n):
            v = want[i, k]
            if math.isnan(v):
                s = bins + 2
            elif v < f32(lo):
                s = bins
            elif v >= f32(hi):
                s = bins + 1
            else:
                s = min(int((v - f32(lo)) * scale), bins - 1)
            assert slots[i] == s, (k, i, v)
            assert stats_np.in_range(got[:, k], lo, hi)[i] == (not math.isnan(v) and f32(lo) <= v <= f32(hi))
    empty = stats_np.stats(got, np.zeros(n, bool))
    assert empty["count"] == 0 and not empty["finite"].any() and not empty["sum"].any()
    assert np.isposinf(empty["min"]).all() and np.isneginf(empty["max"]).all()


def test_sort_keys_order_the_zeros():
    v = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-45, -1e-45], f32)
    order = np.argsort(stats_np.sort_keys(v), kind="stable")
    assert v[order].tobytes() == np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], f32).tobytes()
    for x in v:
        assert stats_np.key_to_float(stats_np.sort_keys(np.array([x], f32))[0]).tobytes() == x.tobytes()


@pytest.mark.parametrize("attr", [stats_np.RED, stats_np.GREEN, stats_np.BLUE, stats_np.OPACITY])
def test_histogram_equals_numpy_where_both_are_exact(gs, attr):
    """lo = 0, hi = 1, bins = 256 on a byte / 255: v 256 is exact in binary32 (8 bits times a power of two), so the slot is
    floor(256 b / 255) rounded from the nearest binary32 of b / 255 — np.histogram with the edges k / 256 (exact) counts the
    same values per bin, except that it puts v == 1 into the last bin, which here is the `above` slot."""
    n = 100
    pod = gs.GaussianPod(3, 2)
    rows = np.asarray(pod.from_gaussian(hostile_scene(n))).reshape(n, pod.size)
    v = stats_np.attributes(3, 2, rows)[:, attr]
    mask = np.random.default_rng(3).random(n) < 0.4
    h = stats_np.histogram(v, 0.0, 1.0, 256, mask)
    edges = np.arange(257, dtype=np.float64) / 256.0
    for row, m in ((0, mask), (1, ~mask)):
        ref = np.histogram(v[m & (v < 1)].astype(np.float64), bins=edges)[0]
        assert np.array_equal(h[row, :256], ref.astype(np.uint64))
        assert h[row, 256] == 0 and h[row, 257] == int((v[m] == 1).sum()) and h[row, 258] == 0
        assert h[row].sum() == int(m.sum())


def test_cpp_stats_compiles():
    assert os.path.exists(cpp_test.build("stats"))
