"""Snapshots, concatenation and range select, the parts that need no device: the header declares the
entry points with their notes, the ctypes layer binds them, the Rust file and the C++ mirror name them, and the Python
layer refuses wrong arguments before any library call."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNAPSHOT_ENTRIES = ["gs_gaussians_buffer_snapshot", "gs_snapshot_destroy", "gs_snapshot_len", "gs_snapshot_count",
                    "gs_snapshot_bytes", "gs_snapshot_selection", "gs_gaussians_buffer_restore",
                    "gs_gaussians_buffer_create_concat"]
ENTRIES = SNAPSHOT_ENTRIES + ["gs_select_range"]
TITLE = "Snapshots of the selected records, concatenation"


def _header():
    return open(os.path.join(ROOT, "include", "gs3d.h")).read()


def test_header_declares_the_history_api(gs):
    text = _header()
    lib = gs._capi.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
        assert getattr(lib, name).restype == gs._capi.SIGNATURES[name][0]
    assert "typedef struct gs_snapshot gs_snapshot;" in text
    # the new section sits between the edits and the stand-alone primitives, and the three older titles appear once
    for title in ("Gaussian selections", "Edits of the selected Gaussians", TITLE, "Stand-alone device primitives"):
        assert text.count(title) == 1, title
    assert text.index("Edits of the selected Gaussians") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    for name in SNAPSHOT_ENTRIES:
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.9" in comment, name
    selections = text[text.index("Gaussian selections"):text.index("Edits of the selected Gaussians")]
    comment = selections[:selections.index("gs_select_range(")].rsplit("/*", 1)[1]
    assert "no reference item" in comment and "DESIGN.md 3.7" in comment
    # widths of the scalar arguments and results
    sig = gs._capi.SIGNATURES
    assert sig["gs_snapshot_count"][0] is C.c_uint64 and sig["gs_snapshot_len"][0] is C.c_size_t
    assert sig["gs_snapshot_bytes"][0] is C.c_size_t and sig["gs_snapshot_destroy"][0] is None
    assert sig["gs_select_range"][1][2:4] == [C.c_size_t, C.c_size_t]
    assert sig["gs_gaussians_buffer_create_concat"][1][3] is C.c_uint32


def test_rust_and_cpp_name_the_history_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ENTRIES + ["pub struct gs_snapshot"]:
        assert name in rs, name
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ENTRIES + ["class Snapshot"]:
        assert name in hpp, name
    # move-only RAII
    cls = hpp[hpp.index("class Snapshot"):]
    cls = cls[:cls.index("};")]
    assert "Snapshot(const Snapshot &) = delete" in cls and "Snapshot(Snapshot &&o) noexcept" in cls and "gs_snapshot_destroy" in cls


def _stand_in(cls, **attrs):
    """a handle-less object: nothing it is given to may reach the library"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_history_arguments_are_checked_without_a_device(gs):
    pod = gs.GaussianPod(0, 0)
    buf = _stand_in(gs.GaussiansBuffer, pod=pod, device=None)
    sel = _stand_in(gs.Selection)
    snap = _stand_in(gs.Snapshot, pod=pod, device=None)
    with pytest.raises(TypeError):
        buf.snapshot(None, np.zeros(4, bool))
    with pytest.raises(TypeError):
        buf.snapshot(None, "all")
    with pytest.raises(TypeError):
        buf.restore(None, None)
    with pytest.raises(TypeError):
        buf.restore(None, sel)
    with pytest.raises(ValueError):
        buf.restore(None, snap)                       # a destroyed snapshot
    with pytest.raises(TypeError):
        snap.selection(None, np.zeros(4, bool))
    with pytest.raises(TypeError):
        snap.selection(None, None)
    with pytest.raises(ValueError):
        snap.selection(None, sel, "nand")
    with pytest.raises(TypeError):
        gs.GaussiansBuffer.concat(None, [buf, "b"])
    with pytest.raises(TypeError):
        gs.GaussiansBuffer.concat(None, [sel])
    with pytest.raises(TypeError):
        gs.GaussiansBuffer.concat(None, [buf, buf], [None, np.ones(3, bool)])
    with pytest.raises(ValueError):
        gs.GaussiansBuffer.concat(None, [buf, buf], [None])          # one selection per buffer
    with pytest.raises(ValueError):
        gs.GaussiansBuffer.concat(None, [buf], [None, sel])
    for bad in [(-1, 1), (0, -1)]:
        with pytest.raises(ValueError):
            sel.select_range(None, *bad)
    for bad in [(0.0, 1), (0, 1.5), ("0", 1), (None, 1), (True, 1)]:
        with pytest.raises(TypeError):
            sel.select_range(None, *bad)
    with pytest.raises(ValueError):
        sel.select_range(None, 0, 1, op=7)
    import inspect
    assert inspect.signature(gs.GaussiansBuffer.snapshot).parameters["selection"].default is None
    assert inspect.signature(gs.GaussiansBuffer.restore).parameters["exchange"].default is False
    assert inspect.signature(gs.GaussiansBuffer.concat).parameters["selections"].default is None
    assert inspect.signature(gs.Selection.select_range).parameters["op"].default == gs.SEL_SET
    assert inspect.signature(gs.Snapshot.selection).parameters["op"].default == gs.SEL_SET
    assert isinstance(inspect.getattr_static(gs.GaussiansBuffer, "concat"), staticmethod)
    for prop in ("len", "count", "nbytes"):
        assert isinstance(inspect.getattr_static(gs.Snapshot, prop), property)


def test_null_arguments_are_errors_of_the_c_abi(gs):
    """no device is touched: null handles and a source count outside 1..64"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    out = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_snapshot(None, None, None, C.byref(out)) == bad and out.value is None
    assert lib.gs_gaussians_buffer_restore(None, None, None, 0) == bad
    assert lib.gs_snapshot_selection(None, None, None, 0) == bad
    assert lib.gs_select_range(None, None, 0, 0, 0) == bad
    assert lib.gs_snapshot_len(None) == 0 and lib.gs_snapshot_count(None) == 0 and lib.gs_snapshot_bytes(None) == 0
    lib.gs_snapshot_destroy(None)
    src = (C.c_void_p * 65)()
    for count in (0, 65):
        out = C.c_void_p(1)
        assert lib.gs_gaussians_buffer_create_concat(None, src, None, count, C.byref(out), None) == bad
        assert out.value is None
    out = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_create_concat(None, src, None, 2, C.byref(out), None) == bad      # null sources
    assert out.value is None
    assert lib.gs_gaussians_buffer_create_concat(None, None, None, 1, C.byref(out), None) == bad
