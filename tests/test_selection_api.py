"""Gaussian selections, the parts that need no device: the header declares the entry points, the ctypes layer binds
them (the Rust sync test of test_host_api.py then covers the bindings), and the Python layer checks the selection
keywords of a frame before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["gs_selection_create", "gs_selection_destroy", "gs_selection_len", "gs_selection_clear", "gs_selection_fill",
           "gs_selection_invert", "gs_selection_combine", "gs_selection_upload", "gs_selection_download",
           "gs_selection_count", "gs_select_sphere", "gs_select_box", "gs_renderer_select_visible", "gs_render_frame_sel"]


def _header():
    return open(os.path.join(ROOT, "include", "gs3d.h")).read()


def test_header_declares_the_selection_api(gs):
    text = _header()
    lib = gs._capi.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
    for word in ("gs_selection", "gs_frame_selection", "GS_SEL_SET", "GS_SEL_OR", "GS_SEL_AND", "GS_SEL_ANDNOT", "GS_SEL_XOR"):
        assert word in text
    # every new entry says that the reference has no such item
    section = text[text.index("Gaussian selections"):text.index("Stand-alone device primitives")]
    assert section.count("no reference item") >= len(ENTRIES) - 3
    assert (gs.SEL_SET, gs.SEL_OR, gs.SEL_AND, gs.SEL_ANDNOT, gs.SEL_XOR) == (0, 1, 2, 3, 4)
    for k, name in enumerate(["GS_SEL_SET", "GS_SEL_OR", "GS_SEL_AND", "GS_SEL_ANDNOT", "GS_SEL_XOR"]):
        assert re.search(r"%s\s*=\s*%d\b" % (name, k), text)


def test_frame_selection_struct_matches_the_header(gs):
    fs = gs.FrameSelection
    assert [f[0] for f in fs._fields_] == ["hide", "tint", "tint_rgba", "reserved"]
    assert C.sizeof(fs) == 2 * C.sizeof(C.c_void_p) + 16 + 8
    assert fs.tint_rgba.offset == 16 and fs.reserved.offset == 32


def test_select_op_names(gs):
    assert [gs.select_op(n) for n in ("set", "or", "and", "andnot", "xor")] == [0, 1, 2, 3, 4]
    assert gs.select_op("XOR") == gs.SEL_XOR and gs.select_op(3) == 3 and gs.select_op(np.int32(1)) == 1
    for bad in ("nand", 5, -1, None, 1.0, True):
        with pytest.raises(ValueError):
            gs.select_op(bad)
    assert [gs.selection_words(n) for n in (0, 1, 31, 32, 33, 100003)] == [0, 1, 1, 1, 2, 3126]
    with pytest.raises(ValueError):
        gs.selection_words(-1)


def test_render_keywords_are_checked_without_a_device(gs):
    sel = object.__new__(gs.Selection)      # a handle-less stand-in: nothing below reaches the library
    sel._h = None
    assert gs.frame_selection() is None
    with pytest.raises(TypeError):
        gs.frame_selection(hide=np.zeros(4, bool))
    with pytest.raises(TypeError):
        gs.frame_selection(tint="all", tint_rgba=(1, 0, 0, 1))
    with pytest.raises(ValueError):
        gs.frame_selection(tint_rgba=(1, 0, 0, 1))                 # a colour without a selection
    with pytest.raises(ValueError):
        gs.frame_selection(hide=sel, tint_rgba=(1, 0, 0, 1))
    with pytest.raises(ValueError):
        gs.frame_selection(tint=sel)                               # a selection without a colour
    for rgba in [(1, 0, 0), (1, 0, 0, 1, 1), (np.nan, 0, 0, 1), (0, np.inf, 0, 1), (0, 0, 0, -0.01), (0, 0, 0, 1.01),
                 (0, 0, 0, np.nan)]:
        with pytest.raises(ValueError):
            gs.frame_selection(tint=sel, tint_rgba=rgba)
    fs = gs.frame_selection(hide=sel, tint=sel, tint_rgba=(0.25, 0.5, 1.0, 0.75))
    assert list(fs.tint_rgba) == [0.25, 0.5, 1.0, 0.75] and list(fs.reserved) == [0, 0]
    fs = gs.frame_selection(hide=sel)
    assert list(fs.tint_rgba) == [0.0] * 4
    import inspect
    for fn in (gs.Renderer.render, gs.FrameRing.render):
        params = inspect.signature(fn).parameters
        assert all(params[k].default is None for k in ("hide", "tint", "tint_rgba"))


def test_box_from_bounds(gs):
    b = gs.box_from_bounds((-1, 0, 2), (3, 4, 10))
    assert b.dtype == np.float32 and b.shape == (12,)
    m = b.reshape(4, 3).T.astype(np.float64)      # 3 x 4, column-major in memory
    for p, q in [((-1, 0, 2), (-1, -1, -1)), ((3, 4, 10), (1, 1, 1)), ((1, 2, 6), (0, 0, 0))]:
        assert np.allclose(m[:, :3] @ np.array(p, float) + m[:, 3], q)
