"""CPU checks of the contribution scores' API surface (gs_render_frame_contrib, gs_contributions_clear,
gs_select_contribution): the symbols are exported, the record matches the header's layout, the C++ and Rust
mirrors carry them, the Python keywords exist, and the argument checks that need no device answer."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gs_render_frame_contrib", "gs_contributions_clear", "gs_select_contribution"]


def test_contribution_symbols_are_exported(gs):
    lib = gs._capi.library_path()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
        assert name in gs._capi.SIGNATURES
    assert gs._capi.load().gs_abi_version() == 1


def test_contribution_record_layout_matches_the_header(gs):
    """sizeof / offsets of gs_contribution as a C compiler lays it out, and the kinds"""
    import tempfile
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "gs3d.h"
int main(void) {
    printf("%zu %zu %zu %zu %d %d %d\n", sizeof(gs_contribution), offsetof(gs_contribution, sum), offsetof(gs_contribution, hits),
           offsetof(gs_contribution, wmax), (int)GS_CONTRIB_SUM, (int)GS_CONTRIB_HITS, (int)GS_CONTRIB_MAX);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    dt = gs.CONTRIBUTION_DTYPE
    assert got[:4] == [16, 0, 8, 12]
    assert got[:4] == [dt.itemsize, dt.fields["sum"][1], dt.fields["hits"][1], dt.fields["wmax"][1]]
    assert (dt.fields["sum"][0], dt.fields["hits"][0], dt.fields["wmax"][0]) == (np.dtype("<u8"), np.dtype("<u4"), np.dtype("<f4"))
    assert got[4:] == [gs.CONTRIB_SUM, gs.CONTRIB_HITS, gs.CONTRIB_MAX] == [0, 1, 2]


def test_python_signatures(gs):
    for fn in (gs.Renderer.render, gs.FrameRing.render):
        params = inspect.signature(fn).parameters
        assert "contributions" in params and params["contributions"].default is None, fn
    sig = gs._capi.SIGNATURES
    assert sig["gs_render_frame_contrib"] == (C.c_int32, [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3)
    assert sig["gs_contributions_clear"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t])
    assert sig["gs_select_contribution"][1][3:] == [C.c_uint32, C.c_float, C.c_float, C.c_int32]
    for name in ("new", "clear", "download", "select", "release"):
        assert callable(getattr(gs.Contributions, name)), name
    assert list(inspect.signature(gs.Contributions.select).parameters)[1:] == ["stream", "selection", "kind", "lo", "hi", "op"]


def test_mirrors_declare_the_contribution_calls():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    assert "pub struct gs_contribution {" in rs
    for name in ENTRIES:
        assert "pub fn %s(" % name in rs, name
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ENTRIES:
        assert name + "(" in hpp, name
    header = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    assert header.index("/* Export (DESIGN.md 3.13") < header.index("Contribution scores (DESIGN.md 3.5c") < header.index("Stand-alone device primitives")
    assert "could not undo" in header      # why a contribution frame is planned as one round


def test_argument_checks_that_need_no_device(gs):
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    frame = [None] * 6 + [0, 0xFFFFFFFF, None]
    with pytest.raises(gs.InvalidArgumentError, match="null argument"):
        gs._check(lib.gs_render_frame_contrib(*frame, None, None))
    fs = gs.FrameSelection()
    fs.reserved[0] = 1
    with pytest.raises(gs.InvalidArgumentError, match="reserved"):     # the selection is checked as gs_render_frame_sel checks it
        gs._check(lib.gs_render_frame_contrib(*frame, C.byref(fs), None))
    assert lib.gs_contributions_clear(None, None, 0) == bad
    assert lib.gs_contributions_clear(None, None, 16) == bad
    for kind, lo, hi, op in ((0, 0.0, 1.0, 0), (7, 0.0, 1.0, 0), (0, float("nan"), 1.0, 0), (0, 0.0, 1.0, 9)):
        assert lib.gs_select_contribution(None, None, None, kind, lo, hi, op) == bad


def test_python_helper_checks(gs):
    with pytest.raises(ValueError, match="planes"):
        gs.Renderer.render(object.__new__(gs.Renderer), None, None, None, None, None, 0, depth_device_ptr=16, contributions=object())
