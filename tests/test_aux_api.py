"""CPU checks of the depth / pick planes' API surface (gs_render_frame_aux): the symbol is exported,
the ctypes struct matches the header's layout, the C++ and Rust mirrors carry it, and the Python keywords exist."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_frame_aux_is_exported(gs):
    lib = gs._capi.library_path()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT gs_render_frame_aux$", out, flags=re.M)
    assert re.search(r"\bT gs_render_frame$", out, flags=re.M)
    assert gs._capi.load().gs_abi_version() == 1


def test_aux_targets_layout_matches_the_header(gs):
    """sizeof / offsets of gs_aux_targets as a C compiler lays it out"""
    import tempfile
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "gs3d.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %u\n", sizeof(gs_aux_targets), offsetof(gs_aux_targets, depth),
           offsetof(gs_aux_targets, pick), offsetof(gs_aux_targets, pick_threshold), offsetof(gs_aux_targets, reserved),
           (unsigned)GS_PICK_NONE);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    A = gs.AuxTargets
    assert got[:5] == [C.sizeof(A), A.depth.offset, A.pick.offset, A.pick_threshold.offset, A.reserved.offset]
    assert C.sizeof(A) == 24
    assert got[5] == gs.PICK_NONE == 0xFFFFFFFF


def test_python_render_takes_the_planes(gs):
    for fn in (gs.Renderer.render, gs.FrameRing.render):
        params = inspect.signature(fn).parameters
        for k in ("depth_device_ptr", "pick_device_ptr", "pick_threshold"):
            assert k in params, (fn, k)
        assert params["pick_threshold"].default == 0.5
    assert gs._capi.SIGNATURES["gs_render_frame_aux"][1][-1] is C.c_void_p


def test_aux_threshold_is_checked_before_anything_else(gs):
    """No device needed: the aux arguments are checked first.  A threshold so small that 1 - t rounds to 1 in f32 would be
    a cut no step can cross; it is refused like 0, 1 and NaN.  Without planes the threshold is not looked at (the plain
    frame's own checks answer: here, the null renderer)."""
    import pytest
    fake_plane = C.c_void_p(0x10000)     # aligned, never dereferenced: the call fails before it is used
    f = gs._capi.load().gs_render_frame_aux
    args = [None] * 6 + [0, 0xFFFFFFFF, None]
    for t in (1e-9, 2.0 ** -25, 1.4e-45, 0.0, 1.0, float("nan")):
        with pytest.raises(gs.InvalidArgumentError, match="threshold"):
            gs._check(f(*args, C.byref(gs.AuxTargets(None, fake_plane, t, 0))))
    with pytest.raises(gs.InvalidArgumentError, match="null argument"):      # accepted threshold: the next check speaks
        gs._check(f(*args, C.byref(gs.AuxTargets(None, fake_plane, 2.0 ** -24, 0))))
    with pytest.raises(gs.InvalidArgumentError, match="null argument"):      # no planes: threshold 0 is not an error
        gs._check(f(*args, C.byref(gs.AuxTargets())))
    with pytest.raises(gs.InvalidArgumentError, match="reserved"):
        gs._check(f(*args, C.byref(gs.AuxTargets(None, fake_plane, 0.5, 1))))


def test_mirrors_declare_the_aux_frame():
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    assert "pub struct gs_aux_targets {" in rs and "pub fn gs_render_frame_aux(" in rs
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    assert hpp.count("const gs_aux_targets *aux") >= 2      # Renderer::render and FrameRing::render
