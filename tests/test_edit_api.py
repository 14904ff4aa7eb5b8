"""Edits of the selected Gaussians, the parts that need no device: the header declares the entry points,
the ctypes layer binds them, the Rust file is in sync, gs_edit has one size on both sides, the SH rotation matrices have
their defining property, and the Python builders produce what they document."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["gs_gaussians_buffer_edit", "gs_gaussians_buffer_create_from_selection", "gs_sh_rotation_matrices"]


def _header():
    return open(os.path.join(ROOT, "include", "gs3d.h")).read()


def test_header_declares_the_edit_api(gs):
    text = _header()
    lib = gs._capi.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
        assert getattr(lib, name).restype == gs._capi.SIGNATURES[name][0]
    section = text[text.index("Edits of the selected Gaussians"):text.index("Stand-alone device primitives")]
    # every entry point carries the note and cites the design section: the comment in front of its declaration
    for name in ENTRIES:
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.8" in comment, name
    for k, name in zip((1, 2, 4, 8), ["GS_EDIT_TRANSFORM", "GS_EDIT_ROTATE_SH", "GS_EDIT_COLOR", "GS_EDIT_OPACITY"]):
        assert re.search(r"%s\s*=\s*%d\b" % (name, k), text)
    assert (gs.EDIT_TRANSFORM, gs.EDIT_ROTATE_SH, gs.EDIT_COLOR, gs.EDIT_OPACITY) == (1, 2, 4, 8)
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for word in ("gs_gaussians_buffer_edit", "gs_gaussians_buffer_create_from_selection", "gs_sh_rotation_matrices"):
        assert word in hpp


def test_rust_bindings_are_in_sync():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ENTRIES + ["pub struct gs_edit", "GS_EDIT_ROTATE_SH"]:
        assert name in rs, name


def test_edit_struct_matches_the_header(gs, tmp_path):
    e = gs.Edit
    assert [f[0] for f in e._fields_] == ["flags", "transform", "color", "opacity", "reserved"]
    assert (e.flags.offset, e.transform.offset, e.color.offset, e.opacity.offset, e.reserved.offset) == (0, 4, 52, 100, 108)
    assert C.sizeof(e) == 124
    # ... and the C compiler agrees
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gs3d.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(gs_edit), offsetof(gs_edit, transform), offsetof(gs_edit, color), offsetof(gs_edit, opacity), "
                   "offsetof(gs_edit, reserved)); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(e), e.transform.offset, e.color.offset, e.opacity.offset, e.reserved.offset]


# ---- the basis of DESIGN.md §3.2, written from the text: constants of Kerbl et al., zero-based rest coefficients ----

def _basis(d):
    """d: m x 3 unit vectors -> m x 15 (bands 1, 2, 3)"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    C1 = 0.4886025119029199
    C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
    C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
          1.445305721320277, -0.5900435899266435]
    return np.stack([-C1 * y, C1 * z, -C1 * x,
                     C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                     C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy),
                     C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
                     C3[6] * x * (xx - 3 * yy)], axis=1)


def _rot64(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _unit(rng, m, k):
    v = rng.normal(size=(m, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _block(ds):
    D = np.zeros((15, 15))
    for first, d in zip((0, 3, 8), ds):
        D[first:first + len(d), first:first + len(d)] = d.astype(np.float64)
    return D


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def test_sh_rotation_identity_and_shapes(gs):
    d1, d2, d3 = gs.sh_rotation_matrices((0, 0, 0, 1))
    assert (d1.shape, d2.shape, d3.shape) == ((3, 3), (5, 5), (7, 7)) and d1.dtype == np.float32
    for d in (d1, d2, d3):
        assert np.array_equal(d, np.eye(len(d), dtype=np.float32))
    # -q is the same rotation; a scaled quaternion is normalised
    q = np.array([0.3, -0.5, 0.2, 0.7])
    a, b, c = gs.sh_rotation_matrices(q), gs.sh_rotation_matrices(-q), gs.sh_rotation_matrices(3.0 * q)
    for k in range(3):
        assert np.abs(a[k] - b[k]).max() <= 1e-6 and np.abs(a[k] - c[k]).max() <= 1e-6
    for bad in [(0, 0, 0, 0), (np.nan, 0, 0, 1), (np.inf, 0, 0, 1)]:
        with pytest.raises(gs.InvalidArgumentError):
            gs.sh_rotation_matrices(bad)


def test_sh_rotation_is_a_homomorphism(gs):
    rng = np.random.default_rng(11)
    for _ in range(50):
        q1, q2 = _unit(rng, 2, 4)
        q12 = _qmul(q1, q2)                      # the rotation R(q1) R(q2)
        D1, D2, D12 = (_block(gs.sh_rotation_matrices(q)) for q in (q1, q2, q12))
        assert np.abs(D12 - D1 @ D2).max() <= 1e-6


def test_sh_rotation_defining_property(gs):
    """for every unit d: sum_k Y_k(d) c'_k = sum_k Y_k(R^T d) c_k with c' = D c, evaluated in float64 for 200 random
    rotations x 200 directions x random coefficients in [-1, 1].  Bound 1e-5, derived: D is exact up to its rounding to
    binary32; a row has at most 7 entries of magnitude <= 1, each off by at most 2^-24 = 6e-8, against |c| <= 1: about
    4e-7 per coefficient, times the basis (|Y| of a few) and summed over a band: about 1e-6."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(200):
        q = _unit(rng, 1, 4)[0].astype(np.float32)
        D = _block(gs.sh_rotation_matrices(q))
        q64 = q.astype(np.float64)
        R = _rot64(q64 / np.linalg.norm(q64))
        d = _unit(rng, 200, 3)
        c = rng.uniform(-1, 1, (15, 3))
        Y, Yr = _basis(d), _basis(d @ R)        # the rows of d @ R are R^T d
        for a, b in ((0, 3), (3, 8), (8, 15)):  # per band: D is block diagonal
            assert not D[a:b, :a].any() and not D[a:b, b:].any()
            worst = max(worst, float(np.abs(Y[:, a:b] @ (D[a:b, a:b] @ c[a:b]) - Yr[:, a:b] @ c[a:b]).max()))
        worst = max(worst, float(np.abs(Y @ (D @ c) - Yr @ c).max()))
    print("defining property: max error %.3g" % worst)
    assert worst <= 1e-5


# ---- builders ----------------------------------------------------------------------------------------------------

def test_edit_builder(gs):
    e = gs.edit()
    assert isinstance(e, gs.Edit) and e.flags == 0 and list(e.reserved) == [0] * 4
    mt = gs.model_transform_pod(pos=(1, 2, 3), rot=(0, 0, 0, 1), scale=(2, 2, 2))
    e = gs.edit(transform=mt)
    assert e.flags == gs.EDIT_TRANSFORM | gs.EDIT_ROTATE_SH
    assert list(e.transform.pos) == [1, 2, 3] and list(e.transform.scale) == [2, 2, 2]
    assert gs.edit(transform=mt, rotate_sh=False).flags == gs.EDIT_TRANSFORM
    e = gs.edit(color=gs.color_override((1, 0.5, 0)), opacity=0.5)
    assert e.flags == gs.EDIT_COLOR | gs.EDIT_OPACITY
    assert list(e.color) == [0] * 9 + [1, 0.5, 0] and list(e.opacity) == [0.5, 0.0]
    assert list(gs.edit(opacity=(0.25, 0.5)).opacity) == [0.25, 0.5]
    m = np.arange(12, dtype=np.float64).reshape(3, 4)        # rows = output channels
    assert list(gs.edit(color=m).color) == list(m.T.reshape(-1))
    assert list(gs.edit(color=list(range(12))).color) == list(range(12))
    for bad in (dict(pivot=(0, 0, 0)), dict(color=np.zeros(9)), dict(opacity=(1, 2, 3)), dict(transform="x")):
        with pytest.raises((ValueError, TypeError)):
            gs.edit(**bad)
    # pivot: the pivot stays where it is, p' = s R (p - c) + c + t
    q = np.array([0.3, -0.5, 0.2, 0.7])
    q = (q / np.linalg.norm(q)).astype(np.float32)
    mt = gs.model_transform_pod(pos=(0.5, -1, 2), rot=tuple(q), scale=(1.5, 1.5, 1.5))
    c = np.array([3.0, -2.0, 0.5])
    e = gs.edit(transform=mt, pivot=c)
    R = _rot64(q) * 1.5
    assert np.allclose(R @ c + np.array(list(e.transform.pos), float), c + np.array([0.5, -1, 2]), atol=1e-5)
    assert list(e.transform.rot) == list(mt.rot) and list(e.transform.scale) == list(mt.scale)


def test_color_helpers(gs):
    def mat(c):
        assert c.dtype == np.float32 and c.shape == (12,)
        return c.reshape(4, 3).T.astype(np.float64)
    rgb = np.array([0.2, 0.5, 0.9])

    def ap(c, v=rgb):
        m = mat(c)
        return m[:, :3] @ v + m[:, 3]
    assert np.allclose(ap(gs.color_override((0.1, 0.2, 0.3))), (0.1, 0.2, 0.3)) and not mat(gs.color_override((1, 1, 1)))[:, :3].any()
    assert np.allclose(ap(gs.color_exposure(1.0)), 2 * rgb) and np.allclose(ap(gs.color_exposure(0.0)), rgb)
    assert np.allclose(ap(gs.color_contrast(2.0)), (rgb - 0.5) * 2 + 0.5) and np.allclose(ap(gs.color_contrast(1.0)), rgb)
    luma = float(np.dot([0.2126, 0.7152, 0.0722], rgb))
    assert np.allclose(ap(gs.color_saturation(0.0)), [luma] * 3, atol=1e-6) and np.allclose(ap(gs.color_saturation(1.0)), rgb)
    assert np.allclose(ap(gs.color_hue(0.0)), rgb, atol=1e-6) and np.allclose(ap(gs.color_hue(360.0)), rgb, atol=1e-6)
    assert np.allclose(ap(gs.color_hue(120.0)), rgb[[2, 0, 1]], atol=1e-6)          # r -> g -> b
    assert np.allclose(ap(gs.color_hue(77.0), np.ones(3)), np.ones(3), atol=1e-6)   # grey stays grey


def test_edit_arguments_are_checked_without_a_device(gs):
    """what the Python layer refuses before any library call; the library's own checks run in tests/test_gpu_edit.py"""
    buf = object.__new__(gs.GaussiansBuffer)
    buf._h = None
    with pytest.raises(TypeError):
        buf.edit(None, np.zeros(4, bool), gs.edit())
    with pytest.raises(TypeError):
        buf.edit(None, None, dict(flags=0))
    with pytest.raises(TypeError):
        buf.extract(None, "all")
    # a null buffer / edit is an argument error of the C ABI (no device is touched)
    lib = gs._capi.load()
    assert lib.gs_gaussians_buffer_edit(None, None, None, None) == gs.InvalidArgumentError.code
    out = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_create_from_selection(None, None, None, 0, C.byref(out), None) == gs.InvalidArgumentError.code
