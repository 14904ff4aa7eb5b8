"""Image metrics, the parts that need no device: the header declares gs_image_compare with its notes in
the stated place, the ctypes layer binds it with structs of the header's layout, the Rust file and the C++ mirror name it,
every argument check comes before the device is touched, and the numpy model of tests/metrics_np.py has the tabulated
weights, gives exactly 1 for identical images and stays within its bounds of a float64 witness."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import metrics_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TITLE = "Image metrics (DESIGN.md 3.14; no reference item)"
f32 = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "gs3d.h")).read()


def test_header_declares_the_metrics_api(gs):
    text = _header()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    assert re.search(r"\bgs_image_compare\s*\(", text)
    assert "gs_image_compare" in gs._capi.SIGNATURES
    assert lib.gs_image_compare.argtypes == gs._capi.SIGNATURES["gs_image_compare"][1]
    assert lib.gs_image_compare.restype == gs._capi.SIGNATURES["gs_image_compare"][0] == C.c_int32
    assert gs._capi.SIGNATURES["gs_image_compare"][1][4:6] == [C.c_uint32, C.c_uint32]
    assert text.count(TITLE) == 1
    assert text.index("Contribution scores") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    for key in ("gs_image_compare(", "gs_image_compare_desc {", "gs_image_metrics {", "GS_COMPARE_SSIM = 1"):
        comment = section[:section.index(key)].rsplit("/*", 1)[1] if key != "GS_COMPARE_SSIM = 1" else section[:section.index(key)]
        assert "no reference item" in comment and "DESIGN.md 3.14" in comment, key
    assert gs.COMPARE_SSIM == 1
    for h in metrics_np.WEIGHT_HEX:
        assert h in open(os.path.join(ROOT, "wgpu-3dgs-core_amd", "csrc", "gs_metrics_kernels.h")).read(), h


def test_rust_and_cpp_name_the_metrics_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ("pub fn gs_image_compare(", "pub struct gs_image_compare_desc", "pub struct gs_image_metrics", "pub const GS_COMPARE_SSIM: u32 = 1;",
                 "pub err_plane: *mut f32,", "pub max_abs_at: [u32; 4],", "pub ssim_finite: [u64; 3],"):
        assert name in rs, name
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ("gs_image_metrics image_compare(", "gs_image_compare(", "image_psnr(", "image_ssim("):
        assert name in hpp, name


def test_structs_match_the_header(gs, tmp_path):
    d, m = gs._capi.ImageCompareDesc, gs._capi.ImageMetricsRecord
    assert [f[0] for f in d._fields_] == ["flags", "data_range", "err_plane", "ssim_plane", "reserved"]
    assert (d.flags.offset, d.data_range.offset, d.err_plane.offset, d.ssim_plane.offset, d.reserved.offset, C.sizeof(d)) == (0, 4, 8, 16, 24, 40)
    names = ["pixels", "finite", "differing", "bit_differing", "sum_sq", "sum_abs", "max_abs", "max_abs_at", "ssim_sum", "ssim_finite"]
    assert [f[0] for f in m._fields_] == names
    assert [getattr(m, n).offset for n in names] + [C.sizeof(m)] == [0, 8, 16, 24, 32, 64, 96, 112, 128, 152, 176]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gs3d.h"\nint main(void) { printf("'
                   + "%zu " * (6 + 11) + '%d\\n", '
                   + ", ".join("offsetof(gs_image_compare_desc, %s)" % n for n in ("flags", "data_range", "err_plane", "ssim_plane", "reserved"))
                   + ", sizeof(gs_image_compare_desc), " + ", ".join("offsetof(gs_image_metrics, %s)" % n for n in names)
                   + ", sizeof(gs_image_metrics), (int)GS_COMPARE_SSIM); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [0, 4, 8, 16, 24, 40] + [getattr(m, n).offset for n in names] + [176, 1]


def test_every_argument_check_comes_before_the_device(gs):
    """a NULL device is refused last in effect: each of the other faults is reported with it, none of them touches a device"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    out = gs._capi.ImageMetricsRecord()
    out.pixels = 77
    img, plane = C.c_void_p(0x10000), 0x20000      # never dereferenced

    def desc(flags=0, data_range=1.0, err=None, ssim=None, reserved=(0, 0, 0, 0)):
        d = gs._capi.ImageCompareDesc()
        d.flags, d.data_range, d.err_plane, d.ssim_plane = flags, data_range, err, ssim
        d.reserved[:] = reserved
        return C.byref(d)

    def call(dev=None, a=img, b=img, w=8, h=8, d=None, o=C.byref(out)):
        return lib.gs_image_compare(dev, None, a, b, w, h, d, o)

    assert call() == bad                                       # a null device, everything else valid
    assert call(a=None) == bad and call(b=None) == bad and call(o=None) == bad
    assert call(w=0) == bad and call(h=0) == bad
    assert call(w=0xFFFFFFFF, h=1) == bad and call(w=65536, h=65536) == bad and call(w=0x80000000, h=2) == bad
    assert call(a=C.c_void_p(0x10008)) == bad and call(b=C.c_void_p(0x10004)) == bad
    assert call(d=desc(err=plane + 2)) == bad and call(d=desc(flags=1, ssim=plane + 1)) == bad
    assert call(d=desc(flags=2)) == bad and call(d=desc(flags=0x80000001)) == bad
    for k in range(4):
        assert call(d=desc(reserved=tuple(int(j == k) for j in range(4)))) == bad
    for L in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(d=desc(data_range=L)) == bad, L
    assert call(d=desc(ssim=plane)) == bad                     # ssim_plane without the flag
    assert out.pixels == 77
    # ... and each message names its own fault, so the check ran before the device was looked at
    info = gs._capi.ErrorInfo()
    for kwargs, word in ((dict(w=0), "0 x 8"), (dict(w=65536, h=65536), "2^32 - 2"), (dict(a=C.c_void_p(0x10008)), "16-byte"),
                         (dict(d=desc(err=plane + 2)), "4-byte"), (dict(d=desc(flags=2)), "flags"), (dict(d=desc(reserved=(0, 0, 1, 0))), "reserved"),
                         (dict(d=desc(data_range=0.0)), "data_range"), (dict(d=desc(ssim=plane)), "GS_COMPARE_SSIM")):
        dev = C.c_void_p(0x30000)      # a non-null device that is never dereferenced: the call fails before it
        assert call(dev=dev, **kwargs) == bad
        lib.gs_last_error(C.byref(info))
        assert word in info.message.decode(), (word, info.message)


def test_python_layer_checks_its_arguments(gs):
    dev = object.__new__(gs.Device)
    dev._h = None
    with pytest.raises(TypeError):
        gs.image_compare(None, None, 16, 16, 4, 4)
    with pytest.raises(TypeError):
        gs.image_compare(dev, "stream", 16, 16, 4, 4)
    with pytest.raises(TypeError):
        gs.image_compare(dev, None, np.zeros(4), 16, 4, 4)
    with pytest.raises(TypeError):
        gs.image_compare(dev, None, 16, 16, 4.0, 4)
    for w, h in ((0, 4), (4, 0), (65536, 65536), (-1, 4)):
        with pytest.raises(ValueError):
            gs.image_compare(dev, None, 16, 16, w, h)
    for L in (0, -2.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError):
            gs.image_compare(dev, None, 16, 16, 4, 4, data_range=L)
    with pytest.raises(ValueError):
        gs.image_compare(dev, None, 16, 16, 4, 4, ssim_plane_ptr=32)
    m = gs.ImageMetrics(pixels=4, finite=4, differing=1, bit_differing=1, sum_sq=np.array([3.0, 0.0, 0.0, 1.0]), sum_abs=np.zeros(4),
                        max_abs=np.zeros(4, f32), max_abs_at=np.zeros(4, np.uint32), ssim_sum=np.array([4.0, 2.0, 3.0]),
                        ssim_finite=np.array([4, 4, 4], np.uint64))
    assert list(m.mse) == [0.75, 0.0, 0.0, 0.25] and m.mse_rgb == 0.25 and not m.identical
    assert m.psnr() == pytest.approx(10 * np.log10(4.0)) and m.psnr(255) == pytest.approx(10 * np.log10(255.0 ** 2 * 4))
    assert m.ssim == 0.75 and list(m.ssim_channels) == [1.0, 0.5, 0.75]
    same = gs.ImageMetrics(pixels=4, finite=4, differing=0, bit_differing=0, sum_sq=np.zeros(4), sum_abs=np.zeros(4), max_abs=np.zeros(4, f32),
                           max_abs_at=np.zeros(4, np.uint32), ssim_sum=np.zeros(3), ssim_finite=np.zeros(3, np.uint64))
    assert same.identical and same.psnr() == float("inf")


# ---- the model -----------------------------------------------------------------------------------------------------------

def test_model_weights_have_the_tabulated_bits():
    g = metrics_np.weights()
    assert g.dtype == f32 and len(g) == 11
    assert [float(v).hex() for v in g] == [float.fromhex(h).hex() for h in metrics_np.WEIGHT_HEX]
    assert np.array_equal(g, g[::-1]) and abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-7
    text = _header() + open(os.path.join(ROOT, "DESIGN.md")).read()
    for h in metrics_np.WEIGHT_HEX:
        assert h in text, h


@pytest.mark.parametrize("h,w", metrics_np.SIZES)
def test_model_gives_exactly_one_for_identical_images(h, w):
    for kind in metrics_np.PAIRS:
        a, _ = metrics_np.image_pair(kind, h, w)
        r = metrics_np.compare(a, a.copy(), ssim=True)
        assert (r["ssim_map"].view(np.uint32) == 0x3F800000).all(), kind
        assert (r["ssim_plane"].view(np.uint32) == 0x3F800000).all(), kind
        assert list(r["ssim_sum"]) == [h * w] * 3 and list(r["ssim_finite"]) == [h * w] * 3
        assert r["differing"] == 0 and r["bit_differing"] == 0 and not r["sum_sq"].any() and not r["err_plane"].any()
        assert list(r["max_abs_at"]) == [0] * 4


def test_model_against_the_float64_witness():
    worst_pixel = worst_mean = 0.0
    for h, w, kind, a, b in metrics_np.image_set():
        s = metrics_np.ssim_map(a, b).astype(np.float64)
        t = metrics_np.ssim_witness(a, b)
        assert np.isfinite(s).all() and np.isfinite(t).all(), (h, w, kind)
        dp = float(np.abs(s - t).max())
        dm = float(np.abs(s.mean(axis=(0, 1)) - t.mean(axis=(0, 1))).max())
        print("%3d x %3d %-14s per pixel %.3e  mean %.3e" % (h, w, kind, dp, dm))
        worst_pixel, worst_mean = max(worst_pixel, dp), max(worst_mean, dm)
    print("worst per pixel %.4g  worst mean %.4g" % (worst_pixel, worst_mean))
    assert worst_pixel <= metrics_np.PIXEL_BOUND and worst_mean <= metrics_np.MEAN_BOUND
    # the recorded values are the ones this model shows
    assert worst_pixel == pytest.approx(metrics_np.MEASURED_PIXEL_DEV, rel=0.05)
    assert worst_mean == pytest.approx(metrics_np.MEASURED_MEAN_DEV, rel=0.05)


def test_model_error_fields_on_a_hand_made_pair():
    a = np.zeros((2, 3, 4), f32)
    b = np.zeros((2, 3, 4), f32)
    a[0, 1] = (1.0, 2.0, 3.0, 4.0)
    b[0, 1] = (0.5, 2.0, 5.0, 4.0)
    a[1, 0, 2] = -2.0             # the same |d_b| later: the smaller index wins
    a[1, 2, 0] = np.nan           # not finite: out of everything but bit_differing
    a[0, 0, 3] = -0.0             # bits differ, values do not
    r = metrics_np.compare(a, b)
    assert (r["pixels"], r["finite"], r["differing"], r["bit_differing"]) == (6, 5, 2, 4)
    assert list(r["sum_sq"]) == [0.25, 0.0, 8.0, 0.0] and list(r["sum_abs"]) == [0.5, 0.0, 4.0, 0.0]
    assert list(r["max_abs"]) == [0.5, 0.0, 2.0, 0.0] and list(r["max_abs_at"]) == [1, 0, 1, 0]
    e = r["err_plane"]
    assert e[0, 1] == 2.0 and e[1, 0] == 2.0 and e[0, 0] == 0.0 and e.view(np.uint32)[1, 2] == 0x7FC00000
    none = metrics_np.compare(np.full((1, 1, 4), np.inf, f32), np.zeros((1, 1, 4), f32))
    assert none["finite"] == 0 and list(none["max_abs"]) == [0.0] * 4 and list(none["max_abs_at"]) == [0xFFFFFFFF] * 4
