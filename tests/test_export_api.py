"""The host side of the export path: gs_gaussian_to_ply and gs_spz_encode_decompressed — which now run
gs_convert.h's gaussian_to_ply_words / gaussian_to_spz_bytes, the functions the export kernels run — against the oracle's
Gaussian::to_ply / to_spz and against tests/golden/export_v1.npz; the declarations of the new entry points; what they check
before they need a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gs_gaussians_buffer_export_ply", "gs_gaussians_buffer_export_spz_decompressed", "gs_gaussians_buffer_export_spz",
           "gs_gaussians_buffer_write"]
INVALID_ARGUMENT = -1
N = 20000
CONFIGS = [(v, d, b) for v in (1, 2, 3) for d in (0, 1, 2, 3) for b in (8, 5, 4, 0)]


@pytest.fixture(scope="module")
def mk():
    return scenes.golden_export()


@pytest.fixture(scope="module")
def scene(gs):
    return scenes.export_scene(N)


def _is_nan(bits):
    return (bits & 0x7fffffff) > 0x7f800000


def _ordered(bits):
    b = bits.astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7fffffff), b)


def test_scene_holds_the_hostile_records(scene):
    s, q, a = scene["scale"], scene["rot"], scene["color"][:, 3]
    assert (s == 0).any() and (s == -1).any() and np.isnan(s).any() and np.isinf(s).any()
    tiny = np.finfo(np.float32).tiny
    assert ((s > 0) & (s < tiny)).any(), "a subnormal scale"
    assert (a == 0).any() and (a == 255).any()
    assert (q == 0).all(axis=1).any() and np.isnan(q).any()


def test_to_ply_matches_the_oracle_within_one_ulp(gs, ob, mk, scene):
    got = gs.gaussian_to_ply(scene).view(np.uint32).reshape(N, 62)
    want = mk.oracle_to_ply(ob, scene).view(np.uint32).reshape(N, 62)
    assert np.array_equal(_is_nan(got), _is_nan(want))
    ok = ~_is_nan(want)
    d = np.abs(_ordered(got[ok]) - _ordered(want[ok]))
    print("to_ply vs oracle: %d of %d words differ, at most %d ulp" % (int((got != want).sum()), got.size, int(d.max())))
    assert d.max() <= 1
    # everything but the three log-scales and the opacity is copied or computed without logf: bit-equal on any C library
    exact = [k for k in range(62) if k not in (54, 55, 56, 57)]
    assert np.array_equal(got[:, exact], want[:, exact])


@pytest.mark.parametrize("version", [1, 2, 3])
def test_to_spz_matches_the_oracle(gs, ob, mk, scene, version):
    for cfg in [c for c in CONFIGS if c[0] == version]:
        v, d, b = cfg
        got = np.frombuffer(gs.SpzGaussians.write_gaussians_decompressed(
            scene, gs.spz_options(version=v, sh_degree=d, sh_quantize_bits=(b, b, b))), dtype=np.uint8)
        want = mk.oracle_to_spz(ob, scene, cfg)
        assert got.size == want.size, cfg
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s: %d bytes differ, first at %d" % (cfg, len(bad), bad[0])


def test_host_encoders_match_the_golden_file(gs, mk):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "export_v1.npz"))
    g = np.ascontiguousarray(gold["gaussians"]).view(gs.GAUSSIAN_DTYPE).reshape(-1)
    assert len(g) == mk.GOLDEN_N == 300 and str(gold["libc"]) == "glibc 2.35"
    assert g.tobytes() == mk.scene(mk.GOLDEN_N).tobytes(), "the golden records are the scene of the tests"
    assert gs.gaussian_to_ply(g).tobytes() == gold["ply"].tobytes()
    for cfg in mk.GOLDEN_CONFIGS:
        v, d, b = cfg
        got = gs.SpzGaussians.write_gaussians_decompressed(g, gs.spz_options(version=v, sh_degree=d, sh_quantize_bits=(b, b, b)))
        assert got == gold["spz_v%d_d%d_b%d" % cfg].tobytes(), cfg


def test_threaded_host_encoders_give_the_same_bytes(gs, scene):
    """above 32768 records the host loops run on several threads"""
    g = np.concatenate([scene, scene])
    one = gs.gaussian_to_ply(scene).tobytes()
    assert gs.gaussian_to_ply(g).tobytes() == one + one
    opt = gs.spz_options(version=2, sh_degree=3)
    raw = np.frombuffer(gs.SpzGaussians.write_gaussians_decompressed(g, opt), dtype=np.uint8)
    assert gs.SpzGaussians(raw.tobytes()).gaussians[N:].tobytes() == gs.SpzGaussians(
        gs.SpzGaussians.write_gaussians_decompressed(scene, opt)).gaussians.tobytes()


def test_header_declares_the_export_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    for name in ENTRIES + ["gs_logf"]:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
    section = text[text.index("/* Export (DESIGN.md 3.13"):text.index("Stand-alone device primitives")]
    for name in ENTRIES:
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.13" in comment, name
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ENTRIES + ["gs_logf"]:
        assert name in rs, name


def test_null_arguments_and_internal_source_fail_without_a_device(gs):
    lib = gs._capi.load()
    n64, nsz = C.c_uint64(7), C.c_size_t(7)
    out = np.full(64, 0xAB, dtype=np.uint8)
    fake = C.c_void_p(1)      # never dereferenced: the null checks come first
    assert lib.gs_gaussians_buffer_export_ply(None, None, None, 0, None, 0, C.byref(n64)) == INVALID_ARGUMENT
    assert lib.gs_gaussians_buffer_export_ply(fake, None, None, 0, None, 0, None) == INVALID_ARGUMENT
    for fn in (lib.gs_gaussians_buffer_export_spz_decompressed, lib.gs_gaussians_buffer_export_spz):
        assert fn(None, None, None, 0, None, out.ctypes.data, out.size, C.byref(nsz)) == INVALID_ARGUMENT
        assert fn(fake, None, None, 0, None, out.ctypes.data, out.size, None) == INVALID_ARGUMENT
    for source in (0, 1, 2):
        assert lib.gs_gaussians_buffer_write(None, None, None, 0, source, out.ctypes.data, out.size, C.byref(nsz)) == INVALID_ARGUMENT
        assert lib.gs_gaussians_buffer_write(fake, None, None, 0, source, out.ctypes.data, out.size, None) == INVALID_ARGUMENT
    assert (out == 0xAB).all()
    # GS_SOURCE_INTERNAL (and an unknown source) with nothing null: refused before the buffer is looked at, as gs_gaussians_write does
    info = gs._capi.ErrorInfo()
    for source in (0, 7):
        nsz.value = 7
        assert lib.gs_gaussians_buffer_write(fake, None, None, 0, source, out.ctypes.data, out.size, C.byref(nsz)) == INVALID_ARGUMENT
        lib.gs_last_error(C.byref(info))
        assert info.message == b"cannot write Internal Gaussians to buffer" and info.a == source
        assert nsz.value == 0 and (out == 0xAB).all()
    g1 = np.zeros(1, dtype=gs.GAUSSIAN_DTYPE)
    assert lib.gs_gaussians_write(g1.ctypes.data, 1, 0, out.ctypes.data, out.size, C.byref(nsz)) == INVALID_ARGUMENT
    lib.gs_last_error(C.byref(info))
    assert info.message == b"cannot write Internal Gaussians to buffer"
    with pytest.raises(gs.InvalidArgumentError):
        gs._check(lib.gs_gaussians_buffer_export_ply(None, None, None, 0, None, 0, C.byref(n64)))


def test_python_type_errors(gs):
    buf = gs.GaussiansBuffer(None, gs.GaussianPod(0, 0), None)
    for call in (lambda: buf.export_ply(None, selection=np.ones(4, bool)),
                 lambda: buf.export_spz(None, selection="all"),
                 lambda: buf.export_spz(None, options={"version": 3}),
                 lambda: buf.write(None, gs.GaussiansSource.Ply, selection=[1, 2]),
                 lambda: buf.write(None, 1),
                 lambda: buf.write(None, "ply")):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError, match="cannot write Internal Gaussians to buffer"):
        buf.write(None, gs.GaussiansSource.Internal)
