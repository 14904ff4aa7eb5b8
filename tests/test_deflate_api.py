"""The Huffman-only gzip member, the parts that need no device: the host encoder gs_gzip_fast is byte-equal
to the Python restatement tests/deflate_np.py, every inflater returns the input, the size bound holds, the member of a
synthetic scene's payload stays under the cap, the bytes do not depend on the thread count, and the header, the ctypes
layer, the Rust file and the C++ mirror declare the API."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TITLE = "Fast gzip members (DESIGN.md 3.15; no reference item)"
NAMES = [name for name, _ in deflate_np.inputs()]
API = ("gs_gzip_fast_bound", "gs_gzip_fast", "gs_buffer_gzip_fast", "gs_gaussians_buffer_export_spz_fast")


@pytest.fixture(scope="module")
def members(gs):
    """{name: (input, the host encoder's member)}: encoded once"""
    return {name: (data, gs.gzip_fast(data)) for name, data in deflate_np.inputs()}


@pytest.mark.parametrize("name", NAMES)
def test_host_bytes_equal_the_model(members, name):
    data, z = members[name]
    info = []
    want = deflate_np.member(data, info)
    if z != want:
        a, b = np.frombuffer(z, np.uint8), np.frombuffer(want, np.uint8)
        m = min(len(a), len(b))
        bad = np.flatnonzero(a[:m] != b[:m])
        pytest.fail("%s: %d bytes, want %d; first difference at byte %s" % (name, len(z), len(want), bad[0] if len(bad) else m))
    forms = [f for f, _ in info]
    if name == "constant":
        assert forms == ["run"]
    elif name == "constant_plus_one":
        assert forms == ["run", "stored"]
    elif name == "uniform":
        assert forms == ["stored"] * 3
    elif name == "three_forms":
        assert forms == ["run", "dynamic", "stored"]
    elif name == "fibonacci":
        assert forms[0] == "dynamic" and info[0][1] > 15, info      # the unlimited tree is deeper than the limit
    elif name == "two_values":
        assert forms == ["dynamic"]


@pytest.mark.parametrize("name", NAMES)
def test_every_inflater_returns_the_input(gs, members, name):
    data, z = members[name]
    assert gzip.decompress(z) == data
    d = zlib.decompressobj(31)
    assert d.decompress(z) + d.flush() == data
    assert d.eof and d.unused_data == b""
    lib = gs._capi.load()
    buf = np.frombuffer(z, np.uint8)
    n = C.c_size_t()
    assert lib.gs_spz_decompress(buf.ctypes.data, buf.size, None, 0, C.byref(n)) == 0 and n.value == len(data)
    out = np.zeros(max(n.value, 1), np.uint8)
    assert lib.gs_spz_decompress(buf.ctypes.data, buf.size, out.ctypes.data, n.value, C.byref(n)) == 0
    assert out[:n.value].tobytes() == data


@pytest.mark.parametrize("name", NAMES)
def test_size_bound(gs, members, name):
    data, z = members[name]
    chunks = (len(data) + 32767) // 32768
    assert len(z) <= 18 + len(data) + 5 * max(1, chunks)
    assert gs.gzip_fast_bound(len(data)) == 18 + len(data) + 5 * max(1, chunks) == deflate_np.bound(len(data))


def test_empty_input_is_the_empty_fixed_block(gs):
    z = gs.gzip_fast(b"")
    assert z == deflate_np.HEADER + b"\x03\x00" + bytes(8) and len(z) == 20


def test_size_query_and_short_capacity(gs):
    lib = gs._capi.load()
    data = np.frombuffer(deflate_np.inputs()[8][1], np.uint8)      # one whole chunk
    n = C.c_size_t()
    assert lib.gs_gzip_fast(data.ctypes.data, data.size, None, 0, C.byref(n)) == 0
    size = n.value
    assert size == len(deflate_np.member(data.tobytes()))
    out = np.full(size, 0xee, np.uint8)
    n.value = 0
    assert lib.gs_gzip_fast(data.ctypes.data, data.size, out.ctypes.data, size - 1, C.byref(n)) == gs.InvalidArgumentError.code
    assert n.value == size and (out == 0xee).all()
    assert lib.gs_gzip_fast(None, 5, out.ctypes.data, size, C.byref(n)) == gs.InvalidArgumentError.code
    assert lib.gs_gzip_fast(data.ctypes.data, data.size, out.ctypes.data, size, None) == gs.InvalidArgumentError.code
    assert (out == 0xee).all()
    assert lib.gs_gzip_fast(data.ctypes.data, data.size, out.ctypes.data, size, C.byref(n)) == 0 and out.tobytes() == deflate_np.member(data.tobytes())


def test_compression_cap_on_a_synthetic_scene(gs):
    """The member of synth.scene(20000)'s default payload is below 0.90 of the payload: a cap, not a target (the prototype of
    the format gave 0.7908, the order-0 entropy bound leaves it a tenth of headroom)."""
    import synth
    payload = gs.SpzGaussians.write_gaussians_decompressed(synth.scene(20000))
    assert len(payload) == 16 + 65 * 20000
    z = gs.gzip_fast(payload)
    ratio = len(z) / len(payload)
    print("member %d B of %d B payload: %.4f; zlib level 6: %d B" % (len(z), len(payload), ratio, len(zlib.compress(payload, 6))))
    assert gzip.decompress(z) == payload
    assert ratio < 0.90, ratio


def test_thread_counts_give_equal_bytes(gs, monkeypatch):
    """1 and 16 host threads: the same bytes (GS3D_HOST_THREADS is read by the library each time it encodes)"""
    data = b"".join(d for _, d in deflate_np.inputs()) * 3      # 60 chunks of every form
    assert len(data) > 40 * 32768
    out = []
    for threads in ("1", "16"):
        monkeypatch.setenv("GS3D_HOST_THREADS", threads)
        out.append(gs.gzip_fast(data))
    assert out[0] == out[1] and gzip.decompress(out[0]) == data


def test_header_declares_the_deflate_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    assert text.count(TITLE) == 1
    assert text.index("Image metrics (DESIGN.md 3.14") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    for name in API:
        assert re.search(r"\b%s\s*\(" % name, section), name
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.15" in comment, name
        assert name in gs._capi.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == gs._capi.SIGNATURES[name][1] and fn.restype == gs._capi.SIGNATURES[name][0]
    sz, vp, i32 = C.c_size_t, C.c_void_p, C.c_int32
    assert gs._capi.SIGNATURES["gs_gzip_fast_bound"] == (sz, [sz])
    assert gs._capi.SIGNATURES["gs_buffer_gzip_fast"] == (i32, [vp, vp, sz, sz, vp, sz, vp])
    assert gs._capi.SIGNATURES["gs_gaussians_buffer_export_spz_fast"] == gs._capi.SIGNATURES["gs_gaussians_buffer_export_spz"]


def test_rust_and_cpp_name_the_deflate_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ("pub fn gs_gzip_fast_bound(len: usize) -> usize;", "pub fn gs_gzip_fast(", "pub fn gs_buffer_gzip_fast(b: *mut gs_buffer, s: *mut gs_stream, offset: usize, len: usize,",
                 "pub fn gs_gaussians_buffer_export_spz_fast("):
        assert name in rs, name
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ("std::vector<uint8_t> gzip_fast(const void *bytes, size_t len)", "gzip_fast(Stream &s, size_t offset, size_t len) const",
                 "export_spz_fast(Stream &s, const Selection *sel", "gs_gzip_fast_bound(", "gs_buffer_gzip_fast", "gs_gaussians_buffer_export_spz_fast"):
        assert name in hpp, name


def test_device_calls_check_their_arguments_first(gs):
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    n = C.c_size_t(77)
    out = np.full(64, 0xee, np.uint8)
    assert lib.gs_buffer_gzip_fast(None, None, 0, 0, out.ctypes.data, 64, C.byref(n)) == bad
    assert lib.gs_gaussians_buffer_export_spz_fast(None, None, None, 0, None, out.ctypes.data, 64, C.byref(n)) == bad
    assert (out == 0xee).all()
    with pytest.raises(TypeError):
        gs.GaussiansBuffer.export_spz_file(object.__new__(gs.GaussiansBuffer), None, options="v3")
    with pytest.raises(TypeError):
        gs.GaussiansBuffer.export_spz_file(object.__new__(gs.GaussiansBuffer), None, selection=5)
