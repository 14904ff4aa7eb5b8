"""Layout conversion, the parts that need no device: the header declares the entry points, the ctypes layer
binds them, the Rust file and the C++ mirror name them, the pair table has its 112 pairs, and the host conversion
gs_convert_pods — the per-record function the device kernel calls — equals the numpy restatement of tests/convert_np.py and
gs_pack(dst, gs_unpack_to_gaussian(src)) byte for byte, keeps a section whose config is kept verbatim, and composes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import convert_np
import edit_np
from records import diff
from scenes import ALL_LAYOUTS, hostile_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TITLE = "Layout conversion"
ENTRIES = ["gs_layout_convertible", "gs_convert_pods", "gs_gaussians_buffer_create_converted", "gs_gaussians_buffer_create_concat_as"]
PAIRS = [(a, b) for a in ALL_LAYOUTS for b in ALL_LAYOUTS]
VALID = [(a, b) for a, b in PAIRS if convert_np.convertible(*a, *b)]
f32 = np.float32
N = 257


@pytest.fixture(scope="module")
def packed(gs):
    """{(sh, cov): the N records of the scene packed by gs_pack}, computed once and left unchanged"""
    g = hostile_scene(N)
    out = {}
    for sh, cov in ALL_LAYOUTS:
        out[(sh, cov)] = gs.GaussianPod(sh, cov).from_gaussian(g)
        out[(sh, cov)].setflags(write=False)
    return out, g


# ---- header and bindings ---------------------------------------------------------------------------------------------

def test_header_declares_the_conversion_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    assert text.count(TITLE) == 1
    assert text.index("Neighbour counts and select by neighbourhood") < text.index("gs_select_neighbors(") < text.index(TITLE) \
        < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    for name in ENTRIES:
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
        assert getattr(lib, name).restype == gs._capi.SIGNATURES[name][0]
        assert len(re.findall(r"\b%s\s*\(" % name, text)) == 1, name
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.12" in comment, name
    assert re.search(r"#define\s+GS3D_ABI_VERSION\s+1\b", text) and lib.gs_abi_version() == 1
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for word in ("gs_gaussians_buffer_create_converted", "gs_gaussians_buffer_create_concat_as", "LossyConfigError"):
        assert word in hpp, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**3.12 " in design


def test_rust_bindings_name_the_conversion_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn %s\(" % name, rs), name


def test_python_layer_checks_arguments_without_a_device(gs):
    """what the Python layer refuses before any library call, on handle-less stand-ins"""
    buf = object.__new__(gs.GaussiansBuffer)
    buf._h = None
    pod = gs.GaussianPod(1, 2)
    with pytest.raises(TypeError):
        buf.convert(None, (1, 2))
    with pytest.raises(TypeError):
        buf.convert(None, pod, selection=np.zeros(4, bool))
    with pytest.raises(TypeError):
        gs.GaussiansBuffer.concat(None, [buf], pod="f16")
    with pytest.raises(TypeError):
        gs.GaussiansBuffer.concat(None, [object()], pod=pod)
    with pytest.raises(ValueError):
        gs.GaussiansBuffer.concat(None, [buf], selections=[None, None], pod=pod)
    with pytest.raises(TypeError):
        pod.convertible_to((0, 0))
    with pytest.raises(TypeError):
        pod.convert(np.zeros(pod.size, np.uint8), "f32")
    with pytest.raises(ValueError):
        pod.convert(np.zeros(pod.size + 1, np.uint8), gs.GaussianPod(0, 1))
    assert pod.convert(np.zeros(0, np.uint8), gs.GaussianPod(0, 1)).size == 0


def test_null_arguments_are_c_abi_errors(gs):
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    out = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_create_converted(None, None, None, 0, 1, 2, C.byref(out), None) == bad
    assert out.value is None
    assert lib.gs_gaussians_buffer_create_converted(None, None, None, 0, 1, 2, None, None) == bad
    for count in (0, 65):
        out = C.c_void_p(1)
        srcs = (C.c_void_p * 65)()
        assert lib.gs_gaussians_buffer_create_concat_as(None, srcs, None, count, 1, 2, C.byref(out), None) == bad
        assert out.value is None
    out = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_create_concat_as(None, None, None, 1, 1, 2, C.byref(out), None) == bad and out.value is None
    srcs = (C.c_void_p * 1)()
    assert lib.gs_gaussians_buffer_create_concat_as(None, srcs, None, 1, 1, 2, C.byref(out), None) == bad      # source 0 is null
    assert lib.gs_gaussians_buffer_create_concat_as(None, srcs, None, 1, 4, 0, C.byref(out), None) == bad      # unknown config
    buf = np.full(256, 0xAB, np.uint8)
    src = np.zeros(256, np.uint8)
    assert lib.gs_convert_pods(0, 0, 1, 2, None, 1, buf.ctypes.data_as(C.c_void_p)) == bad
    assert lib.gs_convert_pods(0, 0, 1, 2, src.ctypes.data_as(C.c_void_p), 1, None) == bad
    for cfg in ((4, 0, 1, 2), (0, 3, 1, 2), (0, 0, -1, 2), (0, 0, 1, 3)):
        assert lib.gs_convert_pods(*cfg, src.ctypes.data_as(C.c_void_p), 1, buf.ctypes.data_as(C.c_void_p)) == bad, cfg
        assert lib.gs_layout_convertible(*cfg) == 0, cfg
    assert (buf == 0xAB).all()


# ---- the pair table --------------------------------------------------------------------------------------------------

def test_pair_table(gs):
    lib = gs._capi.load()
    assert len(VALID) == 112 and len(PAIRS) == 144
    src = np.zeros(224, np.uint8)
    for a, b in PAIRS:
        ok = (a, b) in VALID
        # §3.12: the SH pair never matters; the cov pair must not go back to rot-scale
        assert ok == (b[1] != 0 or a[1] == 0)
        assert lib.gs_layout_convertible(*a, *b) == int(ok), (a, b)
        assert gs.GaussianPod(*a).convertible_to(gs.GaussianPod(*b)) == ok
        out = np.full(224, 0xAB, np.uint8)
        rc = lib.gs_convert_pods(*a, *b, src.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))
        if ok:
            assert rc == 0, (a, b)
        else:
            assert rc == gs.LossyConfigError.code, (a, b)
            assert (out == 0xAB).all(), (a, b)
            with pytest.raises(gs.LossyConfigError):
                gs.GaussianPod(*a).convert(src[:gs.GaussianPod(*a).size], gs.GaussianPod(*b))


# ---- bytes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src", ALL_LAYOUTS)
def test_bytes_equal_the_restatement(gs, packed, src):
    pods, _ = packed
    spod = gs.GaussianPod(*src)
    done = 0
    for dst in ALL_LAYOUTS:
        if (src, dst) not in VALID:
            continue
        dpod = gs.GaussianPod(*dst)
        got = spod.convert(pods[src], dpod)
        assert got.size == N * dpod.size == N * edit_np.pod_bytes(*dst)
        want = convert_np.convert(*src, *dst, pods[src])
        assert np.array_equal(got, want), (src, dst, diff(got, want, dpod.size))
        done += 1
    assert done == (12 if src[1] == 0 else 8)


@pytest.mark.parametrize("src", [(0, 0), (1, 0), (2, 0)])
def test_bytes_equal_unpack_then_pack(gs, packed, src):
    """the three sources that gs_unpack_to_gaussian accepts: convert == gs_pack(dst, gs_unpack_to_gaussian(src))"""
    pods, _ = packed
    spod = gs.GaussianPod(*src)
    g = spod.into_gaussian(pods[src])
    for dst in ALL_LAYOUTS:
        dpod = gs.GaussianPod(*dst)
        got, want = spod.convert(pods[src], dpod), dpod.from_gaussian(g)
        assert np.array_equal(got, want), (src, dst, diff(got, want, dpod.size))
        if src == (0, 0):       # the f32 / rot-scale layout holds the Gaussians themselves
            assert np.array_equal(got, pods[dst]), (src, dst)


# ---- the verbatim rule -----------------------------------------------------------------------------------------------

def _raw_records(sh, cov, n=8):
    """records of random bytes with what a decode / encode round trip would change: an snorm8 byte 0x80, a signalling f16
    NaN 0x7d01, nonzero pad bytes in the SH section, nonzero trailing pad words.  The cov section holds plain values."""
    rng = np.random.default_rng(5)
    nb = edit_np.pod_bytes(sh, cov)
    r = rng.integers(0, 256, (n, nb), dtype=np.uint8)
    sh0, cov0 = 16, 16 + edit_np.SH_BYTES[sh]
    if sh == 1:
        h = np.ascontiguousarray(r[:, sh0:sh0 + 92]).view(np.uint16)
        h[:, :45] = rng.uniform(-2, 2, (n, 45)).astype(np.float16).view(np.uint16)
        h[:, 7] = 0x7D01
        h[:, 45] = 0xBEEF                                        # the pad half-word
        r[:, sh0:sh0 + 92] = h.view(np.uint8)
    if sh == 2:
        r[:, sh0 + 11] = 0x80
        r[:, sh0 + 45:sh0 + 48] = (0x11, 0x22, 0x33)             # the pad bytes
    if sh == 0:
        r[:, sh0:sh0 + 180] = rng.uniform(-2, 2, (n, 45)).astype(f32).view(np.uint8)
    c = rng.uniform(-2, 2, (n, 7)).astype(f32)
    if cov == 2:
        r[:, cov0:cov0 + 12] = c[:, :6].astype(np.float16).view(np.uint8)
    else:
        r[:, cov0:cov0 + edit_np.COV_BYTES[cov]] = c[:, :edit_np.COV_BYTES[cov] // 4].view(np.uint8)
    pad = nb - (cov0 + edit_np.COV_BYTES[cov])
    if pad:
        r[:, nb - pad:] = 0xCD
    return r, pad


def test_a_kept_section_is_copied_verbatim(gs):
    for sh in range(4):
        for scov, dcov in ((0, 1), (0, 2), (1, 2), (2, 1)):
            src, spad = _raw_records(sh, scov)
            if sh == 1:
                assert spad >= 8     # the f16 layouts have two or three trailing pad words, nonzero here
            got = gs.GaussianPod(sh, scov).convert(src.reshape(-1), gs.GaussianPod(sh, dcov)).reshape(len(src), -1)
            nsh = edit_np.SH_BYTES[sh]
            assert np.array_equal(got[:, :16 + nsh], src[:, :16 + nsh]), (sh, scov, dcov)       # SH words kept, pad included
            dpad = got.shape[1] - (16 + nsh + edit_np.COV_BYTES[dcov])
            assert dpad >= 0 and not got[:, got.shape[1] - dpad:].any(), (sh, scov, dcov)       # the trailing pad is zero
            assert np.array_equal(got.reshape(-1), convert_np.convert(sh, scov, sh, dcov, src.reshape(-1)))
    # a decode / encode round trip would NOT keep these: the rule is not cosmetic
    src, _ = _raw_records(2, 0)
    back = gs.GaussianPod(0, 0).convert(gs.GaussianPod(2, 0).convert(src.reshape(-1), gs.GaussianPod(0, 0)), gs.GaussianPod(2, 0))
    assert back.reshape(len(src), -1)[0, 16 + 11] == 0x81
    src, _ = _raw_records(1, 0)
    back = gs.GaussianPod(0, 0).convert(gs.GaussianPod(1, 0).convert(src.reshape(-1), gs.GaussianPod(0, 0)), gs.GaussianPod(1, 0))
    assert back.reshape(len(src), -1)[:, 16:108].view(np.uint16)[0, 7] == 0x7F01
    # identical layouts keep every byte
    for sh, cov in ALL_LAYOUTS:
        src, _ = _raw_records(sh, cov)
        pod = gs.GaussianPod(sh, cov)
        assert np.array_equal(pod.convert(src.reshape(-1), pod), src.reshape(-1)), (sh, cov)
    # a kept cov section is copied verbatim too
    for cov in range(3):
        src, _ = _raw_records(0, cov)
        got = gs.GaussianPod(0, cov).convert(src.reshape(-1), gs.GaussianPod(3, cov)).reshape(len(src), -1)
        nc = edit_np.COV_BYTES[cov]
        assert np.array_equal(got[:, 16:16 + nc], src[:, 196:196 + nc]) and not got[:, 16 + nc:].any()


# ---- chains ----------------------------------------------------------------------------------------------------------

def test_chains(gs, packed):
    pods, _ = packed
    P = gs.GaussianPod
    for sh in range(4):
        p = pods[(sh, 0)]
        # rot-scale -> f32 -> f16 equals rot-scale -> f16
        assert np.array_equal(P(sh, 1).convert(P(sh, 0).convert(p, P(sh, 1)), P(sh, 2)), P(sh, 0).convert(p, P(sh, 2))), sh
        # f16 -> f32 -> f16 is the identity on the cov words (on every byte: the SH section is kept)
        h = pods[(sh, 2)]
        assert np.array_equal(P(sh, 1).convert(P(sh, 2).convert(h, P(sh, 1)), P(sh, 2)), h), sh
    # SH f16 -> f32 -> f16: the identity on coefficients that are not signalling NaNs (gs_pack produces none)
    for cov in range(3):
        h = pods[(1, cov)]
        assert np.array_equal(P(0, cov).convert(P(1, cov).convert(h, P(0, cov)), P(1, cov)), h), cov
    raw, _ = _raw_records(1, 1)
    back = P(0, 1).convert(P(1, 1).convert(raw.reshape(-1), P(0, 1)), P(1, 1)).reshape(len(raw), -1)
    a, b = raw[:, 16:106].view(np.uint16), back[:, 16:106].view(np.uint16)
    snan = ((a & 0x7C00) == 0x7C00) & ((a & 0x03FF) != 0) & ((a & 0x0200) == 0)
    assert snan[:, 7].all() and np.array_equal(a[~snan], b[~snan]) and (b[snan] == (a[snan] | 0x0200)).all()
    # SH none -> X: an all-zero SH section
    for dsh in range(3):
        for cov in range(3):
            got = P(3, cov).convert(pods[(3, cov)], P(dsh, cov)).reshape(N, -1)
            assert not got[:, 16:16 + edit_np.SH_BYTES[dsh]].any(), (dsh, cov)
            assert np.array_equal(got[:, :16], pods[(3, cov)].reshape(N, -1)[:, :16])
