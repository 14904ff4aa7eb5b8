"""gs_logf (csrc/gs_convert.h): the ln of Gaussian::to_ply / to_spz on host and device.

Against the live C library only what holds for ANY correct logf is required: the same inputs give a NaN, and the results are
at most 1 ulp apart.  Exact bits are asserted against tests/golden/logf_v1.npz, recorded on glibc 2.35 with
tests/golden/make_golden_logf.py — the C library whose algorithm gs_logf restates."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_golden_logf", os.path.join(ROOT, "tests", "golden", "make_golden_logf.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def cases(gs):
    """(input bits, gs_logf bits, libm logf bits), computed once"""
    m = _golden_module()
    x = m.inputs()
    lib = gs._capi.load()
    mine = np.zeros(len(x), dtype=np.uint32)
    arg = C.c_float()
    for k, b in enumerate(x):
        C.memmove(C.byref(arg), C.byref(C.c_uint32(int(b))), 4)      # the exact bits, signalling NaNs included
        r = C.c_float(lib.gs_logf(arg))
        C.memmove(mine[k:k + 1].ctypes.data, C.byref(r), 4)
    ref = m.libm_logf_bits(x)
    for a in (x, mine, ref):
        a.setflags(write=False)
    return x, mine, ref


def _is_nan(bits):
    return (bits & 0x7fffffff) > 0x7f800000


def _ordered(bits):
    """binary32 bits -> integers in the order of the values (+0 and -0 coincide)"""
    b = bits.astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7fffffff), b)


def test_inputs_cover_the_specials_and_the_table_boundaries(cases):
    x = set(int(v) for v in cases[0])
    for v in (0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xbf800000, 0x3f800000,
              0x00800000, 0x007fffff, 0x00800001, 0x00000001, 0x7f7fffff):
        assert v in x, hex(v)
    for i in range(16):
        for d in (-1, 0, 1):
            assert 0x3f330000 + (i << 19) + d in x
    assert len(cases[0]) > 80000


def test_gs_logf_is_within_one_ulp_of_libm_logf(cases):
    x, mine, ref = cases
    assert np.array_equal(_is_nan(mine), _is_nan(ref)), "the same inputs give a NaN"
    ok = ~_is_nan(ref)
    d = np.abs(_ordered(mine[ok]) - _ordered(ref[ok]))
    worst = int(d.max())
    print("gs_logf vs libm logf: %d of %d inputs differ, at most %d ulp" % (int((mine != ref).sum()), len(x), worst))
    assert worst <= 1, hex(int(x[ok][np.argmax(d)]))


def test_gs_logf_matches_the_bits_recorded_on_glibc_2_35(cases):
    x, mine, _ = cases
    gold = np.load(os.path.join(ROOT, "tests", "golden", "logf_v1.npz"))
    assert str(gold["libc"]) == "glibc 2.35"
    assert np.array_equal(gold["x"], x), "the golden file holds the inputs of this test"
    bad = np.flatnonzero(gold["y"] != mine)
    assert len(bad) == 0, "%d differ; first: logf(0x%08x) = 0x%08x, recorded 0x%08x" % (
        len(bad), x[bad[0]], mine[bad[0]], gold["y"][bad[0]])


def test_special_values(gs):
    assert gs.logf(1.0) == 0.0 and np.signbit(gs.logf(1.0)) == False      # noqa: E712  (+0)
    assert gs.logf(0.0) == -np.inf and gs.logf(-0.0) == -np.inf
    assert gs.logf(np.inf) == np.inf
    assert np.isnan(gs.logf(-1.0)) and np.isnan(gs.logf(-np.inf)) and np.isnan(gs.logf(np.nan))
    assert gs.logf(2.0) == float(np.float32(np.log(2.0)))
