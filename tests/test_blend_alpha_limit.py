"""k_blend_np_limit (csrc/gs_render_kernels.h): the Splat-mode blend decides "alpha >= 1/255" with one unsigned compare of
bits(-power) against the table's word of the splat's opacity byte k, bits(L(k)) + 1.  The table comes from
tools/blend_alpha_limits.c, which scans every binary32 of [-5.6, -0] (its output: profiles/blend_alpha_limits.txt); here the
header's copy is checked against the ORACLE's exp (gso_exp, through ctypes): L(k) passes the alpha test, the next float
fails it, L(k) <= 5.6, the pass set over the 65 536 floats on either side of L(k) is up-closed, the opacity of a record gives
its byte back, and entry 0 is 0.  The exp is evaluated once over the union of the windows (they overlap from k = 32 on)."""
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WINDOW = 65536
F32 = np.float32


def _limit_table():
    text = open(os.path.join(ROOT, "wgpu-3dgs-core_amd", "csrc", "gs_render_kernels.h")).read()
    body = text[text.index("k_blend_np_limit[256]"):]
    body = body[body.index("{") + 1:body.index("};")]
    return np.asarray([int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", body)], dtype=np.uint32)


def _f(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _alpha_passes(op, e):
    """min(0.99, fl(op * e)) >= 1/255 in binary32, as the step and the oracle compute it"""
    return np.minimum(F32(0.99), F32(op) * np.asarray(e, dtype=np.float32)) >= F32(1.0) / F32(255.0)


@pytest.fixture(scope="module")
def table():
    t = _limit_table()
    assert t.shape == (256,)
    return t


@pytest.fixture(scope="module")
def exp_of(ob, table):
    """bits of np = -power -> gso_exp(-np), over the union of the windows around every L(k)"""
    lo = table[1:].astype(np.int64) - 1 - WINDOW
    hi = table[1:].astype(np.int64) - 1 + WINDOW
    spans = []                                              # the windows, merged (the table is ascending)
    for a, b in zip(np.maximum(lo, 0).tolist(), hi.tolist()):
        if spans and a <= spans[-1][1] + 1:
            spans[-1][1] = max(spans[-1][1], b)
        else:
            spans.append([a, b])
    bits = np.concatenate([np.arange(a, b + 1, dtype=np.uint32) for a, b in spans])
    gso_exp = ob.lib().gso_exp
    e = np.fromiter(map(gso_exp, (-_f(bits)).tolist()), dtype=np.float32, count=len(bits))
    return bits, e


def test_entry_zero_and_order(table):
    assert table[0] == 0
    assert (np.diff(table[1:].astype(np.int64)) > 0).all(), "L(k) grows with the opacity byte"
    assert table[1:].min() >= 1


def test_kop_gives_the_byte_back():
    k = np.arange(256, dtype=np.float32)
    op = k / F32(255.0)                                     # unorm8 of the byte, as project_geom stores it
    kop = (F32(255.0) * op + F32(0.5)).astype(np.uint32)    # two binary32 roundings, then truncation
    assert np.array_equal(kop, np.arange(256, dtype=np.uint32))


def test_limit_is_the_alpha_threshold_of_the_oracles_exp(table, exp_of):
    bits, e = exp_of
    for k in range(1, 256):
        op = F32(k) / F32(255.0)
        lbits = int(table[k]) - 1
        L = float(_f([lbits])[0])
        assert 0.0 < L <= 5.6, (k, L)
        i = int(np.searchsorted(bits, lbits))
        assert bits[i] == lbits and bits[i + 1] == lbits + 1
        assert _alpha_passes(op, e[i]), "L(%d) itself fails the alpha test" % k
        assert not _alpha_passes(op, e[i + 1]), "the float above L(%d) passes" % k
        a, b = int(np.searchsorted(bits, max(lbits - WINDOW, 0))), int(np.searchsorted(bits, lbits + WINDOW))
        assert b - a == min(lbits, WINDOW) + WINDOW
        ok = _alpha_passes(op, e[a:b + 1])
        n_pass = i - a + 1
        assert ok[:n_pass].all() and not ok[n_pass:].any(), "the pass set around L(%d) is not up-closed" % k


def test_generator_output_holds_the_headers_table(table):
    rows = [l for l in open(os.path.join(ROOT, "profiles", "blend_alpha_limits.txt")) if l.startswith("    0x")]
    words = [int(x, 16) for l in rows for x in re.findall(r"0x([0-9a-fA-F]{8})u", l)]
    assert np.array_equal(np.asarray(words, dtype=np.uint32), table)
    head = open(os.path.join(ROOT, "profiles", "blend_alpha_limits.txt")).read()
    assert "# bytes whose pass set is not up-closed: 0\n" in head
