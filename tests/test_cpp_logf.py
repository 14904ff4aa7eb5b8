"""gs::gs_logf (csrc/gs_convert.h) against the C library's logf over EVERY binary32 input: tests/cpp/test_logf.cpp, a
stand-alone host program on up to 16 threads.  On glibc 2.35 — the C library tests/golden/logf_v1.npz was recorded on — the two
must be bit-equal; on another C library they must agree about NaNs and stay within 1 ulp, and the count of last-bit
differences is printed."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_cpp_logf_test()


def test_cpp_logf_sweeps_every_binary32_input():
    exe = _build()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "cpp logf OK" in res.stdout and "of 4294967296 inputs" in res.stdout
