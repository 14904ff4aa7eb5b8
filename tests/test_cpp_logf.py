"""gs::gs_logf (csrc/gs_convert.h) against the C library's logf over EVERY binary32 input: tests/cpp/test_logf.cpp, a
stand-alone host program on up to 16 threads.  On glibc 2.35 — the C library tests/golden/logf_v1.npz was recorded on — the two
must be bit-equal; on another C library they must agree about NaNs and stay within 1 ulp, and the count of last-bit
differences is printed."""
import cpp_test


def test_cpp_logf_sweeps_every_binary32_input():
    cpp_test.build("logf")
    out = cpp_test.run("logf", "cpp logf OK", timeout=600)
    print(out)
    assert "of 4294967296 inputs" in out
