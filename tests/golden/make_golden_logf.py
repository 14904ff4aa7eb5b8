"""Writes tests/golden/logf_v1.npz: the inputs of tests/test_logf.py (binary32 bit patterns) and the bits the C library's
logf returns for them.  The committed file was recorded on glibc 2.35 (x86-64); run this script on that C library only —
it refuses any other unless --any-libc is given.

usage: python tests/golden/make_golden_logf.py [--any-libc]
"""
import ctypes as C
import os
import platform
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "logf_v1.npz")
RECORDED_ON = "glibc 2.35"


def inputs():
    """uint32 bit patterns: the specials, the ends of the normal and subnormal ranges, the 16 table-interval boundaries
    0x3f330000 + (i << 19) with their neighbours, 40 000 random patterns and 40 000 log-uniform values in [1e-12, 1e6]"""
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)
    u = lambda *v: np.array(v, dtype=np.uint32)
    special = np.concatenate([f(0.0, -0.0, np.inf, -np.inf, -1.0, 1.0), u(0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fa55aa5)])
    ends = u(0x00800000, 0x007fffff, 0x00800001,      # FLT_MIN and its neighbours
             0x00000001, 0x007fffff,                  # smallest and largest subnormal
             0x7f7fffff, 0x7f7ffffe,                  # FLT_MAX
             0x3f7fffff, 0x3f800001)                  # around 1
    b = (0x3f330000 + (np.arange(17, dtype=np.uint32) << 19)).astype(np.uint32)
    boundaries = np.concatenate([b - 1, b, b + 1])
    rng = np.random.default_rng(2024)
    random_bits = rng.integers(0, 1 << 32, 40000, dtype=np.uint64).astype(np.uint32)
    log_uniform = np.exp(rng.uniform(np.log(1e-12), np.log(1e6), 40000)).astype(np.float32).view(np.uint32)
    return np.concatenate([special, ends, boundaries, random_bits, log_uniform]).astype(np.uint32)


def libm_logf_bits(x_bits):
    libm = C.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
    out = np.zeros(len(x_bits), dtype=np.float32)
    arg = C.c_float()
    for k, b in enumerate(x_bits):
        # through a c_float holding the exact bits: a Python float would quieten a signalling NaN on the way
        C.memmove(C.byref(arg), C.byref(C.c_uint32(int(b))), 4)
        r = C.c_float(libm.logf(arg))
        out[k] = r.value
        C.memmove(out[k:k + 1].ctypes.data, C.byref(r), 4)
    return out.view(np.uint32)


def main():
    libc = " ".join(platform.libc_ver())
    if libc != RECORDED_ON and "--any-libc" not in sys.argv:
        sys.exit("this C library is %r; the golden file is defined as the output of %s" % (libc, RECORDED_ON))
    x = inputs()
    np.savez_compressed(PATH, x=x, y=libm_logf_bits(x), libc=np.array(libc))
    print("wrote %s: %d inputs, %s" % (PATH, len(x), libc))


if __name__ == "__main__":
    main()
