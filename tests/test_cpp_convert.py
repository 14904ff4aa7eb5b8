"""gs3d::GaussiansBuffer::convert, the concat overload that converts its sources and LossyConfigError (include/gs3d.hpp):
compiles against the C ABI on the CPU; on the GPU the compiled test converts a buffer it built itself, with and without a
selection, compares it with a direct upload in the target layout, and merges buffers of three layouts."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    return ge.build_cpp_convert_test()


def test_cpp_convert_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_convert_on_gpu():
    exe = os.path.join(ROOT, "build", "test_convert")
    if not os.path.exists(exe):
        exe = _build()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "cpp convert OK" in res.stdout
