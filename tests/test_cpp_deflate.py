"""gs3d::gzip_fast, Buffer::gzip_fast and GaussiansBuffer::export_spz_fast (include/gs3d.hpp): compiles
against the C ABI on the CPU; on the GPU the compiled test compares the device member with the host member, inflates both and
reads a saved scene back."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    return ge.build_cpp_deflate_test()


def test_cpp_deflate_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_deflate_on_gpu():
    exe = os.path.join(ROOT, "build", "test_deflate")
    if not os.path.exists(exe):
        exe = _build()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "cpp deflate OK" in res.stdout
