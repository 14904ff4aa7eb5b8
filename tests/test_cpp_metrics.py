"""gs3d::image_compare (include/gs3d.hpp): compiles against the C ABI on the CPU; on the GPU the compiled test compares a
small image with itself and with a copy that has one changed pixel."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    return ge.build_cpp_metrics_test()


def test_cpp_metrics_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_metrics_on_gpu():
    exe = os.path.join(ROOT, "build", "test_metrics")
    if not os.path.exists(exe):
        exe = _build()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "cpp metrics OK" in res.stdout
