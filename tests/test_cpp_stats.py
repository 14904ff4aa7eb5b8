"""gs3d::GaussiansBuffer::stats / histogram and gs3d::Selection::select_attribute (include/gs3d.hpp): compiles against the
C ABI on the CPU; on the GPU the compiled test takes the statistics and one histogram of a buffer it built itself and
compares count, bounds and row sums with a host loop over the same records."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    return ge.build_cpp_stats_test()


def test_cpp_stats_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_stats_on_gpu():
    exe = os.path.join(ROOT, "build", "test_stats")
    if not os.path.exists(exe):
        exe = _build()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "cpp stats OK" in res.stdout
