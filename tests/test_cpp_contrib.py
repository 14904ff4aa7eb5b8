"""gs3d::Renderer::render_contrib, gs3d::contributions_clear and gs3d::Selection::select_contribution (include/gs3d.hpp):
compiles against the C ABI on the CPU; on the GPU the compiled test renders one small frame twice into the same records and
checks that the second frame doubles every sum and hit count."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    return ge.build_cpp_contrib_test()


def test_cpp_contrib_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_contrib_on_gpu():
    exe = os.path.join(ROOT, "build", "test_contrib")
    if not os.path.exists(exe):
        exe = _build()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "cpp contrib OK" in res.stdout
