"""gs3d::GaussiansBuffer::edit / extract and gs3d::sh_rotation_matrices (include/gs3d.hpp): compiles against the C ABI on
the CPU; on the GPU the compiled test edits and splits a grid of Gaussians and checks the records it downloads."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    return ge.build_cpp_edit_test()


def test_cpp_edit_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_edit_on_gpu():
    exe = os.path.join(ROOT, "build", "test_edit")
    if not os.path.exists(exe):
        exe = _build()
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "cpp edit OK" in res.stdout
