"""gs3d::GaussiansBuffer::edit / extract and gs3d::sh_rotation_matrices (include/gs3d.hpp): compiles against the C ABI on
the CPU; on the GPU the compiled test edits and splits a grid of Gaussians and checks the records it downloads."""
import os

import pytest

import cpp_test


def test_cpp_edit_compiles():
    assert os.path.exists(cpp_test.build("edit"))


@pytest.mark.gpu
def test_cpp_edit_on_gpu():
    cpp_test.run("edit", "cpp edit OK")
