"""gs3d::Selection and the selection overload of gs3d::Renderer::render (include/gs3d.hpp): compiles against the C ABI
on the CPU; on the GPU the compiled test crops a scene with a box and compares the frame with one of the kept half."""
import os

import pytest

import cpp_test


def test_cpp_selection_compiles():
    assert os.path.exists(cpp_test.build("selection"))


@pytest.mark.gpu
def test_cpp_selection_on_gpu():
    cpp_test.run("selection", "cpp selection OK")
