"""gs3d::GaussiansBuffer::components, gs3d::Selection::select_components and ::select_connected (include/gs3d.hpp,
DESIGN.md §3.16): compiles against the C ABI on the CPU; on the GPU the compiled test builds a buffer itself and compares
labels, sizes, info and both selects with a host union-find using the same binary32 operations."""
import os

import pytest

import cpp_test


def test_cpp_components_compiles():
    assert os.path.exists(cpp_test.build("components"))


@pytest.mark.gpu
def test_cpp_components_on_gpu():
    cpp_test.build("components")     # always: a binary left by an older source must not run in its place (one g++ -O1 of one file)
    cpp_test.run("components", "cpp components OK")
