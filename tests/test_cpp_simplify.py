"""gs3d::GaussiansBuffer::simplify<To> (include/gs3d.hpp): compiles against the C ABI on the CPU; on the GPU the compiled test
simplifies a small buffer it built itself and checks K, the cell plane and one merged cell against values computed in the
test."""
import os

import pytest

import cpp_test


def test_cpp_simplify_compiles():
    assert os.path.exists(cpp_test.build("simplify"))


@pytest.mark.gpu
def test_cpp_simplify_on_gpu():
    cpp_test.run("simplify", "cpp simplify OK")
