"""gs3d::GaussiansBuffer::convert, the concat overload that converts its sources and LossyConfigError (include/gs3d.hpp):
compiles against the C ABI on the CPU; on the GPU the compiled test converts a buffer it built itself, with and without a
selection, compares it with a direct upload in the target layout, and merges buffers of three layouts."""
import os

import pytest

import cpp_test


def test_cpp_convert_compiles():
    assert os.path.exists(cpp_test.build("convert"))


@pytest.mark.gpu
def test_cpp_convert_on_gpu():
    cpp_test.run("convert", "cpp convert OK")
