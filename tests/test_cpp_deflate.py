"""gs3d::gzip_fast, Buffer::gzip_fast and GaussiansBuffer::export_spz_fast (include/gs3d.hpp): compiles
against the C ABI on the CPU; on the GPU the compiled test compares the device member with the host member, inflates both and
reads a saved scene back."""
import os

import pytest

import cpp_test


def test_cpp_deflate_compiles():
    assert os.path.exists(cpp_test.build("deflate"))


@pytest.mark.gpu
def test_cpp_deflate_on_gpu():
    cpp_test.run("deflate", "cpp deflate OK")
