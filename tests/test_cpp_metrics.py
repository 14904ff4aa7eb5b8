"""gs3d::image_compare (include/gs3d.hpp): compiles against the C ABI on the CPU; on the GPU the compiled test compares a
small image with itself and with a copy that has one changed pixel."""
import os

import pytest

import cpp_test


def test_cpp_metrics_compiles():
    assert os.path.exists(cpp_test.build("metrics"))


@pytest.mark.gpu
def test_cpp_metrics_on_gpu():
    cpp_test.run("metrics", "cpp metrics OK")
