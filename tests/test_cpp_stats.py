"""gs3d::GaussiansBuffer::stats / histogram and gs3d::Selection::select_attribute (include/gs3d.hpp): compiles against the
C ABI on the CPU; on the GPU the compiled test takes the statistics and one histogram of a buffer it built itself and
compares count, bounds and row sums with a host loop over the same records."""
import os

import pytest

import cpp_test


def test_cpp_stats_compiles():
    assert os.path.exists(cpp_test.build("stats"))


@pytest.mark.gpu
def test_cpp_stats_on_gpu():
    cpp_test.run("stats", "cpp stats OK")
