"""gs3d::GaussiansBuffer::knn, Selection::select_knn and gs3d::knn_summary (include/gs3d.hpp): compile against the C ABI on
the CPU; on the GPU the compiled test searches a small buffer it built itself and checks the rows, the selection of the
incomplete rows and the summary against values computed by a plain double loop in the test."""
import os

import pytest

import cpp_test


def test_cpp_knn_compiles():
    assert os.path.exists(cpp_test.build("knn"))


@pytest.mark.gpu
def test_cpp_knn_on_gpu():
    cpp_test.run("knn", "cpp knn OK")
