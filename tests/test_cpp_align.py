"""gs3d::GaussiansBuffer::knn_to, ::pair_sums, gs3d::rigid_fit and gs3d::compose (include/gs3d.hpp): compile against the C
ABI on the CPU; on the GPU the compiled test searches two small buffers it built itself and checks the rows, the overlap
selection, the pair sums and one ICP step against values computed by a plain double loop in the test."""
import os

import pytest

import cpp_test


def test_cpp_align_compiles():
    assert os.path.exists(cpp_test.build("align"))


@pytest.mark.gpu
def test_cpp_align_on_gpu():
    cpp_test.run("align", "cpp align OK")
