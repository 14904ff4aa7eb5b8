"""gs3d::GaussiansBuffer::neighbor_counts and gs3d::Selection::select_neighbors (include/gs3d.hpp):
compiles against the C ABI on the CPU; on the GPU the compiled test counts the neighbours of a buffer it built itself and
compares counts, capped counts and the selected floaters with a host double loop using the same binary32 operations."""
import os

import pytest

import cpp_test


def test_cpp_neighbors_compiles():
    assert os.path.exists(cpp_test.build("neighbors"))


@pytest.mark.gpu
def test_cpp_neighbors_on_gpu():
    cpp_test.build("neighbors")     # always: a binary left by an older source must not run in its place (one g++ -O1 of one file)
    cpp_test.run("neighbors", "cpp neighbors OK")
