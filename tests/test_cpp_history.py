"""gs3d::Snapshot, gs3d::GaussiansBuffer::snapshot / restore / concat and gs3d::Selection::select_range (include/gs3d.hpp):
compiles against the C ABI on the CPU; on the GPU the compiled test takes a snapshot, edits, exchanges twice, concatenates
and range-selects, and compares the bytes it downloads."""
import os

import pytest

import cpp_test


def test_cpp_history_compiles():
    assert os.path.exists(cpp_test.build("history"))


@pytest.mark.gpu
def test_cpp_history_on_gpu():
    cpp_test.run("history", "cpp history OK")
