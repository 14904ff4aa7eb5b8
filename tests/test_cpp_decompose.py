"""gs3d::GaussiansBuffer::decompose<SH>, GaussianPod::decompose<SH> and cov3d_decompose (include/gs3d.hpp): compiles against the
C ABI on the CPU; on the GPU the compiled test decomposes an SH f16 / cov f16 buffer it built itself, with and without a
selection, compares it with the host decomposition, and exports the result where the source throws LossyConfigError."""
import os

import pytest

import cpp_test


def test_cpp_decompose_compiles():
    assert os.path.exists(cpp_test.build("decompose"))


@pytest.mark.gpu
def test_cpp_decompose_on_gpu():
    cpp_test.run("decompose", "cpp decompose OK")
