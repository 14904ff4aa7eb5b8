"""gs3d::Renderer::render_contrib, gs3d::contributions_clear and gs3d::Selection::select_contribution (include/gs3d.hpp):
compiles against the C ABI on the CPU; on the GPU the compiled test renders one small frame twice into the same records and
checks that the second frame doubles every sum and hit count."""
import os

import pytest

import cpp_test


def test_cpp_contrib_compiles():
    assert os.path.exists(cpp_test.build("contrib"))


@pytest.mark.gpu
def test_cpp_contrib_on_gpu():
    cpp_test.run("contrib", "cpp contrib OK")
