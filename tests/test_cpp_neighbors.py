"""gs3d::GaussiansBuffer::neighbor_counts and gs3d::Selection::select_neighbors (include/gs3d.hpp):
compiles against the C ABI on the CPU; on the GPU the compiled test counts the neighbours of a buffer it built itself and
compares counts, capped counts and the selected floaters with a host double loop using the same binary32 operations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "test_neighbors")


def _build():
    import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_neighbors.cpp"), "-o", EXE,
                    "-L" + os.path.join(ROOT, "wgpu-3dgs-core_amd", "lib"), "-lgs3d_hip",
                    "-Wl,-rpath,$ORIGIN/../wgpu-3dgs-core_amd/lib"], check=True)
    return EXE


def test_cpp_neighbors_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_neighbors_on_gpu():
    exe = _build()      # always: a binary left by an older source must not run in its place (one g++ -O1 of one file)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "cpp neighbors OK" in res.stdout
