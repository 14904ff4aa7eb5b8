"""The frame plan (csrc/gs_policy.h) is plain host code without a HIP header: tests/cpp/test_policy.cpp pins its
rules on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_rules():
    out = os.path.join(ROOT, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "test_policy")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "wgpu-3dgs-core_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_policy.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and "policy OK" in res.stdout, res.stdout
