"""Contribution frames in the frame plan (csrc/gs_policy.h, Requests::single_round): tests/cpp/test_policy_contrib.cpp pins,
on the CPU, that they are planned as one round under every pin and feedback state, as a frame pinned to one round is."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_contribution_frames_plan_one_round():
    out = os.path.join(ROOT, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "test_policy_contrib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "wgpu-3dgs-core_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_policy_contrib.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and "policy contrib OK" in res.stdout, res.stdout
