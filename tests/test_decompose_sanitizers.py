"""The covariance decomposition under AddressSanitizer + UBSan on the CPU: the per-record functions that
gs_cov3d_decompose and gs_decompose_pods consist of (and that the device kernel runs) are compiled for the host into the
stand-alone program tests/cpp/sanitize_decompose.cpp, which runs them over the set of the decomposition tests and over
hostile words, each record in a heap block of exactly its size.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decomposition_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_decompose")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    build = subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host",
                            "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "cpp", "sanitize_decompose.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and "sanitize decompose OK" in res.stdout, res.stdout[-3000:]
