"""gs_rigid_fit and gs_model_transform_compose under AddressSanitizer + UBSan on the CPU: their host
arithmetic (csrc/gs_align_fit.h, which gs_align.hip wraps into the C ABI) is compiled into the stand-alone program
tests/cpp/sanitize_align_fit.cpp, which runs well-posed fits, every refusal and hostile sums, each record in a heap block
of exactly its size.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rigid_fit_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_align_fit")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            os.path.join(ROOT, "tests", "cpp", "sanitize_align_fit.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and "sanitize align fit OK" in res.stdout, res.stdout[-3000:]
