"""The host encoder of the Huffman-only gzip member under AddressSanitizer + UBSan (CPU only): the product
sources are rebuilt with the sanitizers into the stand-alone program tests/cpp/fuzz_deflate.cpp, which encodes the inputs of
the format's tests and mutations of them into buffers of exactly the returned size and inflates them with zlib and with
gs_spz_decompress."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_encoder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "fuzz_deflate")
    csrc = os.path.join(ROOT, "wgpu-3dgs-core_amd", "csrc")
    # gs_spz.cpp (gs_spz_decompress) also holds the format-agnostic readers, which need gs_ply.cpp to link.  The sanitizer
    # runtimes are linked statically: the program does not depend on where a shared runtime comes in the library list.
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                            "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-pthread", os.path.join(ROOT, "tests", "cpp", "fuzz_deflate.cpp"),
                            os.path.join(csrc, "gs_deflate.cpp"), os.path.join(csrc, "gs_spz.cpp"), os.path.join(csrc, "gs_ply.cpp"),
                            "-lz", "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    res = subprocess.run([exe, "200"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and "fuzz OK" in res.stdout, res.stdout[-3000:]
