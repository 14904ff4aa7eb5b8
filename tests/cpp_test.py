"""The compiled host tests (tests/cpp/test_<name>.cpp; __graft_entry__.CPP_TESTS says how each is compiled): build one, run one."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exe(name):
    return os.path.join(ROOT, "build", "test_" + name)


def build(name):
    """compile the test (and, by importing the package, the library it links, if needed); returns the executable's path"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    if ge.CPP_TESTS[name][2]:
        import wgpu_3dgs_core_amd  # noqa: F401  (builds the library if needed)
    return ge.build_cpp_test(name)


def run(name, marker, timeout=120, args=()):
    """run the test, built first where no executable is there: exit status 0 and the marker word in its output, which is
    returned"""
    path = exe(name) if os.path.exists(exe(name)) else build(name)
    res = subprocess.run([path, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout
    assert marker in res.stdout, res.stdout
    return res.stdout
