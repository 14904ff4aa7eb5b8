"""tests/gpu_child.py's launcher without a GPU: its children are `python -c` one-liners that never import the package.
Every test has a fresh ChildRunner, so that a child killed here stops nothing of the suite's own."""
import os
import subprocess

import pytest

from gpu_child import ChildRunner

FAULT = "an illegal memory access was encountered"


def _touch(path):
    return ["-c", "open(%r, 'w').close()" % str(path)]


def test_status_0_passes_and_the_expected_word_is_asserted():
    r = ChildRunner()
    res = r.run(["-c", "print('all fine')"], timeout=30, label="fine", expect="all fine")
    assert res.returncode == 0 and res.stdout == "all fine\n"
    with pytest.raises(AssertionError, match="something else entirely"):      # the message carries the child's output
        r.run(["-c", "print('something else entirely')"], timeout=30, label="no word", expect="all fine")
    assert r.dead is None


def test_unset_removes_and_env_adds_variables(monkeypatch):
    monkeypatch.setenv("GS3D_CHILD_TEST_A", "a")
    monkeypatch.setenv("GS3D_CHILD_TEST_B", "b")
    monkeypatch.setenv("GPUCHILD_EXACT", "x")
    monkeypatch.setenv("GPUCHILD_EXACT_NOT", "y")
    show = ["-c", "import os; print(sorted((k, v) for k, v in os.environ.items() if k.startswith(('GS3D_CHILD', 'GPUCHILD'))))"]
    r = ChildRunner()
    assert eval(r.run(show, timeout=30, label="as is").stdout) == [
        ("GPUCHILD_EXACT", "x"), ("GPUCHILD_EXACT_NOT", "y"), ("GS3D_CHILD_TEST_A", "a"), ("GS3D_CHILD_TEST_B", "b")]
    res = r.run(show, unset=("GPUCHILD_EXACT", "GS3D_CHILD_*"), env={"GPUCHILD_NEW": "n", "GS3D_CHILD_TEST_B": "again"},
                timeout=30, label="changed")
    assert eval(res.stdout) == [("GPUCHILD_EXACT_NOT", "y"), ("GPUCHILD_NEW", "n"), ("GS3D_CHILD_TEST_B", "again")]
    assert os.environ["GS3D_CHILD_TEST_A"] == "a" and "GPUCHILD_NEW" not in os.environ      # the parent's own is untouched


def test_an_ordinary_failure_does_not_stop_the_runner(tmp_path):
    r = ChildRunner()
    with pytest.raises(AssertionError, match="about to fail"):
        r.run(["-c", "import sys; print('about to fail'); sys.exit(1)"], timeout=30, label="exit 1")
    assert r.dead is None
    r.run(_touch(tmp_path / "next"), timeout=30, label="next")
    assert (tmp_path / "next").exists()


@pytest.mark.parametrize("code,timeout,raised", [
    ("import sys; sys.exit(134)", 30, AssertionError),
    ("import sys; sys.exit(139)", 30, AssertionError),
    ("import time; time.sleep(30)", 1, subprocess.TimeoutExpired),
    ("print('hipErrorIllegalAddress: %s')" % FAULT, 30, None),       # status 0: HIP reported the fault and the program went on
], ids=["exit 134", "exit 139", "time limit", "fault reported"])
def test_after_an_abnormal_end_nothing_more_is_started(tmp_path, code, timeout, raised):
    r = ChildRunner()
    if raised is None:
        assert r.run(["-c", code], timeout=timeout, label="first").returncode == 0
    else:
        with pytest.raises(raised):
            r.run(["-c", code], timeout=timeout, label="first")
    assert r.dead == "first"
    for check in (True, False):
        with pytest.raises(AssertionError, match="not started: the first child ended abnormally"):
            r.run(_touch(tmp_path / "second"), timeout=30, label="second", check=check)
    assert not (tmp_path / "second").exists()


def test_check_false_returns_a_nonzero_status_and_stops_nothing(tmp_path):
    r = ChildRunner()
    res = r.run(["-c", "import sys; print('three'); sys.exit(3)"], timeout=30, label="exit 3", check=False)
    assert res.returncode == 3 and res.stdout == "three\n" and r.dead is None
    r.run(_touch(tmp_path / "next"), timeout=30, label="next")
    assert (tmp_path / "next").exists()


def test_check_false_still_applies_the_stop_rule():
    r = ChildRunner()
    assert r.run(["-c", "import sys; sys.exit(134)"], timeout=30, label="abort", check=False).returncode == 134
    assert r.dead == "abort"
