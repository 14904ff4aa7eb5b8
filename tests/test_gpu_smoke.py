"""`__graft_entry__.smoke()` the way the driver runs it at round end: a fresh process WITHOUT the variables tests/conftest.py
pins (tile rect version, rounds) — the renderer's own per-scene choices, and a checker that has to follow them (round 5: the
oracle binding defaults to rect version 4, the renderer picks version 3 for a scene this small, and nothing but the driver
ran smoke())."""
import pytest

import gpu_child


@pytest.mark.gpu
def test_smoke_in_a_clean_environment():
    gpu_child.run(["-c", "import __graft_entry__ as g; g.smoke()"], unset=("GS3D_*",), timeout=600, label="smoke", expect="smoke OK")
