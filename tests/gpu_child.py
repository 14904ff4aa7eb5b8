"""The one launcher of the GPU tests' child processes, and the rig their children open.

Parent side: run() starts a child, one at a time, and keeps the rule of a shared GPU: after a child that ended on a signal,
an abort, its time limit or a reported GPU fault, no further child is started by this pytest process.  Child side:
child_rig() is what a child that renders opens and closes around its body."""
import contextlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tests/conftest.py's three pins (the reasons are there): a child started outside pytest gets the same ones
PINS = (("GS3D_TILE_MASKS", "1"), ("GS3D_ROUNDS", "0"), ("GS3D_ROUND_PARTITION", "1"))

# how HIP reports a GPU fault while the program may go on running, to an ordinary status
FAULT_WORDS = ("an illegal memory access was encountered", "Memory access fault by GPU")


class ChildRunner:
    """run() and the label of the first child that ended abnormally (None: none has)"""

    def __init__(self):
        self.dead = None

    def run(self, argv, *, env=None, unset=(), timeout, label, check=True, expect=None, cwd=ROOT):
        """Run [sys.executable] + argv under os.environ minus `unset` (a name ending in * is a prefix) plus `env`, output
        captured as one text.  check: status 0 and, if given, `expect` in the output.  Returns the CompletedProcess."""
        assert self.dead is None, "not started: the %s child ended abnormally" % self.dead
        child_env = {k: v for k, v in os.environ.items()
                     if not any(k.startswith(u[:-1]) if u.endswith("*") else k == u for u in unset)}
        child_env.update(env or {})
        try:
            res = subprocess.run([sys.executable] + list(argv), cwd=cwd, env=child_env, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            self.dead = label
            raise
        # a signal, an abort, a time limit (pytest's own codes are 0 to 5), or a fault that HIP only reported
        if res.returncode < 0 or res.returncode >= 124 or any(w in res.stdout for w in FAULT_WORDS):
            self.dead = label
        if check:
            assert res.returncode == 0, res.stdout[-3000:]
            assert expect is None or expect in res.stdout, res.stdout[-3000:]
        return res


_runner = ChildRunner()      # pytest runs the GPU suite in one process: one instance is the whole suite's
run = _runner.run


def load_npz(path):
    return dict(np.load(path))


@contextlib.contextmanager
def child_rig():
    """(gs, ob, dev, st): the package, the built oracle binding, Device(0) and a stream, closed on the way out"""
    for key, val in PINS:
        os.environ.setdefault(key, val)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import wgpu_3dgs_core_amd as gs
    from oracle import binding as ob
    ob.build()
    ob.lib()
    dev = gs.Device(0)
    st = dev.create_stream()
    try:
        yield gs, ob, dev, st
    finally:
        st.close()
        dev.close()
