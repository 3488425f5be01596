"""Guard bands around every buffer the feature rank and the per-tensor norms touch (tests/rank_guard_run.py: the capture and the norms
on both hidden-48 nets, the Gram matrix at two ragged shapes) under RB_GUARD=1, in a child process as tests/test_redo_guard.py runs
its own (RB_GUARD is read when the library first allocates)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(which, timeout):
    env = dict(os.environ, RB_GUARD="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rank_guard_run.py"), which], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0 and "guard run ok" in p.stdout, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    assert p.stdout.count("overwritten guard bands 0") == 6 and "de48" in p.stdout and "canon48" in p.stdout and "gram (130" in p.stdout
    return p.stdout


def test_host_interpreted_rank_kernels_stay_inside_their_buffers():
    _run("emu", 600)


@pytest.mark.gpu
def test_hip_rank_kernels_stay_inside_their_buffers():
    _run("hip", 300)
