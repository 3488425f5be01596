"""Guard bands around the target buffer (and every other one) while the optimiser pass carries the target's EMA: one hosted pass and
one pair pass with tau = 0.5 under RB_GUARD=1, in a child process as tests/test_guard.py runs its own (RB_GUARD is read when the
library first allocates)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(which, timeout):
    env = dict(os.environ, RB_GUARD="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "target_ema_guard_run.py"), which], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0 and "guard run ok" in p.stdout, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    assert p.stdout.count("overwritten guard bands 0") == 2 and "hosted pass" in p.stdout and "pair pass" in p.stdout
    return p.stdout


def test_host_interpreted_ema_passes_stay_inside_their_buffers():
    _run("emu", 900)


@pytest.mark.gpu
def test_hip_ema_passes_stay_inside_their_buffers():
    _run("hip", 300)
