"""Out-of-bounds WRITE hunt for the device Breakout environment (run as a script, with RB_GUARD=1 in the environment, like
tests/noise_rows_guard_run.py): rb_breakout_reset / _step / _reset_stats / _set_state with the library's own allocation — the
64-byte state blocks — guarded (rb_debug_check_guards) and every caller-owned buffer canaried (tests/guarded_mem.py), at
stream counts 1, 7 and 64, through game ends, lost lives and step caps.  Exits non-zero if any guard band changed.
  python tests/breakout_guard_run.py emu     host-interpreted kernels (CPU)
  python tests/breakout_guard_run.py hip     librainbow_hip.so on cuda:0
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("RB_GUARD") == "1", "run with RB_GUARD=1"

import breakout_scenarios as BS  # noqa: E402
import device_loop_scenarios as DS  # noqa: E402
from rainbow_amd import _lib as L  # noqa: E402

CASES = ((1, 1, 40), (7, 4, 40), (64, 2, 30))          # (streams, history, rounds); max_steps = 25: every run meets the cap


def run(lib, mem, S, history, rounds):
    rs = np.random.RandomState(S)
    env = BS.BreakoutHandle(lib, mem, S, history, 25, seed=S)
    env.reset()
    ends = 0
    for r in range(rounds):
        _, _, nonterminals = env.step(DS.random_actions(rs, S))
        ends += int((nonterminals == 0).sum())
        if r == rounds // 2:
            env.reset_stats()
            assert env.set_state(env.get_state()) == 0
    assert ends >= S and env.stats()["steps"] == S * (rounds - rounds // 2 - 1)
    nb, bad = C.c_int64(0), C.c_int64(0)
    L.check(lib, lib.rb_debug_check_guards(C.byref(nb), C.byref(bad)))
    cn, cbad = mem.check()
    print("  S = %2d history = %d: library blocks %d, caller blocks %d, overwritten guard bands %d"
          % (S, history, nb.value, cn, bad.value + len(cbad)), flush=True)
    assert nb.value > 0, "library allocations are not guarded (RB_GUARD read too late?)"
    assert bad.value == 0 and not cbad, (lib.rb_last_error().decode(), cbad)
    env.close()


def main(which):
    if which == "emu":
        from guarded_mem import GuardedNumpyMem as Mem
        from hipemu import loader
        lib = loader.load()
    else:
        from guarded_mem import GuardedTorchMem as Mem
        lib = L.load()
    for S, history, rounds in CASES:
        run(lib, Mem(), S, history, rounds)
    print("guard run ok")


if __name__ == "__main__":
    main(sys.argv[1])
