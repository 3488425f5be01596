"""Out-of-bounds WRITE hunt for the per-row-noise act path (run as a script, with RB_GUARD=1 in the environment, like
tests/guard_run.py): rb_learner_noise_rows and rb_learner_act_batch_rows with every caller-owned buffer canaried
(tests/guarded_mem.py) and the library's own allocations guarded (rb_debug_check_guards), at row counts on both sides of the
m-tiles and past the learner's 3 * batch forward rows.  Exits non-zero if any guard band changed.
  python tests/noise_rows_guard_run.py emu     host-interpreted kernels, small shapes (CPU)
  python tests/noise_rows_guard_run.py hip     librainbow_hip.so on cuda:0, the BASELINE cfg-2 network included
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("RB_GUARD") == "1", "run with RB_GUARD=1"

import noise_rows_scenarios as NR  # noqa: E402
from oracle import learner_oracle as O  # noqa: E402
from rainbow_amd import _lib as L  # noqa: E402

CASES = {"emu": (("k10", (1, 17)), ("atoms21", (3,))),
         "hip": (("k10", (1, 16, 33)), ("atoms21", (3,)), (NR.CFG2, (1, 64, 100, 256)))}


def run(lib, mem, name, ns):
    cfg = O.Config(**NR.shape_of(name))
    ad = NR.make_learner(lib, mem, name, NR.scaled_params(cfg))
    n_max = max(ns)
    states = mem.upload(np.random.RandomState(2).random_sample((n_max, cfg.history, 84, 84)).astype(np.float32))
    noise = mem.empty((n_max, ad.n_noise), np.float32)
    L.check(lib, lib.rb_learner_noise_rows(ad.h, n_max, 3, 11, 5, None, mem.ptr(noise), mem.stream))
    for n in ns:
        a, q = mem.empty((n,), np.int32), mem.empty((n,), np.float32)
        L.check(lib, lib.rb_learner_act_batch_rows(ad.h, mem.ptr(states), n, mem.ptr(noise), mem.ptr(a), mem.ptr(q), mem.stream))
        mem.sync()
        assert np.isfinite(mem.download(q)).all() and 0 <= mem.download(a).min() and mem.download(a).max() < cfg.actions
        nb, bad = C.c_int64(0), C.c_int64(0)
        L.check(lib, lib.rb_debug_check_guards(C.byref(nb), C.byref(bad)))
        cn, cbad = mem.check()
        print("  %-32s n = %3d: library blocks %4d, caller blocks %3d, overwritten guard bands %d"
              % (name, n, nb.value, cn, bad.value + len(cbad)), flush=True)
        assert nb.value > 0, "library allocations are not guarded (RB_GUARD read too late?)"
        assert bad.value == 0 and not cbad, (lib.rb_last_error().decode(), cbad)
    ad.close()


def main(which):
    if which == "emu":
        from guarded_mem import GuardedNumpyMem as Mem
        from hipemu import loader
        lib = loader.load()
    else:
        from guarded_mem import GuardedTorchMem as Mem
        lib = L.load()
    for name, ns in CASES[which]:
        run(lib, Mem(), name, ns)
    print("guard run ok")


if __name__ == "__main__":
    main(sys.argv[1])
