"""Out-of-bounds WRITE hunt for the dormant-unit recycling (run as a script, with RB_GUARD=1 in the environment, like
tests/reset_guard_run.py): k_unit_activity, k_dormant_mask and k_recycle_units on the two hidden-48 nets of tests/redo_scenarios.py —
the canonical one's runs of 49 columns and the data-efficient one's two-element output columns end inside quads — with every
caller-owned buffer canaried (tests/guarded_mem.py) and the library's own allocations guarded (rb_debug_check_guards).  Exits
non-zero if any guard band changed.
  python tests/redo_guard_run.py emu     host-interpreted kernels (CPU)
  python tests/redo_guard_run.py hip     librainbow_hip.so on cuda:0
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("RB_GUARD") == "1", "run with RB_GUARD=1"

import numpy as np  # noqa: E402

import redo_oracle as RD  # noqa: E402
import redo_scenarios as R  # noqa: E402
from rainbow_amd import _lib as L  # noqa: E402


def guards(lib, mem, label):
    nb, bad = C.c_int64(0), C.c_int64(0)
    L.check(lib, lib.rb_debug_check_guards(C.byref(nb), C.byref(bad)))
    cn, cbad = mem.check()
    print("  %-40s library blocks %4d, caller blocks %3d, overwritten guard bands %d" % (label, nb.value, cn, bad.value + len(cbad)),
          flush=True)
    assert nb.value > 0, "library allocations are not guarded (RB_GUARD read too late?)"
    assert bad.value == 0 and not cbad, (lib.rb_last_error().decode(), cbad)


def main(which):
    if which == "emu":
        from guarded_mem import GuardedNumpyMem as Mem
        from hipemu import loader
        lib = loader.load()
    else:
        from guarded_mem import GuardedTorchMem as Mem
        lib = L.load()
    for row in ("de48", "canon48"):
        rig = R.Rig(lib, Mem, row)
        m = rig.mem
        masks = R.masks_of(rig)
        # the measurement: activity, mask, counts and scores in canaried buffers of exactly U (n_layers) elements
        R.load_net(rig, 5)
        sbuf = m.upload(R.random_states(rig.c, 17))
        act, mask, counts, scores = m.empty((rig.U,), np.float64), m.empty((rig.U,), np.uint8), m.empty((len(rig.units),), np.int32), \
            m.empty((rig.U,), np.float32)
        L.check(lib, rig.activity(sbuf, 0, act))
        L.check(lib, rig.mask(act, 0.1, mask, counts, scores))
        m.sync()
        got = RD.dormant(rig.layout, m.download(act), 0.1)
        assert np.array_equal(m.download(mask), got[0]) and np.array_equal(m.download(counts), got[1])
        guards(lib, m, "%s, activity and mask" % row)
        for k, name in enumerate(("every", "first-and-last")):
            st = rig.fill(60 + k)
            L.check(lib, rig.recycle(masks[name]))
            want, _kind, _both = RD.recycle(rig.layout, st, masks[name], R.STD, R.SEED, R.DRAW)
            R.same(rig.state(), want, (row, name), keys="ptmv")
            guards(lib, m, "%s, recycle %s" % (row, name))
        rig.close()
    print("guard run ok")


if __name__ == "__main__":
    main(sys.argv[1])
