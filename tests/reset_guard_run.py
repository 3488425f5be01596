"""Out-of-bounds WRITE hunt for the shrink-and-perturb reset (run as a script, with RB_GUARD=1 in the environment, like
tests/guard_run.py): k_shrink_perturb on the two hidden-48 nets of tests/reset_scenarios.py — the canonical one's last tensors end
inside a quad, the data-efficient one's two-float biases share one — with every caller-owned buffer canaried (tests/guarded_mem.py)
and the library's own allocations guarded (rb_debug_check_guards).  Exits non-zero if any guard band changed.
  python tests/reset_guard_run.py emu     host-interpreted kernels (CPU)
  python tests/reset_guard_run.py hip     librainbow_hip.so on cuda:0
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("RB_GUARD") == "1", "run with RB_GUARD=1"

import reset_oracle as RO  # noqa: E402
import reset_scenarios as R  # noqa: E402
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
    for net in ("de48", "canon48"):
        rig = R.Rig(lib, Mem, net)
        for k, (ae, ah) in enumerate(((0.5, 0.0), (0.0, 0.25))):
            st = rig.fill(60 + k)
            L.check(lib, rig.reset(ae, ah))
            want, _ = RO.shrink_perturb(rig.layout, st, ae, ah, R.STD, R.SEED, R.DRAW)
            R.same(rig.state(), want, (net, ae, ah), keys="ptmv")
            guards(lib, rig.mem, "%s, alpha (%g, %g)" % (net, ae, ah))
        rig.close()
    print("guard run ok")


if __name__ == "__main__":
    main(sys.argv[1])
