"""Out-of-bounds WRITE hunt for the feature rank and the per-tensor norms (run as a script, with RB_GUARD=1 in the environment, like
tests/redo_guard_run.py): the capture of both layers, k_gram_f64 at (33, 70, 72) and (130, 257, 260) — ragged tiles, ragged k — and
k_tensor_partials / k_tensor_fold on the two hidden-48 nets of tests/redo_scenarios.py, with every caller-owned buffer canaried
(tests/guarded_mem.py: Phi, K, the captured rows and the norms sit in buffers of exactly their size) and the library's own
allocations guarded (rb_debug_check_guards).  Exits non-zero if any guard band changed.
  python tests/rank_guard_run.py emu     host-interpreted kernels (CPU)
  python tests/rank_guard_run.py hip     librainbow_hip.so on cuda:0
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("RB_GUARD") == "1", "run with RB_GUARD=1"

import numpy as np  # noqa: E402

import rank_scenarios as K  # noqa: E402
import redo_scenarios as R  # noqa: E402
from rainbow_amd import _lib as L  # noqa: E402


def guards(lib, mem, label, library=True):
    nb, bad = C.c_int64(0), C.c_int64(0)
    L.check(lib, lib.rb_debug_check_guards(C.byref(nb), C.byref(bad)))
    cn, cbad = mem.check()
    print("  %-40s library blocks %4d, caller blocks %3d, overwritten guard bands %d" % (label, nb.value, cn, bad.value + len(cbad)),
          flush=True)
    assert not library or nb.value > 0, "library allocations are not guarded (RB_GUARD read too late?)"
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
        m, B = rig.mem, rig.c["batch"]
        R.load_net(rig, 5)
        sbuf = m.upload(R.random_states(rig.c, 17))
        for which_layer in (K.HIDDEN, K.CONV):
            d = K.feature_dim(lib, rig.cfg, which_layer)
            for ld in (d, d + 4):
                out = m.empty((B * ld - (ld - d),), np.float32)         # (the last row's pad columns are not the call's to write)
                L.check(lib, K.features(rig, sbuf, which_layer, out, ld))
                m.sync()
                assert np.abs(m.download(out)).sum() > 0
        guards(lib, m, "%s, capture" % row)
        a, b = K.scaled_buffers(rig, 70)
        got = K.run_norms(rig, a, b)
        K.assert_norms(row, got, K.norms_reference(rig.layout, a, b), rig.layout)
        guards(lib, m, "%s, tensor norms" % row)
        rig.close()
    for n, d, ld in ((33, 70, 72), (130, 257, 260)):
        mem = Mem()
        phi, want, A = K.gram_case(n, d)
        pbuf = mem.upload(K.padded(phi, ld)[:n])                        # exactly n rows: nothing behind the last one
        kbuf = mem.empty((n, n), np.float64)
        L.check(lib, lib.rb_gram_f64(mem.ptr(pbuf), n, d, ld, mem.ptr(kbuf), mem.stream))
        mem.sync()
        assert np.all(np.abs(mem.download(kbuf) - want) <= d * K.U53 * A)
        guards(lib, mem, "gram (%d, %d, %d)" % (n, d, ld), library=False)
    print("guard run ok")


if __name__ == "__main__":
    main(sys.argv[1])
