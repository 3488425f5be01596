"""Out-of-bounds WRITE hunt for the optimiser pass with an EMA target (run as a script, with RB_GUARD=1 in the environment, like
tests/guard_run.py): one pass hosted by the sampler launch and one (mu, sigma) pair pass, hosted as well, with tau = 0.5, every
caller-owned buffer — the target parameters among them — canaried (tests/guarded_mem.py) and the library's own allocations
guarded (rb_debug_check_guards).  Exits non-zero if any guard band changed.
  python tests/target_ema_guard_run.py emu     host-interpreted kernels (CPU)
  python tests/target_ema_guard_run.py hip     librainbow_hip.so on cuda:0
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("RB_GUARD") == "1", "run with RB_GUARD=1"

import optimizer_scenarios as S  # noqa: E402
import scenarios  # noqa: E402
import target_ema_scenarios as T  # noqa: E402
from rainbow_amd import _lib as L  # noqa: E402
from ts_scenarios import ts_args  # noqa: E402

NAME, TAU = "dataeff", 0.5


def guards(lib, mem, label):
    nb, bad = C.c_int64(0), C.c_int64(0)
    L.check(lib, lib.rb_debug_check_guards(C.byref(nb), C.byref(bad)))
    cn, cbad = mem.check()
    print("  %-40s library blocks %4d, caller blocks %3d, overwritten guard bands %d" % (label, nb.value, cn, bad.value + len(cbad)),
          flush=True)
    assert nb.value > 0, "library allocations are not guarded (RB_GUARD read too late?)"
    assert bad.value == 0 and not cbad, (lib.rb_last_error().decode(), cbad)


def hosted(lib, Mem):
    """A synthetic gradient, the pass left pending and hosted by the next sampler launch (k_sample<1024, 4, true>, plain workgroups)."""
    os.environ["RB_OPTS"] = "spec_draw=0"
    rig = S.build_rig(lib, Mem, NAME, True, L.LEARNER_DEFER_UPDATE)
    T.set_tau(rig, TAU)
    t0 = T.target(rig)
    g = S.make_grad(rig.ad.layout, rig.ad.n_params, 3, "scales")
    _, after, _, was_hosted = S.run_synthetic(rig, "hosted", g, S.resolve_max_norm("bite", g), 4)
    assert was_hosted == 1
    T.check_target("guard_hosted", TAU, t0, after["p"], T.target(rig), "guard run, hosted")
    guards(lib, rig.mem, "hosted pass, tau = %g" % TAU)
    S.close_rig(rig)


def pairs(lib, Mem):
    """A real train step under DEFER_UPDATE | IMPLICIT_SIGMA, its pair pass hosted by the next sampler launch."""
    os.environ["RB_OPTS"] = "implicit_small=1,spec_draw=0"
    flags = L.LEARNER_DEFER_UPDATE | L.LEARNER_IMPLICIT_SIGMA
    assert S.plan_reports_implicit_sigma(lib, NAME, os.environ["RB_OPTS"], flags)
    rig = S.build_rig(lib, Mem, NAME, True, flags)
    m, ad = rig.mem, rig.ad
    T.set_tau(rig, TAU)
    ts = ts_args(NAME, m, rig.rp, ad, rig.out, rig.job, 0.4, 0, 1e-3)
    ts.norm_dev = m.ptr(rig.norm)
    L.check(lib, lib.rb_learner_train_step(ad.h, C.byref(ts), m.stream))
    t0 = T.target(rig)
    job2, job_out = L.NoiseJob(), L.NoiseJob()
    L.check(lib, lib.rb_learner_noise_job(ad.h, 2, C.byref(job2)))
    assert lib.rb_learner_attach_pending(ad.h, C.byref(job2), scenarios.LEARN_CONFIGS[NAME]["batch"], C.byref(job_out)) == 1
    S._sample(rig, job_out)
    L.check(lib, lib.rb_learner_pending_launched(ad.h))
    T.check_target("guard_pairs", TAU, t0, S.state(rig)["p"], T.target(rig), "guard run, pairs")
    guards(lib, m, "pair pass, tau = %g" % TAU)
    S.close_rig(rig)


def main(which):
    if which == "emu":
        from guarded_mem import GuardedNumpyMem as Mem
        from hipemu import loader
        lib = loader.load()
    else:
        from guarded_mem import GuardedTorchMem as Mem
        lib = L.load()
    T.declare(lib)
    hosted(lib, Mem)
    pairs(lib, Mem)
    print("guard run ok")


if __name__ == "__main__":
    main(sys.argv[1])
