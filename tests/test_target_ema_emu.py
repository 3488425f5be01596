"""The target network's EMA inside the optimiser pass on the host interpreter (tests/target_ema_scenarios.py has the rule, the
bounds and the forms), the host logic around it, the loops' cadence with an EMA target, and the gfx950 code of the new pending
kernel."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

import optimizer_scenarios as S
import target_ema_scenarios as T
from cabi_adapter import NumpyMem
from hipemu import loader
from rainbow_amd import _lib as L
from rainbow_amd import loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    yield T.declare(loader.load())
    out = os.environ.get("RB_OPTIMIZER_RATIOS")      # the observed error / bound table of profiles/optimizer_bounds.txt
    if out:
        with open(out, "a") as f:
            f.write(T.format_ratios("host interpreter"))


@pytest.mark.parametrize("n", T.PLAIN_SHAPES)
def test_rule_on_buffers_of_any_length(emu, n):
    T.plain_shapes_check(emu, NumpyMem, n)


def test_rule_in_the_pair_workgroups_around_a_hole(emu):
    T.pair_shapes_check(emu, NumpyMem)


def test_rule_in_every_form_of_the_small_layout(emu, monkeypatch):
    T.forms_check(emu, NumpyMem, monkeypatch)


def test_rule_in_the_pair_pass_flushed_and_hosted(emu, monkeypatch):
    T.pairs_check(emu, NumpyMem, monkeypatch)


def test_rule_behind_the_fused_tile_pass(emu):
    T.fused_tile_check(emu, NumpyMem)


@pytest.mark.parametrize("flags,hows", [(L.LEARNER_DEFER_UPDATE, ("hosted", "flush")), (0, ("value",)),
                                        (L.LEARNER_FUSE_FC_H_DW | L.LEARNER_WRITE_FUSED_GRADS, ("value",))],
                         ids=["deferred", "k_clip_adam", "fused-tile"])
def test_failed_draw_leaves_the_target_alone(emu, flags, hows):
    T.failed_draw_check(emu, NumpyMem, flags, hows)


# ------------------------------------------------------------------------------------------------------ host logic --
def test_tau_outside_the_unit_interval_is_refused_by_name(emu):
    rig = S.build_rig(emu, NumpyMem, "dataeff", False)
    t0 = T.target(rig)
    for fn in (emu.rb_learner_set_target_tau, emu.rb_learner_target_ema):
        for bad in (-0.1, 1.5, float("nan"), float("inf")):
            assert fn(rig.ad.h, bad, rig.mem.stream) != 0, bad
            assert b"tau" in emu.rb_last_error(), emu.rb_last_error()
    for ok in (0.0, 1.0, 0.005):
        L.check(emu, emu.rb_learner_set_target_tau(rig.ad.h, ok, rig.mem.stream))
    assert np.array_equal(T.target(rig), t0)
    S.close_rig(rig)


def test_set_target_tau_runs_a_pending_pass_with_the_old_tau(emu):
    lib = emu
    rig = S.build_rig(lib, NumpyMem, "dataeff", False, L.LEARNER_DEFER_UPDATE)
    m, ad = rig.mem, rig.ad
    g = S.make_grad(ad.layout, ad.n_params, 5, "scales")
    T.set_tau(rig, 0.5)
    for old, new in ((0.5, 0.005), (0.005, 0.0)):
        S._store(ad.grads, g)
        L.check(lib, lib.rb_learner_grads_modified(ad.h))
        S._store(rig.ctr, np.array([3], np.int64))
        before, t0 = S.state(rig), T.target(rig)
        S._clip_adam(rig, lib.rb_learner_clip_adam_deferred, 10.0, 0, m.ptr(rig.norm))
        S.same_state(before, S.state(rig), "the pass is pending")
        assert np.array_equal(T.target(rig), t0)
        T.set_tau(rig, new)                                         # runs the pending pass first: it carries the old tau
        after, t1 = S.state(rig), T.target(rig)
        assert not np.array_equal(after["p"], before["p"])
        T.check_target("set_tau", old, t0, after["p"], t1, "pending pass under tau %g, then set to %g" % (old, new))
        wrong = t0.astype(np.float64) + new * (after["p"].astype(np.float64) - t0)
        # (far outside any rounding: a thousand half-ulps of the largest target value)
        assert float(np.max(np.abs(t1 - wrong))) > 1e3 * T.U * float(np.max(np.abs(t1))), "the pass must not have used the new tau"
    # tau = 0 now: the next pass leaves the target alone
    S._store(ad.grads, g)
    L.check(lib, lib.rb_learner_grads_modified(ad.h))
    t0 = T.target(rig)
    S._clip_adam(rig, lib.rb_learner_clip_adam_deferred, 10.0, 0, m.ptr(rig.norm))
    L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
    assert np.array_equal(T.target(rig), t0)
    S.close_rig(rig)


def test_target_ema_entry_point_flushes_then_moves_the_target_once(emu):
    lib = emu
    rig = S.build_rig(lib, NumpyMem, "dataeff", False, L.LEARNER_DEFER_UPDATE)
    m, ad = rig.mem, rig.ad
    g = S.make_grad(ad.layout, ad.n_params, 6, "scales")
    for tau in T.TAUS:
        S._store(ad.grads, g)
        L.check(lib, lib.rb_learner_grads_modified(ad.h))
        S._store(rig.ctr, np.array([2], np.int64))
        before, t0 = S.state(rig), T.target(rig)
        S._clip_adam(rig, lib.rb_learner_clip_adam_deferred, 10.0, 0, m.ptr(rig.norm))
        L.check(lib, lib.rb_learner_target_ema(ad.h, tau, m.stream))
        after, t1 = S.state(rig), T.target(rig)
        assert not np.array_equal(after["p"], before["p"]), "the pending pass must have run first"
        T.check_target("target_ema", tau, t0, after["p"], t1, "rb_learner_target_ema")
        L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
        S.same_state(after, S.state(rig), "nothing was left pending")
    t0 = T.target(rig)
    L.check(lib, lib.rb_learner_target_ema(ad.h, 0.0, m.stream))
    assert np.array_equal(T.target(rig), t0)
    S.close_rig(rig)


# --------------------------------------------------------------------------------------------------- loop cadence --
@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
@pytest.mark.parametrize("S_", [1, 3])
def test_loops_skip_the_hard_sync_only_with_an_ema_target(which, S_, monkeypatch):
    import test_loop_cadence as LC
    with open(LC.GOLDEN) as f:
        want = json.load(f)[LC._case_key(which, S_, False)]
    assert any(name == "agent.update_target_net" for name, _, _ in want)

    def run(tau):
        class Agent(LC.FakeAgent):
            pass
        if tau is not None:
            Agent.target_tau = tau
        monkeypatch.setattr(LC, "FakeAgent", Agent)
        return json.loads(json.dumps(LC.run_train(loop, which, S_, False)))

    assert run(None) == want and run(0.0) == want                  # no attribute, or tau = 0: today's cadence, call for call
    got = run(0.005)
    assert got == [c for c in want if c[0] != "agent.update_target_net"]
    assert run(1.0) == got


# ------------------------------------------------------------------------------------------------------------ ISA --
def test_no_waterfall_block_in_the_pending_pass_with_ema():
    """k_adam_pending_ema is the hosted body with the EMA and nothing else (tests/test_hosted_pass_isa.py looks at the plain one):
    the target's quad loads (4 plain + 4 pair) and stores are there on top of the pass's own, and none sits in a waterfall loop."""
    from test_hosted_pass_isa import kernel_body, waterfall_blocks
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rainbow_amd", "csrc", "learner.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "learner.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                               src, "-o", out], stderr=subprocess.DEVNULL)
        body = kernel_body(out, "k_adam_pending_ema")
        plain = kernel_body(out, "k_adam_pending")
    assert body, "k_adam_pending_ema is not in the learner's unit"
    count = lambda b, pat: sum(bool(re.search(pat, ln)) for ln in b)
    loads, stores = count(body, r"\bbuffer_load_dwordx4\b"), count(body, r"\bbuffer_store_dwordx4\b")
    assert loads >= 16 + 14 + 4 + 4 and stores >= 12 + 14 + 4 + 4, ("the target's quad accesses must be there to be judged", loads, stores)
    assert loads >= count(plain, r"\bbuffer_load_dwordx4\b") + 8 and stores >= count(plain, r"\bbuffer_store_dwordx4\b") + 8
    assert waterfall_blocks(body) == []
    assert not any(re.search(r"\bscratch_|\bflat_(load|store)", ln) for ln in body)
