"""Read-before-write hunt on the host interpreter: every group of tests/poison_run.py that the interpreter gets through, once on
zero-filled allocations (RB_GUARD=1) and once on allocations left at the poison byte 0xC5 (RB_GUARD=2: the library's own blocks,
include/rainbow_hip.h rb_debug_check_guards, and every caller-owned buffer, guarded_mem.Poisoned*Mem), each in a child process
(RB_GUARD is read when the library first allocates).  Per child: exit 0, no guard band overwritten.  Across the pair: the digests
of every named output identical, key by key (poison_pair.same_digests names the tensors that are not).  The interpreter's
hipMalloc is calloc, the device's fresh pages read as zero, and every Mem class of the suite hands out zeros — without the
poison no test here or on the device ever gives a kernel memory that is not zero.

What it found when first run, at atoms21 (hidden 48: no multiple of 32, so the learn call leaves no norm partials; the route of
d-h1, d-h3 and the h48 head rows, and of every gradient a caller has modified): the gradient norm of that route
(optimizer_host.h sumsq_pass: k_sumsq over the whole flat gradient) squares the alignment padding between the tensors of the
CALLER's grads_dev, which no kernel writes: 0.6759 on zeros, 85 846.95 on poison, and with it the clip factor of every gradient
and everything downstream (the unclipped gradients were identical).  Poisoning the library's blocks alone changed nothing.
rb_learner_create now zero-fills grads_dev and the header says so.

Measured wall times of the PAIR (pytest call time, this file on six workers of an 8-core host): learn-range 1083 s, learn-head
842 s, learn-small 312 s (canon, the one-step canonical row, is 84 s of each child), envs-eval 96 s, envs-obs 70 s,
replay-streams 53 s, envs-breakout 35 s, replay-golden 29 s, replay-shift 17 s, control 4 s; the run-to-run test (learn-k10
twice) 44 s."""
import pytest

import poison_pair as PP

GROUPS = ["learn-small", "learn-range", "learn-head", "replay-golden", "replay-streams", "replay-shift", "envs-obs", "envs-breakout",
          "envs-eval"]


def test_control_a_fresh_library_block_is_poison_under_2_and_zero_under_1(tmp_path):
    """rb_learner_debug_read of m before any learn call (poison_run.run_control asserts the bytes per level): the hook is live, and
    the comparison below does see memory nobody wrote."""
    zeroed = PP.run_child("emu", "control", 1, tmp_path, timeout=600)
    poisoned = PP.run_child("emu", "control", 2, tmp_path, timeout=600)
    assert zeroed["control"] == dict(m_bytes=[0x00]) and poisoned["control"] == dict(m_bytes=[0xC5])
    assert zeroed["guards"][0]["lib_blocks"] > 0 and poisoned["guards"][0]["lib_blocks"] == zeroed["guards"][0]["lib_blocks"]


@pytest.mark.parametrize("group", GROUPS)
def test_outputs_do_not_depend_on_what_fresh_memory_holds(tmp_path, group):
    PP.run_pair("emu", group, tmp_path, timeout=3000)


def test_digests_are_stable_from_run_to_run(tmp_path):
    """The same level twice: what the pair comparison rests on."""
    a = PP.run_child("emu", "learn-k10", 1, tmp_path, timeout=900)
    b = PP.run_child("emu", "learn-k10", 1, tmp_path, timeout=900)
    PP.same_digests(a, b, "emu learn-k10, RB_GUARD=1 twice")
