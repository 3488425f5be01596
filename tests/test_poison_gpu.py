"""Read-before-write hunt on the MI355X: every group of tests/poison_run.py — every row of the batch ladder, the shape-range, head
and exchange tables, the replay goldens and scenario bodies, the env bodies — once on zero-filled allocations (RB_GUARD=1) and once
on allocations left at the poison byte 0xC5 (RB_GUARD=2), as tests/test_poison_emu.py does on the host interpreter (its docstring
has the method and what the first run found).  One child process at a time; the second is not started if the first failed; nothing
is retried.  A fresh process on the device gets fresh pages from the driver, which read as zero, and ensure_rows /
ensure_rows_scaled hand recycled memory to the forward buffers in a long-lived process: the poison is the only configuration in
which a sweep of one slice too many, or a pad column with a weight, reads something else than 0.0.

First run on the MI355X, after the grads_dev fix the host interpreter run led to: every group identical, no band overwritten.

Measured on the MI355X, per test (pytest call time of the pair; in brackets what one child spends inside its group, the rest being
two interpreter starts with torch and the library each):
  control 4.7 s          learn-small 8.3 s         learn-head 8.2 s [2.0]       learn-range-narrow 9.1 s [2.1]
  learn-range-wide-b4 14.1 s [4.1]                 learn-range-wide-batch 24.6 s [9.1]
  learn-ladder-a 12.6 s [3.6]   -b 11.7 s [3.3]    -c 11.3 s [3.3]              -opts 12.5 s [3.3]
  exchange-finish 8.8 s [2.3]   exchange-learn 8.9 s [2.4]
  replay-golden 8.4 s [2.3]     replay-streams 13.0 s [4.7]     replay-shift 5.6 s [0.8]
  envs-obs 9.8 s [3.0]          envs-breakout 9.6 s [6.4 / 2.7]              envs-eval 7.8 s [1.8]
Against the parity tests of the same tables in the same suite run: those take 0.2 to 1.5 s of call time per row (ladder b1024
1.5 s, shape-range c-b33-h2176 1.0 s, most rows 0.2 to 0.4 s), 5 to 10 s per table, in ONE process that is already up.  The time
inside a child is at or below that (no oracle runs; the wide shape-range rows spend theirs on generating and digesting 19 M to
27 M parameters four times per step), but the test as a whole is not: the two fresh processes a pair needs cost 5 to 6 s before
the first kernel.  The group split keeps each pair near ten seconds; rows were not dropped to get there."""
import pytest

import poison_pair as PP

pytestmark = pytest.mark.gpu

GROUPS = ["learn-small", "learn-ladder-a", "learn-ladder-b", "learn-ladder-c", "learn-ladder-opts", "learn-range-narrow",
          "learn-range-wide-b4", "learn-range-wide-batch", "learn-head", "exchange-finish", "exchange-learn", "replay-golden", "replay-streams", "replay-shift",
          "envs-obs", "envs-breakout", "envs-eval"]


def test_control_a_fresh_library_block_is_poison_under_2_and_zero_under_1_on_device(tmp_path):
    """rb_learner_debug_read of m before any learn call (poison_run.run_control asserts the bytes per level): the hook is live, and
    the comparison below does see memory nobody wrote."""
    zeroed = PP.run_child("hip", "control", 1, tmp_path, timeout=300)
    poisoned = PP.run_child("hip", "control", 2, tmp_path, timeout=300)
    assert zeroed["control"] == dict(m_bytes=[0x00]) and poisoned["control"] == dict(m_bytes=[0xC5])
    assert zeroed["guards"][0]["lib_blocks"] > 0 and poisoned["guards"][0]["lib_blocks"] == zeroed["guards"][0]["lib_blocks"]


@pytest.mark.parametrize("group", GROUPS)
def test_outputs_do_not_depend_on_what_fresh_memory_holds_on_device(tmp_path, group):
    PP.run_pair("hip", group, tmp_path, timeout=600)
