"""The annealed update horizon and discount (rb_replay_set_horizon / rb_learner_set_horizon) on the host interpreter: the SAME
kernel sources as librainbow_hip.so against the oracle replay and the oracle learner (tests/horizon_scenarios.py has the tables and
the bodies; the device runs every row in test_horizon_gpu.py), and — no kernel involved — the schedule: rainbow_amd.loop.horizon_at
against a hand-written table and _train_rounds' set_horizon calls against recording stubs."""
import math
import types

import pytest

import horizon_scenarios as HZ
from cabi_adapter import NumpyMem
from guarded_mem import GuardedNumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


# =============================================================================== A. replay
@pytest.mark.parametrize("row", HZ.A1_EMU_ROWS, ids=HZ.a1_id)
def test_batch_at_n_eff_is_the_oracle_built_with_n_eff(emu, row):
    HZ.check_table_row(emu, NumpyMem(), row)


def test_episode_ends_inside_at_and_beyond_the_horizon(emu):
    HZ.check_episode_ends(emu, NumpyMem())


@pytest.mark.parametrize("streams,cap", [(1, 96), (3, 192)], ids=["S1", "S3"])
def test_write_head_rule_follows_the_horizon(emu, streams, cap):
    HZ.check_write_head(emu, GuardedNumpyMem(), S=streams, cap=cap)


def test_rejection_loop_and_weights_under_random_priorities(emu):
    HZ.check_random_priorities(emu, NumpyMem())


def test_horizon_changes_on_a_live_replay(emu):
    HZ.check_live_change(emu, NumpyMem())


def test_refusals_name_the_argument_and_leave_the_replay_working(emu):
    HZ.check_refusals(emu, NumpyMem())


# =============================================================================== B. learner
def test_learner_refusals(emu):
    HZ.check_learner_refusals(emu, NumpyMem())


def test_two_learn_steps_under_two_horizons_match_the_oracle(emu):
    HZ.check_learn(emu, NumpyMem(), "dataeff-b4-h32", where="emu")


def test_train_step_refuses_mismatched_horizons(emu):
    HZ.check_train_step_mismatch(emu, NumpyMem)


def test_train_step_follows_the_horizon(emu, monkeypatch):
    HZ.check_train_step(emu, NumpyMem, monkeypatch, spec=False)


def test_early_draw_made_under_the_old_horizon_is_discarded(emu, monkeypatch):
    HZ.check_train_step(emu, NumpyMem, monkeypatch, spec=True)


# =============================================================================== D. the schedule (no kernel)
def test_horizon_at_matches_the_hand_written_table():
    """BBF's schedule 10 -> 3, 0.97 -> 0.997 over T = 10 000.  The table is written out here from the closed forms with `math`
    alone: n = floor(10 * 0.3 ** f + 0.5), gamma = 1 - 0.03 * 0.1 ** f, f = min(t, T) / T."""
    from rainbow_amd.loop import horizon_at
    table = {
        0: (10, 0.97),                                                           # f = 0
        1: (10, 1 - 0.03 * math.exp(math.log(0.1) * 1e-4)),                      # 10 * 0.3^1e-4 = 9.9988: still 10
        2500: (7, 1 - 0.03 * 0.1 ** 0.25),                                       # 10 * 0.3^0.25 = 7.4008
        5000: (5, 1 - 0.03 * math.sqrt(0.1)),                                    # 10 * sqrt(0.3) = 5.4772
        9999: (3, 1 - 0.03 * math.exp(math.log(0.1) * 0.9999)),                  # 10 * 0.3^0.9999 = 3.00036
        10000: (3, 0.997),
        20000: (3, 0.997),                                                       # past T: the end values stay
    }
    assert math.floor(10 * math.exp(0.25 * math.log(0.3)) + 0.5) == 7 and math.floor(10 * math.sqrt(0.3) + 0.5) == 5
    for t, (n, g) in table.items():
        got_n, got_g = horizon_at(t, 10, 3, 0.97, 0.997, 10000)
        assert got_n == n and isinstance(got_n, int), (t, got_n, n)
        assert got_g == pytest.approx(g, rel=0, abs=1e-15), (t, got_g, g)
    assert horizon_at(0, 10, 3, 0.97, 0.997, 10000)[1] == pytest.approx(0.97, abs=1e-15)
    # a fixed discount comes back as it went in, bit for bit, and a fixed horizon stays
    assert horizon_at(1234, 10, 3, 0.99, 0.99, 10000)[1] == 0.99
    assert [horizon_at(t, 5, 5, 0.9, 0.99, 100)[0] for t in (0, 50, 100, 500)] == [5, 5, 5, 5]
    # every horizon from 10 down to 3 is visited, never upwards
    ns = [horizon_at(t, 10, 3, 0.97, 0.997, 10000)[0] for t in range(0, 10001, 50)]
    assert sorted(set(ns)) == list(range(3, 11)) and all(a >= b for a, b in zip(ns, ns[1:]))


class _Recorder:
    def __init__(self):
        self.log = []


def _stub_agent(rec):
    return types.SimpleNamespace(
        learn=lambda mem: rec.log.append(("learn",)), reset_parameters=lambda: rec.log.append(("reset",)),
        set_horizon=lambda n, g=None: rec.log.append(("agent", n, g)), reset_noise=lambda: None, train=lambda: None,
        update_target_net=lambda: None, target_tau=0.0)


def _stub_mem(rec):
    return types.SimpleNamespace(priority_weight=0.4, set_horizon=lambda n, g=None: rec.log.append(("mem", n, g)))


def _loop_args(**kw):
    base = dict(seed=0, priority_weight=0.4, learn_start=1, replay_frequency=4, target_update=10 ** 9, evaluation_interval=0,
                replay_ratio=2, reset_interval=250, multi_step=10, discount=0.97)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_train_rounds_sets_the_horizon_at_the_stated_steps():
    """reset_interval 250, horizon_anneal_steps 200, horizon_update_interval 50, replay_ratio 2: set_horizon on agent and memory
    (in that order, the same pair) before the first learn step, before the learn steps number 50, 100, 150 and 200 of every reset
    period (t = 200 is both a multiple of the interval and the end of the anneal: one call), never between 200 and the reset, and
    right after each reset_parameters() with t back at 0 — not a second time before the next learn step."""
    from rainbow_amd.loop import _train_rounds, horizon_at
    rec = _Recorder()
    args = _loop_args(multi_step_final=3, discount_final=0.997, horizon_anneal_steps=200, horizon_update_interval=50)
    learns = _train_rounds(_stub_agent(rec), _stub_mem(rec), 1, args, 300, None, False, None, lambda s: s)
    assert learns == 600
    want = []
    for period in range(3):
        n_learn = 250 if period < 2 else 100
        for t in range(n_learn):
            if t in (50, 100, 150, 200) or (t == 0 and period == 0):
                pair = horizon_at(t, 10, 3, 0.97, 0.997, 200)
                want += [("agent",) + pair, ("mem",) + pair]
            want.append(("learn",))
        if period < 2:
            pair = horizon_at(0, 10, 3, 0.97, 0.997, 200)
            want += [("reset",), ("agent",) + pair, ("mem",) + pair]
    assert rec.log == want
    assert rec.log[0] == ("agent", 10, 0.97) and ("agent", 3, 0.997) in rec.log


def test_train_rounds_without_a_final_horizon_never_calls_set_horizon():
    from rainbow_amd.loop import _train_rounds
    rec = _Recorder()
    _train_rounds(_stub_agent(rec), _stub_mem(rec), 1, _loop_args(), 300, None, False, None, lambda s: s)
    assert [e[0] for e in rec.log if e[0] in ("agent", "mem")] == []
    assert rec.log.count(("learn",)) == 600 and rec.log.count(("reset",)) == 2


def test_train_rounds_keeps_the_discount_without_discount_final_and_refuses_a_growing_horizon():
    from rainbow_amd.loop import _train_rounds
    rec = _Recorder()
    args = _loop_args(multi_step_final=3, horizon_anneal_steps=200, horizon_update_interval=50, reset_interval=0)
    _train_rounds(_stub_agent(rec), _stub_mem(rec), 1, args, 150, None, False, None, lambda s: s)
    calls = [e for e in rec.log if e[0] == "agent"]
    assert [c[1] for c in calls] == [10, 7, 5, 4, 3] and all(c[2] == 0.97 for c in calls)
    with pytest.raises(ValueError, match="multi_step_final"):
        _train_rounds(_stub_agent(rec), _stub_mem(rec), 1, _loop_args(multi_step_final=11), 10, None, False, None, lambda s: s)
