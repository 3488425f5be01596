"""args.rank_interval of rainbow_amd.loop without a GPU, on the recording fakes of test_loop_cadence.py: feature_rank is called on the
right gradient steps with the arguments args carries, before the log, the reset and the recycle of the same step; a loop without the
argument never calls it (and its trace is the one it was before); on_log's records gain the three ranks."""
import pytest

import test_loop_cadence as LC
from rainbow_amd import loop

T_MAX = 13
L_, R_, D_, K_, A_ = "agent.learn", "agent.reset_parameters", "agent.recycle_dormant", "agent.feature_rank", "mem.append_streams"


class Agent(LC.FakeAgent):
    target_tau = 0.005
    measured = 0

    def reset_parameters(self, *args, **kw):
        self.trace.add(R_, *args, **kw)

    def recycle_dormant(self, mem, *args, **kw):
        assert isinstance(mem, LC.FakeMemory)
        self.trace.add(D_, *args, **kw)

    def dormant_fraction(self):
        return None

    def feature_rank(self, mem, *args, **kw):
        assert isinstance(mem, LC.FakeMemory)
        self.trace.add(K_, *args, **kw)
        self.measured += 1
        return dict(srank=10 - self.measured, feature_rank=20 - self.measured, effective_rank=7.5 - self.measured, samples=64)

    def read_stats(self):
        self.trace.add("agent.read_stats")
        return {"token": 1}


def _run(which, on_log=None, **fields):
    args = LC._args()
    for k, v in fields.items():
        setattr(args, k, v)
    S = 2
    trace = LC.Trace()
    agent, mem = Agent(trace), LC.FakeMemory(trace, S, args.priority_weight)
    if which == "train_device":
        learns = loop.train_device(agent, mem, LC.FakeDeviceEnv(trace, S), args, T_MAX, on_log=on_log)
    else:
        emus = [LC.FakeEmu(trace, s, period=s + 3, reward=2.0) for s in range(S)]
        learns = loop.train_host_vec(agent, mem, emus, LC.FakeFront(trace, S), args, T_MAX, on_log=on_log)
    return trace, learns


def _calls(trace, extra=()):
    return [name for name, _, _ in trace if name in (L_, R_, D_, K_, A_) + tuple(extra)]


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_measurements_fall_on_the_right_gradient_steps(which):
    """S = 2, T_max = 13, learn_start = 5, replay_ratio 1.5: 15 learn steps in runs of three (the hand-made trace of
    test_redo_loops.py).  rank_interval = 4: a measurement right after learn 4, 8 and 12, with the defaults passed through."""
    trace, learns = _run(which, replay_ratio=1.5, rank_interval=4)
    want = [A_, A_,
            A_, L_, L_, L_,
            A_, L_, K_, L_, L_,
            A_, L_, L_, K_, L_,
            A_, L_, L_, L_, K_,
            A_, L_, L_, L_]
    assert _calls(trace) == want and learns == 15
    assert [(a, kw) for name, a, kw in trace if name == K_] == [([], dict(batches=8, layer="hidden"))] * 3


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_arguments_are_passed_through(which):
    trace, _ = _run(which, replay_ratio=1.5, rank_interval=5, rank_batches=3, rank_layer="conv")
    assert [kw for name, _a, kw in trace if name == K_] == [dict(batches=3, layer="conv")] * 3


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_the_measurement_comes_before_the_log_the_reset_and_the_recycle(which):
    """rank_interval = 3 with reset_interval = 6, redo_interval = 3 and log_interval = 3: behind learn 3, 9 and 15 the order is
    measurement, log, recycle; behind learn 6 and 12 measurement, log, reset."""
    trace, learns = _run(which, on_log=lambda T, rec: None, replay_ratio=1.5, rank_interval=3, reset_interval=6, redo_interval=3,
                         log_interval=3)
    calls = _calls(trace, extra=("agent.read_stats",))
    seen, after = 0, {}
    for name in calls:                                                 # what follows each learn step, up to the next learn or append
        if name == L_:
            seen += 1
            after[seen] = []
        elif name != A_ and seen:
            after[seen].append(name)
    assert learns == 15
    log = "agent.read_stats"
    assert {k: v for k, v in after.items() if v} == {3: [K_, log, D_], 6: [K_, log, R_], 9: [K_, log, D_], 12: [K_, log, R_],
                                                     15: [K_, log, D_]}


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_no_call_without_the_argument(which):
    """Absent or 0: never, and the trace is the one of a loop that has never heard of it (rank_batches and rank_layer alone do
    nothing); the golden cadence of tests/golden/loop_cadence.json runs on an agent without feature_rank at all."""
    base, _ = _run(which, replay_ratio=1.5)
    for fields in (dict(rank_interval=0), dict(rank_interval=None), dict(rank_batches=2, rank_layer="conv")):
        trace, _ = _run(which, replay_ratio=1.5, **fields)
        assert list(trace) == list(base)
    assert not any(name == K_ for name, _, _ in base)
    assert LC.run_train(loop, which, 2, False)[-1][0] == "returned"


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_on_log_records_gain_the_ranks(which):
    got = []
    trace, learns = _run(which, on_log=lambda T, rec: got.append(rec), replay_ratio=1.5, rank_interval=4, log_interval=2)
    assert len(got) == learns // 2 == 7
    # logs behind learn 2, 4, .., 14; measurements behind learn 4, 8, 12 — the log of the same step already shows them
    assert [r["srank"] for r in got] == [None, 9, 9, 8, 8, 7, 7]
    assert [r["feature_rank"] for r in got] == [None, 19, 19, 18, 18, 17, 17]
    assert [r["effective_rank"] for r in got] == [None, 6.5, 6.5, 5.5, 5.5, 4.5, 4.5]
    assert all(r["token"] == 1 and "dormant_fraction" not in r for r in got)
    # without rank_interval the records are read_stats' own object
    got2 = []
    _run(which, on_log=lambda T, rec: got2.append(rec), replay_ratio=1.5, log_interval=2)
    assert got2 == [{"token": 1}] * 7
