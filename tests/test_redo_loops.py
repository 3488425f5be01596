"""args.redo_interval of rainbow_amd.loop without a GPU, on the recording fakes of test_loop_cadence.py: recycle_dormant is called on
the right gradient steps with the arguments args carries, a recycle that coincides with a full reset is skipped, a loop without
the argument never calls it (and its trace is the one it was before), and on_log's records gain the dormant share."""
import pytest

import test_loop_cadence as LC
from rainbow_amd import loop

T_MAX = 13
L_, R_, D_, A_ = "agent.learn", "agent.reset_parameters", "agent.recycle_dormant", "mem.append_streams"


class Agent(LC.FakeAgent):
    target_tau = 0.005
    fraction = None

    def reset_parameters(self, *args, **kw):
        self.trace.add("agent.reset_parameters", *args, **kw)

    def recycle_dormant(self, mem, *args, **kw):
        assert isinstance(mem, LC.FakeMemory)
        self.trace.add("agent.recycle_dormant", *args, **kw)
        self.fraction = 0.25 if self.fraction is None else self.fraction + 0.125

    def read_stats(self):
        return {"token": 1}

    def dormant_fraction(self):
        self.trace.add("agent.dormant_fraction")
        return self.fraction


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


def _calls(trace):
    return [name for name, _, _ in trace if name in (L_, R_, D_, A_)]


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_recycles_fall_on_the_right_gradient_steps(which):
    """S = 2, T_max = 13, learn_start = 5, replay_ratio 1.5: 15 learn steps in runs of three (the hand-made trace of
    test_param_reset_emu.py).  redo_interval = 4: a recycle right after learn 4, 8 and 12, with the defaults passed through."""
    trace, learns = _run(which, replay_ratio=1.5, redo_interval=4)
    want = [A_, A_,
            A_, L_, L_, L_,
            A_, L_, D_, L_, L_,
            A_, L_, L_, D_, L_,
            A_, L_, L_, L_, D_,
            A_, L_, L_, L_]
    assert _calls(trace) == want and learns == 15
    assert [(a, kw) for name, a, kw in trace if name == D_] == [([], dict(tau=None, batches=1, target=False))] * 3
    assert not any(name == R_ for name, _, _ in trace)


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_arguments_are_passed_through(which):
    trace, _ = _run(which, replay_ratio=1.5, redo_interval=5, redo_tau=0.025, redo_batches=3, redo_target=True)
    assert [kw for name, _a, kw in trace if name == D_] == [dict(tau=0.025, batches=3, target=True)] * 3


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_a_recycle_that_coincides_with_a_reset_is_skipped(which):
    """redo_interval = 3 and reset_interval = 6: learn 3, 9 and 15 recycle, learn 6 and 12 reset and do not recycle."""
    trace, learns = _run(which, replay_ratio=1.5, redo_interval=3, reset_interval=6)
    seen, after = 0, {}
    calls = _calls(trace)
    for i, name in enumerate(calls):
        if name == L_:
            seen += 1
            after[seen] = [c for c in calls[i + 1:i + 2] if c in (R_, D_)]
    assert learns == 15
    assert {k: v for k, v in after.items() if v} == {3: [D_], 6: [R_], 9: [D_], 12: [R_], 15: [D_]}
    assert calls.count(D_) == 3 and calls.count(R_) == 2
    for i, name in enumerate(calls):                                # never both behind one learn step
        if name in (R_, D_):
            assert calls[i - 1] == L_ and (i + 1 == len(calls) or calls[i + 1] not in (R_, D_))


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_no_call_without_the_argument(which):
    """Absent or 0: never, and the trace is the one of a loop that has never heard of it (redo_tau and its companions alone do
    nothing); the golden cadence of tests/golden/loop_cadence.json runs on an agent without recycle_dormant at all."""
    base, _ = _run(which, replay_ratio=1.5)
    for fields in (dict(redo_interval=0), dict(redo_interval=None), dict(redo_tau=0.1, redo_batches=2, redo_target=True)):
        trace, _ = _run(which, replay_ratio=1.5, **fields)
        assert list(trace) == list(base)
    assert not any(name in (D_, "agent.dormant_fraction") for name, _, _ in base)
    assert LC.run_train(loop, which, 2, False)[-1][0] == "returned"


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_on_log_records_gain_the_dormant_fraction(which):
    got = []
    trace, learns = _run(which, on_log=lambda T, rec: got.append(rec), replay_ratio=1.5, redo_interval=4, log_interval=2)
    assert len(got) == learns // 2 == 7
    # logs behind learn 2, 4, .., 14; recycles behind learn 4, 8, 12 (the log of the same step comes first)
    assert [r["dormant_fraction"] for r in got] == [None, None, 0.25, 0.25, 0.375, 0.375, 0.5]
    assert all(r["token"] == 1 for r in got)
    # without redo_interval the records are read_stats' own object, and dormant_fraction is never asked for
    got2 = []
    trace2, _ = _run(which, on_log=lambda T, rec: got2.append(rec), replay_ratio=1.5, log_interval=2)
    assert got2 == [{"token": 1}] * 7 and not any(name == "agent.dormant_fraction" for name, _, _ in trace2)
