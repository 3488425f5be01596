"""on_log / args.log_interval of rainbow_amd.loop without a GPU, on the recording fakes of test_loop_cadence.py: the callback
fires right after every log_interval-th learn step with what agent.read_stats() returned, a loop that is given no on_log makes
exactly the calls it made before (read_stats is never touched, log_interval or not), and _evaluation_result reports the
held-out loss only when asked to."""
from types import SimpleNamespace

import pytest

from rainbow_amd import loop
from test_loop_cadence import FakeAgent, FakeDeviceEnv, FakeEmu, FakeFront, FakeMemory, Trace, _args, run_train

T_MAX = 40


class LoggingAgent(FakeAgent):
    reads = 0

    def read_stats(self):
        self.reads += 1
        self.trace.add("agent.read_stats")
        return {"token": self.reads}


def _run(which, S, args, on_log):
    trace = Trace()
    agent = LoggingAgent(trace)
    mem = FakeMemory(trace, S, args.priority_weight)
    if which == "train_device":
        learns = loop.train_device(agent, mem, FakeDeviceEnv(trace, S), args, T_MAX, on_log=on_log(trace) if on_log else None)
    else:
        emus = [FakeEmu(trace, s, period=s + 3, reward=2.0) for s in range(S)]
        learns = loop.train_host_vec(agent, mem, emus, FakeFront(trace, S), args, T_MAX, on_log=on_log(trace) if on_log else None)
    return trace, agent, learns


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
@pytest.mark.parametrize("S, replay_ratio, interval", [(1, 0, 3), (3, 0, 2), (2, 1.5, 4), (3, 0, 1)])
def test_on_log_fires_every_log_interval_learn_steps(which, S, replay_ratio, interval):
    args = _args()
    args.log_interval, args.replay_ratio = interval, replay_ratio
    got = []

    def on_log(trace):
        def cb(T, records):
            trace.add("on_log", T)
            got.append((T, records))
        return cb

    trace, agent, learns = _run(which, S, args, on_log)
    names = [e[0] for e in trace]
    assert learns == names.count("agent.learn") and learns >= 2 * interval
    assert len(got) == learns // interval == agent.reads
    assert [r["token"] for _T, r in got] == list(range(1, len(got) + 1))          # what read_stats returned, in order
    # each call sits right behind the learn step that made the count a multiple of the interval: read_stats, then on_log
    seen = 0
    for i, name in enumerate(names):
        if name == "agent.learn":
            seen += 1
            follows = names[i + 1:i + 3] == ["agent.read_stats", "on_log"]
            assert follows == (seen % interval == 0), (seen, names[i + 1:i + 3])
    assert [T for T, _r in got] == sorted(T for T, _r in got) and all(args.learn_start <= T <= T_MAX + S for T, _r in got)


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_without_on_log_nothing_changes(which):
    """No on_log: the trace is the one of a loop that has never heard of log_interval, whether args carries one or not."""
    plain = _args()
    with_interval = _args()
    with_interval.log_interval = 1
    a, agent_a, _ = _run(which, 2, plain, None)
    b, agent_b, _ = _run(which, 2, with_interval, None)
    assert list(a) == list(b) and agent_a.reads == agent_b.reads == 0
    assert "agent.read_stats" not in [e[0] for e in a]
    # ... and on_log with log_interval absent or 0 never fires either
    for iv in (None, 0):
        args = _args()
        if iv is not None:
            args.log_interval = iv
        c, agent_c, _ = _run(which, 2, args, lambda trace: (lambda T, r: trace.add("on_log", T)))
        assert list(c) == list(a) and agent_c.reads == 0


def test_golden_cadence_is_untouched_by_the_new_argument():
    """run_train of test_loop_cadence.py (no on_log) on an agent WITHOUT read_stats: the loops must not need it."""
    assert run_train(loop, "train_device", 2, False)[-1][0] == "returned"


def test_evaluation_result_reports_the_held_out_loss_only_on_request():
    calls = []
    agent = SimpleNamespace(evaluate_q_memory=lambda mem: [1.0, 3.0],
                            evaluate_loss=lambda mem: calls.append(mem) or dict(loss_mean=0.25, td_abs_mean=0.5, q_mean=9.0))
    base = loop._evaluation_result(agent, [1.0, 2.0], [3, 4], "val")
    assert calls == [] and set(base) == {"avg_reward", "rewards", "lengths", "avg_Q", "Qs"} and base["avg_Q"] == 2.0
    assert loop._evaluation_result(agent, [1.0, 2.0], [3, 4], None, with_loss=True) == dict(base, avg_Q=None, Qs=None)
    full = loop._evaluation_result(agent, [1.0, 2.0], [3, 4], "val", with_loss=True)
    assert calls == ["val"] and full == dict(base, val_loss=0.25, val_td_abs=0.5)
