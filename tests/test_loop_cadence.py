"""The cadence of rainbow_amd.loop (main.py:146-184 at S steps per round) without a GPU: train_device and train_host_vec are run
against recording fakes — an agent, a memory, a device-style environment on CPU tensors, host emulators behind a front end — that
log every call with its keyword arguments (learn() also logs the memory's priority_weight at that moment), and the whole trace is
compared with tests/golden/loop_cadence.json.

How the expected traces were made: `git show <parent>:rainbow_amd/loop.py` — the loop.py of the commit BEFORE the two training
loops were folded onto one cadence driver, where each loop still spelled the cadence out — was loaded as a module by a throwaway
script that called record_all() below with it and dumped the result as JSON.  They are never re-recorded from the code under
test; a cadence change on purpose records them again from a loop.py that was reviewed by hand.

S in {1, 2, 3} (3 divides none of the cadences), T_max = 13, learn_start = 5, replay_frequency = 4, target_update = 6,
evaluation_interval = 5, reward_clip = 1 against rewards of +-2.0 (the clip shows in the appended rewards), per_stream_noise both
ways.  One more case runs evaluate_host_vec: mode restored, the max_rounds error, the stream-major result."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rainbow_amd import loop

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_cadence.json")
T_MAX = 13


def _plain(x):
    """Tensors, arrays and numpy scalars as plain Python values (what JSON holds)."""
    if isinstance(x, torch.Tensor):
        return x.tolist()
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, (tuple, list)):
        return [_plain(v) for v in x]
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    return x


class Trace(list):
    def add(self, name, *args, **kw):
        self.append([name, _plain(args), _plain(kw)])


class FakeAgent:
    def __init__(self, trace, actions=3):
        self.trace, self.training, self.calls, self.actions = trace, False, 0, actions

    def train(self):
        self.training = True
        self.trace.add("agent.train")

    def eval(self):
        self.training = False
        self.trace.add("agent.eval")

    def reset_noise(self, *args, **kw):
        self.trace.add("agent.reset_noise", *args, **kw)

    def reset_noise_rows(self, *args, **kw):
        self.trace.add("agent.reset_noise_rows", *args, **kw)

    def act_batch(self, states, *args, **kw):
        self.trace.add("agent.act_batch", states, *args, **kw)
        n = int(states.shape[0])
        a = [(self.calls + 2 * i) % self.actions for i in range(n)]
        self.calls += 1
        return torch.tensor(a, dtype=torch.int32) if kw.get("device_out") else np.asarray(a, dtype=np.int64)

    def learn(self, mem, *args, **kw):
        self.trace.add("agent.learn", *args, priority_weight=mem.priority_weight, **kw)

    def update_target_net(self):
        self.trace.add("agent.update_target_net")


class FakeMemory:
    def __init__(self, trace, streams, priority_weight):
        self.trace, self.streams, self.priority_weight = trace, streams, priority_weight

    def append_streams(self, *args, **kw):
        self.trace.add("mem.append_streams", *args, **kw)


class FakeDeviceEnv:
    """S streams on CPU tensors; the state of stream s after t steps is [100 * s + t]; rewards alternate +2 / -2; stream s ends
    an episode every s + 2 steps."""
    reward_range = (-2.0, 2.0)

    def __init__(self, trace, streams):
        self.trace, self.streams, self.t, self.device = trace, streams, 0, torch.device("cpu")

    def _states(self):
        st = torch.tensor([[100.0 * s + self.t] for s in range(self.streams)])
        return st

    def reset(self):
        self.trace.add("env.reset")
        self.t = 0
        return self._states()[0] if self.streams == 1 else self._states()

    def step_device(self, actions):
        self.trace.add("env.step_device", actions)
        self.t += 1
        rewards = torch.tensor([2.0 if (self.t + s) % 2 else -2.0 for s in range(self.streams)])
        nonterminals = torch.tensor([0.0 if self.t % (s + 2) == 0 else 1.0 for s in range(self.streams)])
        return self._states(), rewards, nonterminals


class FakeEmu:
    """Host emulator s: writes a step counter into the screens; its game ends every `period` steps; with lose_life_at, the step of
    that number reports a lost life instead."""

    def __init__(self, trace, s, period, reward, lose_life_at=None):
        self.trace, self.s, self.period, self.reward, self.lose_life_at, self.t = trace, s, period, reward, lose_life_at, 0

    def reset(self, out_a):
        self.trace.add("emu%d.reset" % self.s)
        out_a[...] = 200 + self.s

    def step(self, action, out_a, out_b):
        self.trace.add("emu%d.step" % self.s, action)
        self.t += 1
        out_a[...] = self.t
        out_b[...] = self.t + 50
        life_lost = self.t == self.lose_life_at
        done = not life_lost and self.t % self.period == 0
        return 3, self.reward if self.t % 2 else -self.reward, done, life_lost


class FakeFront:
    RESET, LIFE_RESET = 8, 16

    def __init__(self, trace, streams):
        self.trace, self.streams, self.t = trace, streams, 0
        self.screens = np.zeros((streams, 2, 2, 2), dtype=np.uint8)

    def _states(self):
        return torch.tensor([[100.0 * s + self.t] for s in range(self.streams)])

    def reset_all(self):
        self.trace.add("front.reset_all", screens=self.screens[:, :, 0, 0])
        self.t = 0
        return self._states()

    def step(self, flags):
        self.trace.add("front.step", flags, screens=self.screens[:, :, 0, 0])
        self.t += 1
        return self._states()


def _args():
    return SimpleNamespace(seed=7, priority_weight=0.4, learn_start=5, replay_frequency=4, target_update=6, evaluation_interval=5,
                           reward_clip=1)


def run_train(loop_module, which, S, per_stream_noise):
    """The trace of loop_module.train_device / train_host_vec for S streams, ending in the value it returned."""
    trace = Trace()
    agent, args = FakeAgent(trace), _args()
    mem = FakeMemory(trace, S, args.priority_weight)

    def on_eval(T):
        trace.add("on_eval", T)
        agent.eval()

    if which == "train_device":
        learns = loop_module.train_device(agent, mem, FakeDeviceEnv(trace, S), args, T_MAX, on_eval=on_eval,
                                          per_stream_noise=per_stream_noise)
    else:
        emus = [FakeEmu(trace, s, period=s + 3, reward=2.0, lose_life_at=2 if s == 0 else None) for s in range(S)]
        learns = loop_module.train_host_vec(agent, mem, emus, FakeFront(trace, S), args, T_MAX, on_eval=on_eval,
                                            per_stream_noise=per_stream_noise)
    trace.add("returned", learns, priority_weight=mem.priority_weight, training=agent.training)
    return list(trace)


def run_evaluate_host_vec(loop_module):
    """evaluate_host_vec for 2 emulators with episodes of 2 and 3 steps, 3 episodes (quotas 2 and 1), from training mode: the
    trace, the result, and what a max_rounds too small for it raises and leaves behind."""
    def setup():
        trace = Trace()
        agent = FakeAgent(trace)
        agent.training = True
        emus = [FakeEmu(trace, 0, period=2, reward=1.5), FakeEmu(trace, 1, period=3, reward=0.25)]
        return trace, agent, emus, FakeFront(trace, 2)

    trace, agent, emus, front = setup()
    result = loop_module.evaluate_host_vec(agent, emus, front, 3, epsilon=0.05, seed=11)
    out = dict(trace=list(trace), result=_plain(result), training_after=agent.training)
    trace, agent, emus, front = setup()
    try:
        loop_module.evaluate_host_vec(agent, emus, front, 3, epsilon=0.05, seed=11, max_rounds=2)
        out["max_rounds_error"] = None
    except RuntimeError as e:
        out["max_rounds_error"] = str(e)
    out["max_rounds_trace_tail"], out["max_rounds_training_after"] = list(trace)[-2:], agent.training
    return out


TRAIN_CASES = [(which, S, psn) for which in ("train_device", "train_host_vec") for S in (1, 2, 3) for psn in (False, True)]


def _case_key(which, S, psn):
    return "%s/S=%d/per_stream_noise=%d" % (which, S, int(psn))


def record_all(loop_module):
    """Every expected value of this file, from `loop_module` (see the module docstring for which one that must be)."""
    out = {_case_key(*c): run_train(loop_module, *c) for c in TRAIN_CASES}
    out["evaluate_host_vec"] = run_evaluate_host_vec(loop_module)
    return json.loads(json.dumps(out))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("which,S,per_stream_noise", TRAIN_CASES)
def test_training_loop_trace(golden, which, S, per_stream_noise):
    got = json.loads(json.dumps(run_train(loop, which, S, per_stream_noise)))
    want = golden[_case_key(which, S, per_stream_noise)]
    assert len(want) > 4 * (T_MAX // S)                 # (a recorded trace, not an empty one)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d differs: got %r, recorded %r" % (i, g, w)
    assert len(got) == len(want)
    if not per_stream_noise and which == "train_device":
        assert all("per_row_noise" not in kw for name, _, kw in got if name == "agent.act_batch")


def test_evaluate_host_vec_with_fakes(golden):
    got = json.loads(json.dumps(run_evaluate_host_vec(loop)))
    want = golden["evaluate_host_vec"]
    assert got["training_after"] is True and got["max_rounds_training_after"] is True         # the mode it came in
    assert got["trace"][0][0] == "agent.eval" and got["trace"][-1][0] == "agent.train"
    assert got["max_rounds_error"] == "evaluate_host_vec: 2 of 3 episodes still unfinished after max_rounds = 2 rounds"
    # stream-major: stream 0's two episodes (2 steps: +1.5 - 1.5, then the same), then stream 1's one (3 steps: .25 - .25 + .25)
    assert got["result"]["rewards"] == [0.0, 0.0, 0.25] and got["result"]["lengths"] == [2, 2, 3]
    assert got == want
