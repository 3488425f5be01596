"""The S-stream observation front end on the MI355X: the host-interpreter checks of test_obs_stack_emu.py on the device, and
the Python surface — rainbow_amd.frames.FrameStackVec against the deque oracle, a replay fed through it against one fed
through FramePreprocessor.observe + torch stacking, and rainbow_amd.loop.train_host_vec on a fake host emulator."""
import types

import numpy as np
import pytest
import torch

import obs_stack_oracle as OO
import obs_stack_scenarios as OS
from cabi_adapter import TorchMem
from guarded_mem import GuardedTorchMem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


# ------------------------------------------------------------------ the emulator's checks on the device
@pytest.mark.parametrize("S", [1, 3, 64])
@pytest.mark.parametrize("history", [1, 4])
def test_scripted_rounds_match_the_deque_oracle_on_device(hip, S, history):
    OS.check_scripted(hip, TorchMem(), S, history, seed=3)


def test_scripted_rounds_at_the_longest_history_on_device(hip):
    OS.check_scripted(hip, TorchMem(), 2, 16, seed=4)


def test_scripted_rounds_on_another_screen_geometry_on_device(hip):
    OS.check_scripted(hip, TorchMem(), 3, 4, H=97, W=131, seed=5)


def test_newest_frame_is_frame_preprocess_on_device(hip):
    OS.check_newest_frame_equals_frame_preprocess(hip, TorchMem())


def test_null_frame_pointers_on_device(hip):
    OS.check_null_frames(hip, TorchMem())


def test_refusals_on_device(hip):
    OS.check_refusals(hip, TorchMem())


def test_scripted_rounds_between_guard_bands_on_device(hip):
    OS.check_guarded(hip, GuardedTorchMem())


# ------------------------------------------------------------------ FrameStackVec
@pytest.mark.parametrize("S", [3, 64])
def test_frame_stack_vec_matches_the_oracle(S):
    """30 rounds; the next staging view is overwritten with other bytes as soon as step() has returned; the stack handed out in
    round k is still intact after round k + 1."""
    from rainbow_amd.frames import FrameStackVec
    front = FrameStackVec(S, DEV)
    assert (front.STEP, front.RESET, front.LIFE_RESET) == (6, 3, 2) and (front.BLANK, front.FRAME_A, front.FRAME_B) == (1, 2, 4)
    ora = OO.StackOracle(S, 4)
    rs = np.random.RandomState(40 + S)
    script = OS.build_script(S, 9)[:30]
    first = OS.make_screens(rs, S, 210, 160)
    got = front.reset_all(first)                                   # [S, H, W]: single-frame round
    front.screens[...] = 0xEE
    want = ora.apply([OO.RESET] * S, first, None)
    assert tuple(got.shape) == (S, 4, 84, 84) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)
    prev, prev_want = got, want
    for r in range(30):
        a, b = OS.make_screens(rs, S, 210, 160), OS.make_screens(rs, S, 210, 160)
        if r % 3 == 0:
            got = front.step(script[r], torch.from_numpy(np.stack([a, b], 1)))      # a CPU tensor [S, 2, H, W]
        elif r % 3 == 1:
            got = front.step(script[r], np.stack([a, b], 1))
        else:
            view = front.screens                                   # what an emulator does: write into the slot
            assert view.shape == (S, 2, 210, 160) and view[S - 1, 1].flags["C_CONTIGUOUS"]
            view[:, 0], view[:, 1] = a, b
            got = front.step(script[r])
        front.screens[...] = rs.randint(0, 256, dtype=np.uint8)    # at once, before anything waited for the device
        want = ora.apply(script[r], a, b)
        assert np.array_equal(got.cpu().numpy(), want), r
        assert np.array_equal(prev.cpu().numpy(), prev_want), r    # round r - 1's stack outlives round r
        assert got.data_ptr() != prev.data_ptr()
        prev, prev_want = got, want


def test_frame_stack_vec_single_stream_shape_and_errors():
    from rainbow_amd import _lib as L
    from rainbow_amd.frames import FrameStackVec
    front = FrameStackVec(1, DEV, history_length=2, height=97, width=131)
    scr = OS.make_screens(np.random.RandomState(1), 1, 97, 131)
    out = front.reset_all(scr)
    assert tuple(out.shape) == (1, 2, 84, 84)
    assert np.array_equal(out.cpu().numpy(), OO.StackOracle(1, 2).apply([OO.RESET], scr, None))
    with pytest.raises(L.RainbowError, match="above 7"):
        front.step(9)
    with pytest.raises(TypeError):
        front.step(front.STEP, scr.astype(np.float32))
    with pytest.raises(ValueError):
        front.step(front.STEP, scr[:, :50])
    with pytest.raises(ValueError):
        FrameStackVec(65, DEV)
    with pytest.raises(RuntimeError):
        FrameStackVec(1, "cpu")


def _mem_args(**kw):
    base = dict(device=torch.device(DEV), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _same_replay(a, b):
    torch.cuda.synchronize()
    for k in ("frames", "timestep", "action", "reward", "nonterminal", "tree"):
        assert np.array_equal(a._grab(k), b._grab(k)), k


def test_replay_fed_by_frame_stack_vec_equals_the_existing_route():
    """Two S = 4 replays of 256 slots, 80 rounds (the ring wraps): FrameStackVec + append_streams against
    FramePreprocessor.observe with the stacks rolled and blanked by torch ops, same screens and events."""
    from rainbow_amd.frames import FramePreprocessor, FrameStackVec
    from rainbow_amd.memory import ReplayMemory
    S, cap, rounds = 4, 256, 80
    new, old = (ReplayMemory(_mem_args(), cap, seed=2, streams=S) for _ in range(2))
    front, pre = FrameStackVec(S, DEV), FramePreprocessor(DEV)
    rs = np.random.RandomState(12)
    events = rs.choice([OO.STEP, OO.STEP, OO.STEP, OO.STEP, OO.RESET, OO.LIFE_RESET, 0], size=(rounds + 1, S)).astype(np.uint8)
    events[0] = OO.RESET
    first = OS.make_screens(rs, S, 210, 160)
    states_new = front.reset_all(first)
    states_old = torch.zeros(S, 4, 84, 84, device=DEV)
    states_old[:, -1] = pre.observe(first)
    for r in range(1, rounds + 1):
        a, b = OS.make_screens(rs, S, 210, 160), OS.make_screens(rs, S, 210, 160)
        fl = events[r]
        actions, rewards = rs.randint(0, 6, S), rs.choice([-1.0, 0.0, 1.0], size=S).astype(np.float32)
        terminals = (fl == OO.RESET) | (fl == OO.LIFE_RESET)       # the stream's next stack starts an episode
        new.append_streams(states_new, actions, rewards, terminals)
        old.append_streams(states_old, actions, rewards, terminals)
        states_new = front.step(fl, np.stack([a, b], 1))
        f = torch.from_numpy(fl.astype(np.int64)).to(DEV)[:, None, None]
        both, only_a = pre.observe(a, b), pre.observe(a)
        obs = torch.where(f == OO.STEP, both, torch.where((f & OO.FRAME_A) != 0, only_a, torch.zeros_like(both)))
        rolled = torch.cat([states_old[:, 1:], obs[:, None]], dim=1)
        rolled[:, :-1] = torch.where((f & OO.BLANK)[:, None] != 0, torch.zeros_like(rolled[:, :-1]), rolled[:, :-1])
        states_old = rolled.contiguous()
        assert torch.equal(states_new, states_old), r
    _same_replay(new, old)
    assert new._header().full == 1


# ------------------------------------------------------------------ train_host_vec on a fake emulator
class FakeEmu:
    """A deterministic stand-in for ALE behind env.py's rules: a block that moves over a 210 x 160 screen, 3 lives, games of
    about 25 steps, and the last repeat of every game is cut (after its third frame in even games, before it in odd ones)."""
    H, W = 210, 160

    def __init__(self, seed):
        self.seed, self.game, self.t, self.lives, self.x = seed, -1, 0, 0, 0
        self.life_termination = False
        self.actions = []

    def _render(self, out, phase):
        y = (7 * self.t + 3 * phase + 11 * self.seed) % (self.H - 24)
        x = (self.x + 5 * phase) % (self.W - 20)
        out[...] = 20 + (self.game + self.seed) % 9
        out[y:y + 24, x:x + 20] = 120 + 40 * self.lives + phase

    def reset(self, out_a):
        if self.life_termination:                                  # env.py:36-38: one no-op
            self.life_termination = False
            self._render(out_a, 2)
        else:                                                      # env.py:40-47
            self.game += 1
            self.t, self.lives, self.x = 0, 3, (37 * self.game + 13 * self.seed) % 140
            self._render(out_a, 0)

    def step(self, action, out_a, out_b):
        self.actions.append(int(action))
        self.t += 1
        self.x = (self.x + (0, -9, 9)[action % 3]) % 140
        reward = float((action + self.t + self.seed) % 3 - 1) * 1.5                  # in {-1.5, 0, 1.5}: the clip matters
        last = 22 + (self.game + self.seed) % 6
        if self.t >= last:                                         # game over inside the repeat (env.py:64-66)
            if self.game % 2 == 0:
                self._render(out_a, 0)
                return OO.FRAME_A, reward, True, False
            return 0, reward, True, False
        self._render(out_a, 0)
        self._render(out_b, 1)
        if self.t in (last // 3, 2 * last // 3):                   # env.py:70-75
            self.lives -= 1
            self.life_termination = True
            return OO.STEP, reward, False, True
        return OO.STEP, reward, False, False


def _agent_args(**kw):
    base = dict(device=torch.device(DEV), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=4, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=32, noisy_std=0.1,
                replay_frequency=4, target_update=100, learn_start=200, reward_clip=1, evaluation_interval=120)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _host_vec_run(S, T_max, **kw):
    from rainbow_amd.agent import Agent
    from rainbow_amd.frames import FrameStackVec
    from rainbow_amd.loop import train_host_vec
    from rainbow_amd.memory import ReplayMemory
    args = _agent_args(**kw)
    torch.manual_seed(5)
    np.random.seed(5)
    agent = Agent(args, types.SimpleNamespace(action_space=lambda: 3))
    mem = ReplayMemory(args, 512, seed=5, streams=S)
    emus = [FakeEmu(s) for s in range(S)]
    evals = []
    learns = train_host_vec(agent, mem, emus, FrameStackVec(S, DEV), args, T_max, on_eval=evals.append)
    torch.cuda.synchronize()
    return args, mem, emus, learns, evals


@pytest.mark.parametrize("S", [4, 1])
def test_train_host_vec_cadence(S):
    # learn_start 200: the first draw needs clearly more than batch_size * (multi_step + 1) * S = 64 stored transitions
    T_max = 400
    args, mem, emus, learns, evals = _host_vec_run(S, T_max)
    owed, want = 0.0, 0
    for T in range(1, T_max + 1, S):
        if T >= args.learn_start:
            owed += S / args.replay_frequency
            while owed >= 1:
                owed -= 1
                want += 1
    assert learns == want and want >= 40
    assert mem.failed_samples() == 0
    assert evals == [T for T in range(1, T_max + 1, S) if T >= args.learn_start and T % args.evaluation_interval < S]
    assert all(len(e.actions) == T_max // S for e in emus) and min(e.game for e in emus) >= 2
    assert mem.priority_weight == pytest.approx(1.0)


@pytest.mark.parametrize("S", [4, 1])
def test_train_host_vec_fills_the_replay_the_oracle_deques_fill(S):
    """No learning (learn_start > T_max): the replay equals one filled by driving fresh fake emulators with the recorded
    actions through per-stream oracle deques and host-operand rounds."""
    from rainbow_amd.memory import ReplayMemory
    T_max = 400
    args, mem, emus, learns, _ = _host_vec_run(S, T_max, learn_start=T_max + 100)
    assert learns == 0
    twin = ReplayMemory(args, 512, seed=5, streams=S)
    fresh = [FakeEmu(s) for s in range(S)]
    deques = [OO.DequeOracle(4) for _ in range(S)]
    a, b = np.zeros((S, 210, 160), np.uint8), np.zeros((S, 210, 160), np.uint8)
    for s in range(S):
        fresh[s].reset(a[s])
        deques[s].reset(a[s])
    seen = set()
    for k in range(T_max // S):
        states = np.stack([d.stack() for d in deques])
        actions = np.array([emus[s].actions[k] for s in range(S)])
        rewards, terminals = np.zeros(S, np.float32), np.zeros(S, bool)
        for s in range(S):
            f, r, done, life_lost = fresh[s].step(int(actions[s]), a[s], b[s])
            rewards[s], terminals[s] = min(max(r, -1.0), 1.0), done or life_lost
            if done:
                fresh[s].reset(a[s])
                deques[s].reset(a[s])
            elif life_lost:
                fresh[s].reset(a[s])
                deques[s].life_reset(a[s])
            else:
                deques[s].step([a[s], b[s]])
            seen.add("done%d" % f if done else ("life" if life_lost else "step"))
        twin.append_streams(torch.from_numpy(states).to(DEV), actions, rewards, terminals)
    assert seen == {"done0", "done2", "life", "step"}
    _same_replay(mem, twin)
    assert np.array_equal(mem.stream_t, twin.stream_t)
