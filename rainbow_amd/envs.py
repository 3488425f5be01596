"""Environments that live on the device (librainbow_hip.so, rb_catch_* and rb_breakout_*; rules in include/rainbow_hip.h).

`CatchVec(streams, device, seed)` is S independent games of Catch on the 84 x 84 screen.  `reset()` and `step(actions)` are
one launch each on the current stream and hand back device tensors — nothing is copied to the host and nothing synchronises,
so Agent.act_batch(states, device_out=True) -> env.step -> ReplayMemory.append_streams is a round that never leaves the device
(rainbow_amd.loop.train_device).  Episode totals accumulate on the device; `stats()` fetches them (that call synchronises).

`BreakoutVec(streams, device, seed, history_length=4, max_steps=500, training=True)` is S games of a small Breakout behind the
same surface: 36 bricks worth 2 / 3 / 4, three lives, games of varying length capped at `max_steps`.  In training mode
(`train()`, the default) a lost life is reported as a terminal while the game goes on (env.py:70-75); in evaluation mode
(`eval()`, or training=False) only the end of the game is.  `state_dict()` / `load_state_dict()` checkpoint it exactly.

With streams=1 either object also has the reference's Env surface (env.py): reset() -> state [h,84,84], step(int) -> (state,
reward, done), train(), eval(), action_space(), close() — it can be handed to the reference-shaped single-environment loop."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._util import current_stream_handle


class _DeviceEnv:
    """What the device environments share: the handle, the two stack buffers a step alternates between, and the Env surface of
    one stream.  A game supplies _PREFIX (its rb_* entry points), _create() and _step_call()."""
    ACTIONS = 3
    _PREFIX = None
    _h = None                  # (close() is safe on an object whose construction failed early)

    def __init__(self, streams, device, seed, history_length):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rainbow_amd.envs.%s lives on the device: got %s" % (type(self).__name__, self.device))
        self._lib = L.load()
        self.streams, self.history, self.seed = int(streams), int(history_length), int(seed)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self._lib, self._create())
        S = self.streams
        # two stack buffers used in turn (the step is out of place); per buffer its own reward / flag vectors, so what a step
        # handed out stays valid until the step after the next one
        self._stacks = [torch.zeros(S, self.history, 84, 84, dtype=torch.float32, device=self.device) for _ in range(2)]
        self._rewards = [torch.zeros(S, dtype=torch.float32, device=self.device) for _ in range(2)]
        self._nonterm = [torch.ones(S, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._cur = 0
        self.nonterminals = self._nonterm[0]      # uint8 [S] of the last step (1 = the episode goes on)
        self._auto_reset = False                  # streams == 1: the last step ended the episode and already produced the next stack

    def _fn(self, name):
        return getattr(self._lib, "%s_%s" % (self._PREFIX, name))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return current_stream_handle(self.device)

    def action_space(self):
        return self.ACTIONS

    def train(self):
        pass

    def eval(self):
        pass

    def reset(self):
        """Every stream starts its next episode.  -> stacks f32 [S, h, 84, 84] ([h, 84, 84] with one stream)."""
        if self.streams == 1 and self._auto_reset:
            self._auto_reset = False              # (the step that ended the episode already wrote this stack: no episode is skipped)
            return self._stacks[self._cur][0]
        L.check(self._lib, self._fn("reset")(self._h, self._stacks[self._cur].data_ptr(), self._stream()))
        return self._stacks[self._cur] if self.streams > 1 else self._stacks[self._cur][0]

    def step_device(self, actions):
        """actions int32 [S] on the device -> (next_stacks f32 [S,h,84,84], rewards f32 [S], nonterminals u8 [S]), all on the
        device, no synchronisation.  Where a step ended the episode, next_stacks holds the reset stack of the next one."""
        if actions.dtype != torch.int32 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        self._actions = actions
        cur, nxt = self._cur, self._cur ^ 1
        rc = self._step_call(actions.data_ptr(), self._stacks[cur].data_ptr(), self._stacks[nxt].data_ptr(),
                             self._rewards[nxt].data_ptr(), self._nonterm[nxt].data_ptr(), self._stream())
        if rc != 0:
            L.check(self._lib, rc)
        self._cur = nxt
        self.nonterminals = self._nonterm[nxt]
        return self._stacks[nxt], self._rewards[nxt], self._nonterm[nxt]

    def step(self, actions):
        """Vectorised: actions (device tensor) -> (next_stacks, rewards, terminals) as device tensors (terminals bool [S]).
        With one stream and a plain int: the reference's Env.step -> (state [h,84,84], reward float, done bool); that form
        reads the reward back and therefore synchronises."""
        if self.streams == 1 and not torch.is_tensor(actions):
            a = torch.tensor([int(actions)], dtype=torch.int32).to(self.device)
            stacks, rewards, nonterm = self.step_device(a)
            done = int(nonterm.item()) == 0
            self._auto_reset = done
            return stacks[0], float(rewards.item()), done
        stacks, rewards, nonterm = self.step_device(actions)
        return stacks, rewards, nonterm == 0

    def reset_stats(self):
        L.check(self._lib, self._fn("reset_stats")(self._h, self._stream()))


class CatchVec(_DeviceEnv):
    reward_range = (-1.0, 1.0)
    _PREFIX = "rb_catch"

    def __init__(self, streams, device, seed, history_length=4):
        super().__init__(streams, device, seed, history_length)

    def _create(self):
        return self._lib.rb_catch_create(C.byref(self._h), self.streams, self.history, self.seed)

    def _step_call(self, *operands):
        return self._lib.rb_catch_step(self._h, *operands)

    def stats(self):
        """dict(episodes, catches, return_sum, mean_return) accumulated on the device since the last reset_stats().
        SYNCHRONISES the stream."""
        st = L.CatchStats()
        L.check(self._lib, self._lib.rb_catch_stats(self._h, C.byref(st), self._stream()))
        n = int(st.episodes)
        return dict(episodes=n, catches=int(st.catches), return_sum=float(st.return_sum),
                    mean_return=float(st.return_sum) / n if n else float("nan"))


class BreakoutVec(_DeviceEnv):
    reward_range = (0.0, 4.0)
    _PREFIX = "rb_breakout"

    def __init__(self, streams, device, seed, history_length=4, max_steps=500, training=True):
        self.max_steps, self.training = int(max_steps), bool(training)
        super().__init__(streams, device, seed, history_length)

    def _create(self):
        return self._lib.rb_breakout_create(C.byref(self._h), self.streams, self.history, self.max_steps, self.seed)

    def _step_call(self, actions, stacks_in, stacks_out, rewards, nonterminals, stream):
        return self._lib.rb_breakout_step(self._h, actions, stacks_in, stacks_out, rewards, nonterminals, 1 if self.training else 0, stream)

    def train(self):
        """A lost life is a terminal (nonterminals == 0) although the game goes on: env.py:70-75."""
        self.training = True

    def eval(self):
        """Only the end of a game is a terminal (what evaluate_vec needs: test.py:17 evaluates an env in eval mode)."""
        self.training = False

    def stats(self):
        """dict(games, episodes (= games), return_sum, mean_return, bricks, lives_lost, steps) accumulated on the device since
        the last reset_stats(); return_sum is the sum of the unclipped returns of the games FINISHED.  SYNCHRONISES the stream."""
        st = L.BreakoutStats()
        L.check(self._lib, self._lib.rb_breakout_stats(self._h, C.byref(st), self._stream()))
        n = int(st.games)
        return dict(games=n, episodes=n, return_sum=float(st.return_sum), mean_return=float(st.return_sum) / n if n else float("nan"),
                    bricks=int(st.bricks), lives_lost=int(st.lives_lost), steps=int(st.steps))

    def state_dict(self):
        """Everything the next step depends on: the game state of every stream (rb_breakout_state_t, raw bytes), the current
        stack buffer and the mode.  SYNCHRONISES the stream."""
        arr = (L.BreakoutState * self.streams)()
        L.check(self._lib, self._lib.rb_breakout_get_state(self._h, arr, self._stream()))
        return dict(streams=self.streams, history=self.history, max_steps=self.max_steps, seed=self.seed, training=self.training,
                    auto_reset=self._auto_reset, game=np.frombuffer(bytes(arr), dtype=np.uint8).copy(),
                    stacks=self._stacks[self._cur].cpu())

    def load_state_dict(self, sd):
        """Continue exactly where state_dict() was taken (an environment of the same shape, cap and seed).  SYNCHRONISES."""
        for k in ("streams", "history", "max_steps", "seed"):
            if int(sd[k]) != getattr(self, k):
                raise ValueError("BreakoutVec.load_state_dict: %s is %d here, %d in the checkpoint" % (k, getattr(self, k), int(sd[k])))
        raw = np.ascontiguousarray(sd["game"], dtype=np.uint8).tobytes()
        if len(raw) != C.sizeof(L.BreakoutState) * self.streams:
            raise ValueError("BreakoutVec.load_state_dict: the game state has %d bytes, not %d" % (len(raw), C.sizeof(L.BreakoutState) * self.streams))
        arr = (L.BreakoutState * self.streams).from_buffer_copy(raw)
        L.check(self._lib, self._lib.rb_breakout_set_state(self._h, arr, self._stream()))
        self._stacks[self._cur].copy_(sd["stacks"].to(self.device))
        self.training, self._auto_reset = bool(sd["training"]), bool(sd["auto_reset"])
