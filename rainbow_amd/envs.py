"""Environments that live on the device (librainbow_hip.so, rb_catch_*; rules in include/rainbow_hip.h).

`CatchVec(streams, device, seed)` is S independent games of Catch on the 84 x 84 screen.  `reset()` and `step(actions)` are
one launch each on the current stream and hand back device tensors — nothing is copied to the host and nothing synchronises,
so Agent.act_batch(states, device_out=True) -> env.step -> ReplayMemory.append_streams is a round that never leaves the device
(rainbow_amd.loop.train_device).  Episode totals accumulate on the device; `stats()` fetches them (that call synchronises).

With streams=1 the object also has the reference's Env surface (env.py): reset() -> state [h,84,84], step(int) -> (state,
reward, done), train(), eval(), action_space(), close() — it can be handed to the reference-shaped single-environment loop."""
import ctypes as C

import torch

from . import _lib as L
from .agent import current_stream_handle


class CatchVec:
    ACTIONS = 3
    reward_range = (-1.0, 1.0)

    def __init__(self, streams, device, seed, history_length=4):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rainbow_amd.envs.CatchVec lives on the device: got %s" % self.device)
        self._lib = L.load()
        self.streams, self.history, self.seed = int(streams), int(history_length), int(seed)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self._lib, self._lib.rb_catch_create(C.byref(self._h), self.streams, self.history, self.seed))
        S = self.streams
        # two stack buffers used in turn (the step is out of place); per buffer its own reward / flag vectors, so what a step
        # handed out stays valid until the step after the next one
        self._stacks = [torch.zeros(S, self.history, 84, 84, dtype=torch.float32, device=self.device) for _ in range(2)]
        self._rewards = [torch.zeros(S, dtype=torch.float32, device=self.device) for _ in range(2)]
        self._nonterm = [torch.ones(S, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._cur = 0
        self.nonterminals = self._nonterm[0]      # uint8 [S] of the last step (1 = the episode goes on)
        self._auto_reset = False                  # streams == 1: the last step ended the episode and already produced the reset stack

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rb_catch_destroy(self._h)
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
        L.check(self._lib, self._lib.rb_catch_reset(self._h, self._stacks[self._cur].data_ptr(), self._stream()))
        return self._stacks[self._cur] if self.streams > 1 else self._stacks[self._cur][0]

    def step_device(self, actions):
        """actions int32 [S] on the device -> (next_stacks f32 [S,h,84,84], rewards f32 [S], nonterminals u8 [S]), all on the
        device, no synchronisation.  Where a step ended the episode, next_stacks holds the reset stack of the next one."""
        if actions.dtype != torch.int32 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        self._actions = actions
        cur, nxt = self._cur, self._cur ^ 1
        rc = self._lib.rb_catch_step(self._h, actions.data_ptr(), self._stacks[cur].data_ptr(), self._stacks[nxt].data_ptr(),
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

    def stats(self):
        """dict(episodes, catches, return_sum, mean_return) accumulated on the device since the last reset_stats().
        SYNCHRONISES the stream."""
        st = L.CatchStats()
        L.check(self._lib, self._lib.rb_catch_stats(self._h, C.byref(st), self._stream()))
        n = int(st.episodes)
        return dict(episodes=n, catches=int(st.catches), return_sum=float(st.return_sum),
                    mean_return=float(st.return_sum) / n if n else float("nan"))

    def reset_stats(self):
        L.check(self._lib, self._lib.rb_catch_reset_stats(self._h, self._stream()))
