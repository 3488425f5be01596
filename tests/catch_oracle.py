"""Numpy restatement of the device Catch environment (rules: include/rainbow_hip.h, "device Catch").  TEST INFRASTRUCTURE: the
product path (rainbow_amd/) never imports it.

  - grid 12 x 12, one cell 7 x 7 pixels; ball 1 cell at 1.0, paddle 3 cells wide on the bottom row at 0.5, background 0;
  - actions 0 stay, 1 left, 2 right (paddle's left cell clamped to [0, 9]); anything else counts as stay;
  - per step the paddle moves, then the ball falls one row; on the bottom row the episode ends, reward +1 if the ball's
    column is under the paddle else -1; other steps 0 (11 steps per episode);
  - episode e of stream s starts with ball column x0 % 12 (row 0) and paddle x1 % 10, (x0, x1, ., .) = Philox4x32-10 with
    key = seed and counter (lo = e, hi = s);
  - a step that ends the episode returns the reset stack of the stream's next episode.

`CatchOracle` is the vectorised form (S streams); `CatchEnv` wraps S = 1 in the reference's Env surface (env.py)."""
import numpy as np

GRID, CELL, PADDLE, ACTIONS = 12, 7, 3, 3
M32 = 0xFFFFFFFF


def philox4x32_10(seed, ctr_hi, ctr_lo):
    """Philox4x32-10: 64-bit key `seed`, 128-bit counter (ctr_lo | ctr_hi << 64) -> four uint32 (rb_philox, csrc/rb_common.h)."""
    c0, c1, c2, c3 = ctr_lo & M32, (ctr_lo >> 32) & M32, ctr_hi & M32, (ctr_hi >> 32) & M32
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def episode_start(seed, s, e):
    x = philox4x32_10(int(seed), int(s), int(e))
    return x[0] % GRID, x[1] % (GRID - PADDLE + 1)


def render(ball_col, ball_row, paddle):
    f = np.zeros((GRID, GRID), dtype=np.float32)
    f[GRID - 1, paddle:paddle + PADDLE] = 0.5
    f[ball_row, ball_col] = 1.0
    return np.kron(f, np.ones((CELL, CELL), dtype=np.float32))


class CatchOracle:
    def __init__(self, streams, history, seed):
        self.S, self.h, self.seed = int(streams), int(history), int(seed)
        self.episode = np.full(self.S, -1, dtype=np.int64)
        self.ball_col = np.zeros(self.S, dtype=np.int64)
        self.ball_row = np.zeros(self.S, dtype=np.int64)
        self.paddle = np.zeros(self.S, dtype=np.int64)
        self.stacks = np.zeros((self.S, self.h, 84, 84), dtype=np.float32)
        self.reset_stats()

    def reset_stats(self):
        self.episodes_done, self.catches, self.return_sum = 0, 0, 0.0

    def _begin(self, s):
        self.episode[s] += 1
        self.ball_col[s], self.paddle[s] = episode_start(self.seed, s, self.episode[s])
        self.ball_row[s] = 0
        self.stacks[s] = 0.0
        self.stacks[s, -1] = render(self.ball_col[s], 0, self.paddle[s])

    def reset(self):
        for s in range(self.S):
            self._begin(s)
        return self.stacks.copy()

    def step(self, actions):
        """-> (next_stacks f32 [S,h,84,84], rewards f32 [S], terminals bool [S])"""
        rewards = np.zeros(self.S, dtype=np.float32)
        terminals = np.zeros(self.S, dtype=bool)
        for s in range(self.S):
            a = int(actions[s])
            if a == 1:
                self.paddle[s] = max(self.paddle[s] - 1, 0)
            elif a == 2:
                self.paddle[s] = min(self.paddle[s] + 1, GRID - PADDLE)
            self.ball_row[s] += 1
            if self.ball_row[s] < GRID - 1:
                self.stacks[s, :-1] = self.stacks[s, 1:].copy()
                self.stacks[s, -1] = render(self.ball_col[s], self.ball_row[s], self.paddle[s])
                continue
            caught = self.paddle[s] <= self.ball_col[s] < self.paddle[s] + PADDLE
            rewards[s] = 1.0 if caught else -1.0
            terminals[s] = True
            self.episodes_done += 1
            self.catches += int(caught)
            self.return_sum += float(rewards[s])
            self._begin(s)
        return self.stacks.copy(), rewards, terminals

    def stats(self):
        return dict(episodes=self.episodes_done, catches=self.catches, return_sum=self.return_sum)


class CatchEnv:
    """One stream with the reference's Env surface (env.py): reset() -> state, step(action) -> (state, reward, done), train(),
    eval(), action_space(), close().  States are torch float32 [h, 84, 84] on `device`.  A reset() right after the step that
    ended an episode hands out the reset stack that step already produced (no episode is skipped)."""

    def __init__(self, seed, history_length=4, device="cpu"):
        import torch
        self._torch, self.device = torch, device
        self.core = CatchOracle(1, history_length, seed)
        self._pending = None

    def _t(self, stack):
        return self._torch.from_numpy(stack.copy()).to(self.device)

    def reset(self):
        if self._pending is not None:
            out, self._pending = self._pending, None
            return self._t(out)
        return self._t(self.core.reset()[0])

    def step(self, action):
        self._pending = None
        stacks, rewards, terminals = self.core.step([action])
        if terminals[0]:
            self._pending = stacks[0]
        return self._t(stacks[0]), float(rewards[0]), bool(terminals[0])

    def action_space(self):
        return ACTIONS

    def train(self):
        pass

    def eval(self):
        pass

    def close(self):
        pass
