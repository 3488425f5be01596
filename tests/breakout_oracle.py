"""Numpy restatement of the device Breakout environment (rules: include/rainbow_hip.h, "device Breakout").  TEST
INFRASTRUCTURE: the product path (rainbow_amd/) never imports it.

  - grid 12 x 12, one cell 7 x 7 pixels; ball 1 cell at 1.0, bricks in rows 1 .. 3 at 0.75, paddle 2 cells wide on row 11 at
    0.5, background 0; 3 lives per game; actions 0 stay, 1 left, 2 right, anything else counts as stay;
  - serve k of stream s: (x0, x1, x2, .) = Philox4x32-10 with key = seed and counter (lo = k, hi = s); ball at (x0 % 12, 4),
    dx = +1 if x1 is odd else -1, dy = +1; a new game also sets the paddle to x2 % 11, refills the bricks, lives = 3, t = 0;
  - a step: paddle, t += 1, reflection off the side walls and the ceiling, then brick (reward 5 - row, dy flips, the ball stays)
    or paddle row (bounce: dx by the paddle cell hit, refill when no brick is left; miss: a life is lost, the game is over with
    the last one) or a plain move; t == max_steps ends the game; over -> new game, lost -> serve;
  - a step that ends the game returns the reset stack of the next one; after a lost life the stack just moves on by one frame
    (the render of the serve state).

`BreakoutOracle` is the vectorised form (S streams); `BreakoutEnv` wraps S = 1 in the reference's Env surface (env.py).  After
every step `events` holds, per stream, what happened in it (the coverage asserts of the tests read these)."""
import numpy as np

from catch_oracle import philox4x32_10

GRID, CELL, PADDLE, ACTIONS, LIVES, SERVE_ROW = 12, 7, 2, 3, 3, 4
FULL = 0xFFF
EVENTS = ("lost", "over", "capped", "brick_row", "ceiling", "wall", "paddle_cell", "refill")


def serve_draw(seed, s, k):
    """-> (bx, dx, paddle of a new game)"""
    x = philox4x32_10(int(seed), int(s), int(k))
    return x[0] % GRID, (1 if x[1] & 1 else -1), x[2] % (GRID - PADDLE + 1)


def render(g):
    f = np.zeros((GRID, GRID), dtype=np.float32)
    for r in range(3):
        for c in range(GRID):
            if g["rows"][r] >> c & 1:
                f[r + 1, c] = 0.75
    f[GRID - 1, g["paddle"]:g["paddle"] + PADDLE] = 0.5
    assert f[g["by"], g["bx"]] == 0.0, "the ball is on a brick or paddle cell"
    f[g["by"], g["bx"]] = 1.0
    return np.kron(f, np.ones((CELL, CELL), dtype=np.float32))


def blank_game():
    return dict(bx=0, by=0, dx=0, dy=0, paddle=0, t=0, k=-1, rows=[0, 0, 0], lives=0, game_return=0,
                games=0, return_sum=0, bricks=0, lives_lost=0, steps=0)


TOTALS = ("games", "return_sum", "bricks", "lives_lost", "steps")


class BreakoutOracle:
    def __init__(self, streams, history, max_steps, seed):
        self.S, self.h, self.max_steps, self.seed = int(streams), int(history), int(max_steps), int(seed)
        self.g = [blank_game() for _ in range(self.S)]
        self.stacks = np.zeros((self.S, self.h, 84, 84), dtype=np.float32)
        self.events = [dict() for _ in range(self.S)]

    # ---- the rules
    def _serve(self, s, new_game):
        g = self.g[s]
        g["k"] += 1
        bx, dx, paddle = serve_draw(self.seed, s, g["k"])
        g.update(bx=bx, by=SERVE_ROW, dx=dx, dy=1)
        if new_game:
            g.update(paddle=paddle, rows=[FULL] * 3, lives=LIVES, t=0, game_return=0)

    def _reset_stack(self, s):
        self.stacks[s] = 0.0
        self.stacks[s, -1] = render(self.g[s])

    def reset(self):
        for s in range(self.S):
            self._serve(s, True)
            self._reset_stack(s)
        return self.stacks.copy()

    def _step_one(self, s, a):
        g, ev = self.g[s], dict.fromkeys(EVENTS)
        if a == 1:
            g["paddle"] = max(g["paddle"] - 1, 0)
        elif a == 2:
            g["paddle"] = min(g["paddle"] + 1, GRID - PADDLE)
        g["t"] += 1
        g["steps"] += 1
        reward, lost, over = 0, False, False
        nx = g["bx"] + g["dx"]
        if nx < 0 or nx > GRID - 1:
            g["dx"] = -g["dx"]
            nx = g["bx"] + g["dx"]
            ev["wall"] = True
        ny = g["by"] + g["dy"]
        if ny < 0:
            g["dy"] = 1
            ny = g["by"] + g["dy"]
            ev["ceiling"] = True
        if 1 <= ny <= 3 and g["rows"][ny - 1] >> nx & 1:
            g["rows"][ny - 1] &= ~(1 << nx)
            reward = 5 - ny
            g["dy"] = -g["dy"]
            g["bricks"] += 1
            ev["brick_row"] = ny
        elif ny == GRID - 1:
            if g["paddle"] <= nx <= g["paddle"] + 1:
                g["bx"], g["dy"] = nx, -1
                g["dx"] = -1 if nx == g["paddle"] else 1
                ev["paddle_cell"] = nx - g["paddle"]
                if not any(g["rows"]):
                    g["rows"] = [FULL] * 3
                    ev["refill"] = True
            else:
                g["lives"] -= 1
                g["lives_lost"] += 1
                lost, over = True, g["lives"] == 0
        else:
            g["bx"], g["by"] = nx, ny
        g["game_return"] += reward
        if g["t"] == self.max_steps:
            over = True
            ev["capped"] = True
        if over:
            g["games"] += 1
            g["return_sum"] += g["game_return"]
        if over or lost:
            self._serve(s, over)
        ev["lost"], ev["over"] = lost, over
        self.events[s] = ev
        return reward, lost, over

    def step(self, actions, life_terminals=True):
        """-> (next_stacks f32 [S,h,84,84], rewards f32 [S], terminals bool [S])"""
        rewards = np.zeros(self.S, dtype=np.float32)
        terminals = np.zeros(self.S, dtype=bool)
        for s in range(self.S):
            reward, lost, over = self._step_one(s, int(actions[s]))
            rewards[s] = reward
            terminals[s] = over or (lost and bool(life_terminals))
            if over:
                self._reset_stack(s)
            else:
                self.stacks[s, :-1] = self.stacks[s, 1:].copy()
                self.stacks[s, -1] = render(self.g[s])
        return self.stacks.copy(), rewards, terminals

    # ---- totals and state
    def stats(self):
        return {k: sum(g[k] for g in self.g) for k in TOTALS}

    def reset_stats(self):
        for g in self.g:
            for k in TOTALS:
                g[k] = 0

    def landing_column(self, s):
        """Where the ball of stream s reaches the paddle row if no brick deflects it (the scripted policy aims there)."""
        g = self.g[s]
        bx, by, dx, dy = g["bx"], g["by"], g["dx"], g["dy"]
        for _ in range(64):
            nx = bx + dx
            if nx < 0 or nx > GRID - 1:
                dx = -dx
                nx = bx + dx
            ny = by + dy
            if ny < 0:
                dy = 1
                ny = by + dy
            if ny == GRID - 1:
                return nx
            bx, by = nx, ny
        return bx


class BreakoutEnv:
    """One stream with the reference's Env surface (env.py), like catch_oracle.CatchEnv: train() reports lost lives as
    terminals (env.py:70-75), eval() does not.  A reset() right after a step that ended the GAME hands out the reset stack
    that step already produced; after a step that only lost a life it hands out the current stack (the game goes on)."""

    def __init__(self, seed, history_length=4, max_steps=500, device="cpu"):
        import torch
        self._torch, self.device = torch, device
        self.core = BreakoutOracle(1, history_length, max_steps, seed)
        self.training = True
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
        stacks, rewards, terminals = self.core.step([action], life_terminals=self.training)
        if terminals[0]:
            self._pending = stacks[0]
        return self._t(stacks[0]), float(rewards[0]), bool(terminals[0])

    def action_space(self):
        return ACTIONS

    def train(self):
        self.training = True

    def eval(self):
        self.training = False

    def close(self):
        pass
