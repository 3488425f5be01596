"""Numpy restatement of the evaluation pieces (rules: include/rainbow_hip.h, rb_learner_act_batch_eps and "episode tally").
TEST INFRASTRUCTURE: the product path (rainbow_amd/) never imports it.

  - the e-greedy draw of row `row` in call `round`: (x0, x1, ., .) = Philox4x32-10(key = seed, counter = (lo = round, hi = row)),
    u = float32(x0 >> 8) * 2^-24, explore iff u < float32(epsilon), explored action = x1 % A;
  - the tally: stream s records its first E // S + (s < E % S) episodes as (f32 running return, length), the ending step's
    reward belongs to the ending episode, later episodes are ignored, the record is stream-major, unfilled slots (NaN, 0)."""
import numpy as np

from catch_oracle import philox4x32_10


def eps_draw(seed, rnd, row, epsilon, A):
    """-> (explore bool, explored action int)"""
    x = philox4x32_10(int(seed), int(row), int(rnd))
    u = np.float32(x[0] >> 8) * np.float32(2.0 ** -24)          # (x0 >> 8 < 2^24: exact in f32, and so is the product)
    return bool(u < np.float32(epsilon)), int(x[1] % A)


def eps_rows(seed, rnd, row0, n, epsilon, A):
    """-> (explored uint8 [n], actions int64 [n]) of rows row0 .. row0 + n - 1"""
    d = [eps_draw(seed, rnd, row0 + i, epsilon, A) for i in range(n)]
    return np.array([e for e, _ in d], dtype=np.uint8), np.array([a for _, a in d], dtype=np.int64)


def quotas(S, E):
    return np.array([E // S + (1 if s < E % S else 0) for s in range(S)], dtype=np.int64)


class TallyOracle:
    def __init__(self, streams, episodes):
        self.S, self.E = int(streams), int(episodes)
        self.q = quotas(self.S, self.E)
        self.off = np.concatenate([[0], np.cumsum(self.q)[:-1]]).astype(np.int64)
        self.reset()

    def reset(self):
        self.ret = np.zeros(self.S, dtype=np.float32)
        self.len = np.zeros(self.S, dtype=np.int32)
        self.rec = np.zeros(self.S, dtype=np.int64)
        self.returns = np.full(self.E, np.nan, dtype=np.float32)
        self.lengths = np.zeros(self.E, dtype=np.int32)

    def step(self, rewards, nonterminals):
        for s in range(self.S):
            self.ret[s] = np.float32(self.ret[s] + np.float32(rewards[s]))
            self.len[s] += 1
            if not nonterminals[s]:
                if self.rec[s] < self.q[s]:
                    k = self.off[s] + self.rec[s]
                    self.returns[k], self.lengths[k] = self.ret[s], self.len[s]
                    self.rec[s] += 1
                self.ret[s], self.len[s] = 0.0, 0

    def remaining(self):
        return int((self.q - self.rec).sum())

    def result(self):
        streams = np.repeat(np.arange(self.S), self.q).astype(np.int32)
        return self.returns.copy(), self.lengths.copy(), streams
