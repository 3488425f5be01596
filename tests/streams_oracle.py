"""S interleaved environment streams in one replay — TEST INFRASTRUCTURE, the oracle of rb_replay_create_streams.

A restatement ON TOP OF oracle.replay_oracle (the single-stream ReplayOracle, pinned to the reference by the golden
vectors): storage, sum tree, tree search, n-step arithmetic and IS weights are the base class's own code.  What S streams
change is restated here and nowhere else:
  - an append ROUND is S sequential appends (SegmentTree.append, memory.py:56-61) in stream order, each stream with its own
    episode timestep t[s] (memory.py:100,108); stream s owns the ring slots s, s + S, s + 2S, ...
  - the window of slot idx is idx + k S (mod C), k = -(h-1) .. n (memory.py:111-121 with stride S),
  - validity per stream (memory.py:131): j = idx div S, J = index div S, Cs = C / S;
    (J - j) mod Cs > n and (j - J) mod Cs >= h and prob != 0,
  - validation stacks (memory.py:167-178): slots i - (h-1-t) S (mod C).
Every stream is ALSO fed to an unmodified single-stream ReplayOracle of capacity C / S (`per_stream`), so a test can check
that a window of the S-stream replay is exactly what the plain algorithm gives for that stream alone.
"""
import numpy as np

from oracle.replay_oracle import ReplayOracle


class StreamsOracle(ReplayOracle):
    def __init__(self, capacity, streams, history=4, discount=0.99, multi_step=3, priority_weight=0.4,
                 priority_exponent=0.5, per_stream=True):
        super().__init__(capacity, history=history, discount=discount, multi_step=multi_step,
                         priority_weight=priority_weight, priority_exponent=priority_exponent)
        S = int(streams)
        assert 1 <= S <= 64 and capacity % S == 0 and capacity > (history + multi_step) * S
        self.streams = S
        self.stream_t = np.zeros(S, dtype=np.int32)
        self.per_stream = None
        if per_stream:
            self.per_stream = [ReplayOracle(capacity // S, history=history, discount=discount, multi_step=multi_step,
                                            priority_weight=priority_weight, priority_exponent=priority_exponent)
                               for _ in range(S)]

    # -- writes ------------------------------------------------------------------
    def append_round_frames(self, frames_u8, actions, rewards, terminals):
        """One round: stream s appends (frames_u8[s], actions[s], rewards[s], terminals[s]) at the running max, s = 0..S-1."""
        tr = self.transitions
        assert tr.index % self.streams == 0
        for s in range(self.streams):
            term = bool(terminals[s])
            tr.append(int(self.stream_t[s]), frames_u8[s], int(actions[s]), np.float32(rewards[s]), not term, tr.max)
            self.stream_t[s] = 0 if term else self.stream_t[s] + 1                 # memory.py:108, per stream
            if self.per_stream is not None:
                self.per_stream[s].append_frame(frames_u8[s], int(actions[s]), np.float32(rewards[s]), term)

    def append_round(self, states_f32, actions, rewards, terminals):
        """states_f32 [S, h, 84, 84]: each stream's state[-1] quantised as memory.py:106."""
        self.append_round_frames(np.stack([self.quantise(st) for st in states_f32]), actions, rewards, terminals)

    # -- reads -------------------------------------------------------------------
    def window(self, idxs):
        h, n, S = self.history, self.n, self.streams
        tr = self.transitions
        offs = np.arange(-h + 1, n + 1, dtype=np.int64) * S
        ring = (np.asarray(idxs, dtype=np.int64)[:, None] + offs[None, :]) % self.capacity
        first = tr.timestep[ring] == 0
        blank = np.zeros_like(first)
        for t in range(h - 2, -1, -1):
            blank[:, t] = blank[:, t + 1] | first[:, t + 1]
        for t in range(h, h + n):
            blank[:, t] = blank[:, t - 1] | first[:, t]
        return ring, blank

    def valid(self, idxs, probs):
        """memory.py:131 per stream (elementwise)."""
        S, Cs = self.streams, self.capacity // self.streams
        j = np.asarray(idxs, dtype=np.int64) // S
        J = self.transitions.index // S
        return ((J - j) % Cs > self.n) & ((j - J) % Cs >= self.history) & (np.asarray(probs) != 0)

    def draw_indices(self, batch, unit_uniforms, trace=None):
        """memory.py:124-132 with the per-stream validity; `trace` (a list) receives (samples' data indices, ok) per attempt."""
        tr = self.transitions
        p_total = tr.total()
        seg = np.float32(p_total) / np.float32(batch)
        starts = np.arange(batch, dtype=np.int64) * np.float64(seg)
        unit_uniforms = np.asarray(unit_uniforms, dtype=np.float64).reshape(-1, batch)
        for attempt, u in enumerate(unit_uniforms, 1):
            samples = (0.0 + np.float64(seg) * u) + starts
            probs, idxs, tree_idxs = tr.find(samples)
            ok = bool(np.all(self.valid(idxs, probs)))
            if trace is not None:
                trace.append((idxs.copy(), probs.copy(), ok))
            if ok:
                return probs, idxs, tree_idxs, attempt
        raise RuntimeError("streams oracle: no valid batch within the supplied attempts")

    def state_at(self, i):
        h, S = self.history, self.streams
        tr = self.transitions
        ring = (i - np.arange(h - 1, -1, -1, dtype=np.int64) * S) % self.capacity
        first = tr.timestep[ring] == 0
        blank = np.zeros(h, dtype=bool)
        for t in range(h - 2, -1, -1):
            blank[t] = blank[t + 1] | first[t + 1]
        frames = tr.frames[ring].copy()
        frames[blank] = 0
        return frames.astype(np.float32) / np.float32(255)

    # -- the per-stream view -----------------------------------------------------
    def stream_window(self, idx):
        """The window of ring slot idx as the single-stream oracle of its stream computes it: (ring slots mapped back to the
        interleaved ring, blank mask, action, n-step return, nonterminal)."""
        S = self.streams
        s, j = int(idx) % S, int(idx) // S
        sub = self.per_stream[s]
        ring, blank = sub.window(np.array([j]))
        with np.errstate(all="ignore"):          # (the weight of a lone sample is of no interest here)
            sc = sub.batch_scalars(np.array([j]), np.ones(1, dtype=np.float32))
        return ring[0] * S + s, blank[0], sc["actions"][0], sc["returns"][0], sc["nonterminals"][0, 0]
