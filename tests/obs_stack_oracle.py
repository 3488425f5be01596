"""env.py's observation wrapper restated on numpy, one state deque per stream (TEST INFRASTRUCTURE): the oracle of
rb_obs_stack_step / rainbow_amd.frames.FrameStackVec.  The resize is oracle.frame_oracle's (cv2 parity UNPINNED, see there).

    env.py:24      state_buffer = deque([], maxlen=history_length)
    env.py:31-33   _reset_buffer: history_length blank frames
    env.py:35-52   reset(): after a lost life one no-op and NO blanking, else blank + new game; then append(_get_state())
    env.py:54-68   step(): frame_buffer = zeros(2, 84, 84); the states after frames 3 and 4 of the repeat go into it IF the
                   repeat got that far (it is cut when the game ends); append(frame_buffer.max(0))
"""
from collections import deque

import numpy as np

from oracle import frame_oracle as F

BLANK, FRAME_A, FRAME_B = 1, 2, 4
STEP, RESET, LIFE_RESET = FRAME_A | FRAME_B, BLANK | FRAME_A, FRAME_A


class DequeOracle:
    """One stream: env.py's state_buffer."""

    def __init__(self, history, fill=0.0):
        self.history = history
        self.buf = deque([np.full((84, 84), fill, dtype=np.float32) for _ in range(history)], maxlen=history)

    def _reset_buffer(self):                                    # env.py:31-33
        for _ in range(self.history):
            self.buf.append(np.zeros((84, 84), dtype=np.float32))

    def reset(self, screen):                                    # env.py:40-52, a new game
        self._reset_buffer()
        self.buf.append(F.get_state(screen))
        return self.stack()

    def life_reset(self, screen):                               # env.py:36-38,49-52: the screen after the no-op
        self.buf.append(F.get_state(screen))
        return self.stack()

    def step(self, taken):                                      # env.py:56-68; `taken`: the screens of frames 3, 4 that were reached
        frame_buffer = np.zeros((2, 84, 84), dtype=np.float32)
        for i, screen in enumerate(taken):
            frame_buffer[i] = F.get_state(screen)
        self.buf.append(frame_buffer.max(0))
        return self.stack()

    def apply(self, flags, a, b, get_state=F.get_state):
        """Any of the eight flag values, as include/rainbow_hip.h defines them (3, 2, 6, 2 and 0 are the paths above)."""
        if flags & BLANK:
            self._reset_buffer()
        frame_buffer = np.zeros((2, 84, 84), dtype=np.float32)
        if flags & FRAME_A:
            frame_buffer[0] = get_state(a)
        if flags & FRAME_B:
            frame_buffer[1] = get_state(b)
        self.buf.append(frame_buffer.max(0))
        return self.stack()

    def stack(self):
        return np.stack(list(self.buf), 0)                      # env.py:52,77


class StackOracle:
    """S streams."""

    def __init__(self, S, history, fill=0.0):
        self.streams = [DequeOracle(history, fill) for _ in range(S)]

    def apply(self, flags, a, b, get_state=F.get_state):
        """`get_state`: frame_oracle.get_state, or a memoising wrapper of it (the states do not depend on the history length)."""
        return np.stack([d.apply(int(f), a[s] if a is not None else None, b[s] if b is not None else None, get_state)
                         for s, (d, f) in enumerate(zip(self.streams, flags))])
