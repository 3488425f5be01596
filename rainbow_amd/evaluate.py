"""Per-episode returns of S environment streams, recorded on the device (librainbow_hip.so rb_tally_*; the rules are in
include/rainbow_hip.h, "episode tally").

`EpisodeTally(streams, episodes, device)` is what test.py:19-34 keeps as `T_rewards`, for a vectorised environment: every
round's `rewards` / `nonterminals` device vectors go to `step`, which is one launch on the current stream and never
synchronises; stream s records its first `episodes // S + (s < episodes % S)` episodes and ignores later ones, so `episodes`
episodes are spread evenly over the streams whatever their lengths.  `remaining()` and `result()` synchronise.
rainbow_amd.loop.evaluate_vec is the evaluation loop built on it."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._util import current_stream_handle


def stream_quotas(streams, episodes):
    """Episodes each stream records: int array [streams] that sums to `episodes`."""
    s = np.arange(int(streams))
    return int(episodes) // int(streams) + (s < int(episodes) % int(streams)).astype(np.int64)


class EpisodeTally:
    _h = None                  # (close() is safe on an object whose construction failed early)

    def __init__(self, streams, episodes, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rainbow_amd.evaluate.EpisodeTally lives on the device: got %s" % self.device)
        self._lib = L.load()
        self.streams, self.episodes = int(streams), int(episodes)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self._lib, self._lib.rb_tally_create(C.byref(self._h), self.streams, self.episodes))

    def close(self):
        if self._h:
            self._lib.rb_tally_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return current_stream_handle(self.device)

    def reset(self):
        """Start over (asynchronous)."""
        L.check(self._lib, self._lib.rb_tally_reset(self._h, self._stream()))

    def step(self, rewards, nonterminals):
        """rewards f32 [S], nonterminals u8 / bool [S] (0 = the step ended the episode), device tensors.  One launch, no
        synchronisation."""
        if rewards.dtype != torch.float32 or rewards.device != self.device or not rewards.is_contiguous():
            rewards = rewards.to(device=self.device, dtype=torch.float32).contiguous()
        if nonterminals.dtype != torch.uint8 or nonterminals.device != self.device or not nonterminals.is_contiguous():
            nonterminals = nonterminals.to(device=self.device, dtype=torch.uint8).contiguous()
        if rewards.numel() != self.streams or nonterminals.numel() != self.streams:
            raise ValueError("EpisodeTally.step: %d rewards and %d nonterminals for %d streams"
                             % (rewards.numel(), nonterminals.numel(), self.streams))
        self._keep = (rewards, nonterminals)          # inputs stay alive until the stream has consumed them
        rc = self._lib.rb_tally_step(self._h, rewards.data_ptr(), nonterminals.data_ptr(), self._stream())
        if rc != 0:
            L.check(self._lib, rc)

    def remaining(self):
        """Episodes still to be recorded (0 = done).  SYNCHRONISES the stream."""
        n = C.c_int32(-1)
        L.check(self._lib, self._lib.rb_tally_remaining(self._h, C.byref(n), self._stream()))
        return int(n.value)

    def result(self):
        """(returns f32 [episodes], lengths i32 [episodes], streams i32 [episodes]) as numpy arrays, stream-major: stream 0's
        episodes in the order they ended, then stream 1's, ...  Unfilled slots are (NaN, 0).  SYNCHRONISES the stream."""
        returns = np.empty(self.episodes, dtype=np.float32)
        lengths = np.empty(self.episodes, dtype=np.int32)
        streams = np.empty(self.episodes, dtype=np.int32)
        L.check(self._lib, self._lib.rb_tally_read(self._h, returns.ctypes.data, lengths.ctypes.data, streams.ctypes.data,
                                                   self._stream()))
        return returns, lengths, streams
