"""Agent's device-side diagnostics: the ring of per-step records (track_stats / read_stats) and the held-out loss
(evaluate_loss).  A mixin over the learner handle rainbow_amd.agent.Agent owns; include/rainbow_hip.h has the contracts
(rb_step_stats_t, rb_learner_set_stats, rb_learner_eval_loss).  Everything is off until asked for."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

# numpy view of rb_step_stats_t
STEP_STATS_DTYPE = np.dtype([(name, {C.c_int64: np.int64, C.c_int32: np.int32, C.c_float: np.float32}[ct])
                             for name, ct in L.StepStats._fields_])
assert STEP_STATS_DTYPE.itemsize == C.sizeof(L.StepStats) == 64
STEP_STATS_FIELDS = tuple(n for n in STEP_STATS_DTYPE.names if n != "reserved")


def records_to_dict(rec, dropped=0):
    """A structured array of rb_step_stats_t as {field: array} plus `dropped`."""
    out = {n: np.ascontiguousarray(rec[n]) for n in STEP_STATS_FIELDS}
    out["dropped"] = int(dropped)
    return out


class AgentStats:
    _stats_ring = None

    def track_stats(self, capacity):
        """Keep one record per learn() in a device ring of `capacity` records (rb_learner_set_stats: one extra launch at the end of
        every learn step, no synchronisation, nothing read by the host until read_stats()).  capacity 0 / None switches the
        records off again: every launch is then what it is without them.  Records not yet read are dropped by a new call.
        A call that replaces or drops a ring synchronises the device first: learn steps already queued still write to the old
        ring, on whichever stream they were given.  A captured graph bakes the ring's address in: set the ring BEFORE capturing and
        keep it until the graph is gone."""
        capacity = int(capacity or 0)
        if capacity < 0:
            raise ValueError("track_stats: capacity must be >= 0, got %d" % capacity)
        if self._stats_ring is not None:
            torch.cuda.synchronize(self.device)       # queued steps have written their records before the old tensors go
        if capacity == 0:
            if self._stats_ring is not None:
                L.check(self._lib, self._lib.rb_learner_set_stats(self._h, None, 0, None))
            self._stats_ring = self._stats_count = None
            return
        # (never zeroed on purpose: the kernel writes every byte of a record)
        ring = torch.empty(capacity * STEP_STATS_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._lib, self._lib.rb_learner_set_stats(self._h, ring.data_ptr(), capacity, count.data_ptr()))
        self._stats_ring, self._stats_count, self._stats_cap, self._stats_read = ring, count, capacity, 0

    def read_stats(self):
        """The records written since the last read, oldest first, as a dict of numpy arrays (one entry per field of
        rb_step_stats_t) plus `dropped`, the number of records that were overwritten before they were read.  Synchronises the
        current stream (the one the learn steps went to); None when track_stats is off."""
        if self._stats_ring is None:
            return None
        torch.cuda.current_stream(self.device).synchronize()
        count = int(self._stats_count.item())
        ring = self._stats_ring.cpu().numpy().view(STEP_STATS_DTYPE)
        first = max(self._stats_read, count - self._stats_cap)
        dropped = first - self._stats_read
        rec = ring[[i % self._stats_cap for i in range(first, count)]]
        self._stats_read = count
        return records_to_dict(rec, dropped)

    def evaluate_loss(self, mem, batches=1, unit_uniforms=None):
        """The loss of the current networks on `batches` batches drawn from `mem` — typically a held-out validation memory —
        without learning from them (rb_learner_eval_loss: the learn step's forwards and head in eval mode, nothing else).  Each
        batch is mem.sample_device(self.batch_size, unit_uniforms, gather=True): it advances mem's draw state like any draw
        (injected uniforms, a float64 device tensor [attempts, B], make it repeatable) and never updates priorities.  Raises the
        ValueError of learn() when mem's horizon or discount differ from the agent's, and RuntimeError when a draw found no valid
        batch (a memory too small for the batch: its stacks would be stale; checked once, after the final synchronise).
        Returns a dict: the mean over the batches of every float field of rb_step_stats_t (loss_mean, q_mean, td_abs_mean, ...; loss_max is the maximum), `batches`, and
        `loss`, the per-sample losses as a float32 array [batches, B].  Synchronises the current stream."""
        if mem.horizon != self.horizon or mem.discount != self.discount:
            raise ValueError("Agent.evaluate_loss: the memory's horizon and discount (%d, %r) differ from the agent's (%d, %r): call "
                             "set_horizon on both with the same values" % (mem.horizon, mem.discount, self.horizon, self.discount))
        batches = int(batches)
        if batches < 1:
            raise ValueError("evaluate_loss: batches must be >= 1, got %d" % batches)
        B, d = self.batch_size, self.device
        loss = torch.empty(batches, B, dtype=torch.float32, device=d)
        rec = torch.empty(batches * STEP_STATS_DTYPE.itemsize, dtype=torch.uint8, device=d)
        stream = self._stream()
        failed_before = mem.failed_samples()
        for i in range(batches):
            o = mem.sample_device(B, unit_uniforms, gather=True, stream=stream)
            with torch.cuda.device(d):
                L.check(self._lib, self._lib.rb_learner_eval_loss(
                    self._h, o["states"].data_ptr(), o["next_states"].data_ptr(), o["actions"].data_ptr(), o["returns"].data_ptr(),
                    o["nonterminals"].data_ptr(), loss[i].data_ptr(), rec.data_ptr() + i * STEP_STATS_DTYPE.itemsize, stream))
            self._update_pending = False              # (the library ran a pending optimiser pass first)
        r = rec.cpu().numpy().view(STEP_STATS_DTYPE)   # (the copy synchronises)
        failed = mem.failed_samples() - failed_before  # (pinned host word the sampler writes: exact now that the stream is drained)
        if failed:
            mem.reset_failed_samples()
            raise RuntimeError("Agent.evaluate_loss: %d of %d draws found no valid batch in %d attempts (memory too small for batch "
                               "%d?): the loss of those batches would be that of stale stacks" % (failed, batches, mem.MAX_ATTEMPTS, B))
        out = {n: float(r[n].max() if n == "loss_max" else r[n].astype(np.float64).mean())
               for n in STEP_STATS_FIELDS if STEP_STATS_DTYPE[n] == np.float32 and n != "grad_norm"}
        out["batches"] = batches
        out["loss"] = loss.cpu().numpy()
        return out
