"""Agent's dormant-unit diagnostic and targeted reset (ReDo: Sokar, Agarwal, Castro, Evci, "The Dormant Neuron Phenomenon in
Deep RL", ICML 2023): dormant_stats and recycle_dormant.  A mixin over the learner handle rainbow_amd.agent.Agent owns;
include/rainbow_hip.h has the contracts (rb_learner_unit_layout, rb_learner_unit_activity, rb_learner_dormant_mask,
rb_learner_recycle_units).  Nothing here runs unless it is called."""
import ctypes as C
import math

import torch

from . import _lib as L
from ._util import u64_pair

REDO_TAU = 0.1          # the threshold the paper recycles at


class AgentRedo:
    _unit_layers = None

    def unit_layers(self):
        """([layer names], [units per layer]) in the library's order: the conv layers, fc_h_v, fc_h_a."""
        if self._unit_layers is None:
            n, units = C.c_int32(0), (C.c_int32 * 5)()
            L.check(self._lib, self._lib.rb_learner_unit_layout(C.byref(self._cfg), C.byref(n), units))
            names = ["convs.%d" % (2 * k) for k in range(n.value - 2)] + ["fc_h_v", "fc_h_a"]
            self._unit_layers = (names, [int(u) for u in units[:n.value]])
        return self._unit_layers

    def _redo_tau_of(self, tau, who):
        tau = float(REDO_TAU if self._redo_tau is None else self._redo_tau) if tau is None else float(tau)
        if not (tau >= 0.0 and math.isfinite(tau)):       # (also NaN)
            raise ValueError("%s: tau must be finite and >= 0, got %r" % (who, tau))
        return tau

    def _measure_dormant(self, mem, batches, tau, who, scores):
        """The activity of `batches` batches drawn from mem and the mask at tau, all on the current stream, nothing synchronised.
        -> (mask u8 [U], counts i32 [n_layers], scores f32 [U] or None) as device tensors."""
        batches = int(batches)
        if batches < 1:
            raise ValueError("%s: batches must be >= 1, got %d" % (who, batches))
        units = self.unit_layers()[1]
        U, B, d = sum(units), self.batch_size, self.device
        act = torch.empty(U, dtype=torch.float64, device=d)
        mask = torch.empty(U, dtype=torch.uint8, device=d)
        counts = torch.empty(len(units), dtype=torch.int32, device=d)
        sc = torch.empty(U, dtype=torch.float32, device=d) if scores else None
        stream = self._stream()
        with torch.cuda.device(d):
            for i in range(batches):
                o = mem.sample_device(B, gather=True, stream=stream)        # (priorities are never updated from these draws)
                L.check(self._lib, self._lib.rb_learner_unit_activity(self._h, o["states"].data_ptr(), 1 if i else 0, act.data_ptr(), stream))
                self._update_pending = False              # (the library ran a pending optimiser pass first)
            L.check(self._lib, self._lib.rb_learner_dormant_mask(self._h, act.data_ptr(), tau, mask.data_ptr(), counts.data_ptr(),
                                                                sc.data_ptr() if scores else None, stream))
        return mask, counts, sc

    def dormant_stats(self, mem, batches=1, tau=None):
        """The share of dormant units per layer on `batches` batches drawn from `mem` (mem.sample_device(B, gather=True): it advances
        mem's draw state like any draw and never updates priorities): a unit is dormant when its mean activation is at most tau
        times its layer's mean (tau defaults to args.redo_tau, else 0.1).  Changes nothing in the agent; synchronises once.
        Returns {"layers": [names], "dormant": [per layer], "units": [per layer], "fraction": total share, "scores": float32 [U]}."""
        tau = self._redo_tau_of(tau, "dormant_stats")
        _mask, counts, scores = self._measure_dormant(mem, batches, tau, "dormant_stats", True)
        names, units = self.unit_layers()
        dormant = [int(c) for c in counts.cpu().numpy()]  # (the copy synchronises)
        return {"layers": list(names), "dormant": dormant, "units": list(units), "fraction": sum(dormant) / float(sum(units)),
                "scores": scores.cpu().numpy()}

    def recycle_dormant(self, mem, tau=None, batches=1, target=False, rng=None):
        """ReDo's targeted reset (rb_learner_recycle_units) behind the same measurement, all in stream order with NO
        synchronisation: every dormant unit gets fresh incoming weights and zeroed outgoing ones (weight_sigma: its initial
        constant), so the eval-mode function of the network does not change; both Adam moments of the written elements — those of
        whichever optimiser is active — are cleared.  target=False is the paper's rule (the target follows by EMA or the next
        sync); True writes the same values into the target.  rng = (seed, draw) keys the draw and defaults to (args.seed or 0,
        self.recycles): replicas that pass the same pair draw the same weights, and a run resumed from checkpoint() repeats them bit
        for bit.  self.last_recycle_counts keeps the per-layer dormant counts as a device tensor (reading it synchronises);
        self.recycles counts the recycles done."""
        tau = self._redo_tau_of(tau, "recycle_dormant")
        mask, counts, _ = self._measure_dormant(mem, batches, tau, "recycle_dormant", False)
        seed, draw = u64_pair((self._reset_seed, self.recycles) if rng is None else rng)
        st = self.optimiser.state.get(self._params, {})   # (torch's own Adam has no state before its first step: no moments to clear)
        m, v = st.get("exp_avg"), st.get("exp_avg_sq")
        with torch.cuda.device(self.device):
            L.check(self._lib, self._lib.rb_learner_recycle_units(
                self._h, mask.data_ptr(), self._noisy_std, seed, draw, 1 if target else 0,
                m.data_ptr() if m is not None else None, v.data_ptr() if v is not None else None, self._stream()))
        self._update_pending = False                      # (the library ran a pending pass first)
        self._keep["redo_mask"] = mask                    # (alive until the stream has consumed it)
        self.last_recycle_counts = counts
        self.recycles += 1

    def dormant_fraction(self):
        """The total dormant share the last recycle_dormant found (reads last_recycle_counts: synchronises); None before the first."""
        if self.last_recycle_counts is None:
            return None
        return float(self.last_recycle_counts.sum().item()) / float(sum(self.unit_layers()[1]))
