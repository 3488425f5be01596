"""Agent's two loss-of-plasticity read-outs beside the dormant-unit share (agent_redo.py): feature_rank — srank (Kumar et al.
2021), the feature rank of Lyle et al. 2022 and the effective rank of the learned features — and tensor_norms, the per-tensor
weight norm, gradient norm and online-target distance.  A mixin over the learner handle rainbow_amd.agent.Agent owns;
include/rainbow_hip.h has the contracts (rb_learner_feature_dim, rb_learner_features, rb_gram_f64, rb_learner_tensor_norms), the
spectrum is rainbow_amd/feature_rank.py.  Nothing here runs unless it is called; both synchronise once."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .feature_rank import spectrum_metrics

FEATURE_LAYERS = {"hidden": 0, "conv": 1}       # RB_FEATURES_HIDDEN, RB_FEATURES_CONV
RANK_MAX_SAMPLES = 4096                         # rb_gram_f64's largest n


class AgentRank:
    last_feature_rank = None

    def feature_dim(self, layer="hidden"):
        """The dimension of a state's features: "hidden" = 2 * hidden (the post-ReLU [fc_h_v | fc_h_a] row), "conv" = the last
        conv layer's flattened output."""
        if layer not in FEATURE_LAYERS:
            raise ValueError("feature_rank: layer must be one of %s, got %r" % (sorted(FEATURE_LAYERS), layer))
        d = C.c_int32(0)
        L.check(self._lib, self._lib.rb_learner_feature_dim(C.byref(self._cfg), FEATURE_LAYERS[layer], C.byref(d)))
        return int(d.value)

    def feature_rank(self, mem, batches=8, layer="hidden", eps=0.01, delta=0.01):
        """The rank of the online network's features on `batches` batches drawn from `mem` (mem.sample_device(B, gather=True), as
        dormant_stats draws: it advances mem's draw state like any draw and never updates priorities).  The eval-mode forward of
        every batch is captured into one Phi [batches * B, ld]; ONE launch forms K = Phi Phi^T in double (rb_gram_f64); K is copied
        to the host once — the only synchronisation — and feature_rank.spectrum_metrics reads the spectrum off it.  Returns its
        dict (singular_values, feature_rank, srank, effective_rank, mean_sq_norm, top_share, finite) plus `layer`, `samples` =
        batches * B and `dim`; self.last_feature_rank keeps it.  Changes nothing in the agent: parameters, target, moments,
        gradients, noise and the step counter stay bit for bit (a pending optimiser pass runs first, as before any read).
        batches < 1, batches * B > 4096 or an unknown layer raise ValueError."""
        d = self.feature_dim(layer)
        batches, B = int(batches), int(self.batch_size)
        if batches < 1:
            raise ValueError("feature_rank: batches must be >= 1, got %d" % batches)
        n = batches * B
        if n > RANK_MAX_SAMPLES:
            raise ValueError("feature_rank: batches * batch_size = %d samples, at most %d" % (n, RANK_MAX_SAMPLES))
        ld = (d + 3) // 4 * 4
        dev = self.device
        phi = torch.empty((n, ld), dtype=torch.float32, device=dev)
        K = torch.empty((n, n), dtype=torch.float64, device=dev)
        stream = self._stream()
        with torch.cuda.device(dev):
            for i in range(batches):
                o = mem.sample_device(B, gather=True, stream=stream)        # (priorities are never updated from these draws)
                L.check(self._lib, self._lib.rb_learner_features(self._h, o["states"].data_ptr(), FEATURE_LAYERS[layer],
                                                                 phi[i * B].data_ptr(), ld, stream))
                self._update_pending = False              # (the library ran a pending optimiser pass first)
            L.check(self._lib, self._lib.rb_gram_f64(phi.data_ptr(), n, d, ld, K.data_ptr(), stream))
        out = spectrum_metrics(K.cpu().numpy(), n, d, eps=eps, delta=delta)    # (the copy synchronises)
        out.update(layer=layer, samples=n, dim=d)
        self.last_feature_rank = out
        return out

    def tensor_norms(self, grads=True, target=True):
        """Per named tensor of the parameter layout, as float64 arrays in its order: {"names", "param_norm" (l2), "param_absmax",
        "target_dist" (l2 distance online - target; None with target=False), "grad_norm" (l2 of the gradient the last learn() left;
        None with grads=False)}.  Two launches per buffer (rb_learner_tensor_norms), one copy, which synchronises.  A NaN in a
        tensor shows as NaN in that tensor's entries only.  A pending optimiser pass runs first."""
        names = [n for n, _o, _s in self._layout]
        T = len(names)
        out = torch.empty((2, T, 3), dtype=torch.float64, device=self.device)
        stream = self._stream()
        with torch.cuda.device(self.device):
            L.check(self._lib, self._lib.rb_learner_tensor_norms(self._h, self._params.data_ptr(),
                                                                 self._target_params.data_ptr() if target else None, out[0].data_ptr(), stream))
            self._update_pending = False                  # (the library ran a pending pass first)
            if grads:
                L.check(self._lib, self._lib.rb_learner_tensor_norms(self._h, self._grads.data_ptr(), None, out[1].data_ptr(), stream))
        h = out.cpu().numpy()                             # (the copy synchronises)
        return {"names": names, "param_norm": np.sqrt(h[0, :, 0]), "param_absmax": h[0, :, 2].copy(),
                "target_dist": np.sqrt(h[0, :, 1]) if target else None, "grad_norm": np.sqrt(h[1, :, 0]) if grads else None}
