"""Agent's state_dict (the reference's checkpoint format, agent.py:26-36,106-107) and its exact-resume checkpoints: a mixin
over the flat buffers, layouts and optimiser that rainbow_amd.agent.Agent owns."""
import ctypes as C
import os

import torch

from . import _lib as L
from .params import _FlatAdam

_LAYERS = ("fc_h_v", "fc_h_a", "fc_z_v", "fc_z_a")


class AgentState:
    def state_dict(self):
        """Reference-compatible keys: convs.{0,2,4}.{weight,bias}, fc_*.{weight,bias}_{mu,sigma,epsilon}."""
        self._flush_noise()
        self.flush()
        sd = {}
        for name, _off, _shape in self._layout:
            sd[name] = self._view(self._params, name).clone()
            if name.endswith("bias_sigma"):     # nn.Module.state_dict order: a module's parameters, then its buffers (model.py:15-22)
                layer = name.split(".")[0]
                e_in = self._noise_view(self.noise, layer + ".eps_in")
                e_out = self._noise_view(self.noise, layer + ".eps_out")
                sd[layer + ".weight_epsilon"] = torch.outer(e_out, e_in)    # model.py:39
                sd[layer + ".bias_epsilon"] = e_out.clone()                 # model.py:40
        return sd

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict of the reference's DQN (agent.py:33): STRICT by default — missing or unexpected keys
        raise, as the reference's call does.  The [out, in] weight_epsilon buffers are rank-1 (model.py:39); the
        factorised vectors are recovered EXACTLY (see _recover_eps_in), so save -> load -> save is bit-identical."""
        self.flush()
        sd = dict(state_dict)
        if "conv1.weight" in sd:                                                           # agent.py:29-32
            for old, new in (("conv1.weight", "convs.0.weight"), ("conv1.bias", "convs.0.bias"),
                             ("conv2.weight", "convs.2.weight"), ("conv2.bias", "convs.2.bias"),
                             ("conv3.weight", "convs.4.weight"), ("conv3.bias", "convs.4.bias")):
                sd[new] = sd.pop(old)
        expected = [n for n, _o, _s in self._layout]
        for layer in _LAYERS:
            expected += [layer + ".weight_epsilon", layer + ".bias_epsilon"]
        missing = [k for k in expected if k not in sd]
        unexpected = [k for k in sd if k not in expected]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for DQN: missing key(s) %s; unexpected key(s) %s"
                               % (missing, unexpected))
        self._flush_noise()
        with torch.no_grad():
            for name, _off, shape in self._layout:
                if name not in sd:
                    continue
                t = sd[name]
                if tuple(t.shape) != tuple(shape):
                    raise RuntimeError("size mismatch for %s: %s vs %s" % (name, tuple(t.shape), shape))
                self._view(self._params, name).copy_(t.to(self.device, torch.float32))
            for layer in _LAYERS:
                if layer + ".bias_epsilon" not in sd or layer + ".weight_epsilon" not in sd:
                    continue
                e_out = sd[layer + ".bias_epsilon"].to(self.device, torch.float32)
                e_w = sd[layer + ".weight_epsilon"].to(self.device, torch.float32)
                self._noise_view(self.noise, layer + ".eps_in").copy_(self._recover_eps_in(e_w, e_out))
                self._noise_view(self.noise, layer + ".eps_out").copy_(e_out)

    @staticmethod
    def _recover_eps_in(e_w, e_out):
        """weight_epsilon = fl32(eps_out[i] * eps_in[k]) (model.py:39, torch.ger).  A single division e_w[j] / e_out[j] can
        land one ulp beside the true eps_in[k]; the true value is the neighbour that REPRODUCES the stored products.
        Candidates {q - ulp, q, q + ulp} of the quotient on the row of largest |eps_out| are scored against the 64 rows
        of largest |eps_out|; the best one per column wins (the true vector scores 0 mismatches by construction)."""
        order = torch.argsort(e_out.abs(), descending=True)
        j = int(order[0].item())
        if float(e_out[j]) == 0.0:
            return torch.zeros_like(e_w[0])
        q = e_w[j] / e_out[j]
        inf = torch.full_like(q, float("inf"))
        cands = torch.stack([torch.nextafter(q, -inf), q, torch.nextafter(q, inf)])       # [3, K]
        rows = order[:64]
        prod = e_out[rows][None, :, None] * cands[:, None, :]                              # [3, R, K] float32 products
        miss = (prod != e_w[rows][None, :, :]).sum(dim=1)                                  # [3, K]
        miss[1] = miss[1] * 2 - 1                                                          # ties prefer the quotient itself
        miss[0] *= 2
        miss[2] *= 2
        best = torch.argmin(miss, dim=0)
        return cands.gather(0, best[None, :])[0]

    # ------------------------------------------------------------------ exact resume
    def checkpoint(self, path=None):
        """Everything the learner needs to continue bit-for-bit: online / target parameters (a pending optimiser pass, which
        with target_tau > 0 moves the target too, has run before they are copied), target_tau, both noise buffers, Adam
        moments + step, the Philox (seed, epoch) of the noise generator, the pending-resample flag, the numbers of resets and recycles done
        (reset_parameters / recycle_dormant: the next one's draw) and the effective (horizon, discount) of set_horizon.  The reference's
        save() (weights only, agent.py:106-107) stays what main.py:182 calls; this is the superset a resumable run needs
        (main.py has no such thing: it restarts the optimiser).  Returns the dict; writes it with torch.save if `path`."""
        if not isinstance(self.optimiser, _FlatAdam):
            raise NotImplementedError("checkpoint() covers the library's own Adam (RAINBOW_AMD_FUSED_ADAM=1)")
        self.flush()
        self._sync_step()
        seed, epoch = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib, self._lib.rb_learner_get_rng(self._h, C.byref(seed), C.byref(epoch), self._stream()))
        st = self.optimiser.state[self._params]
        ck = dict(version=1, config=bytes(self._cfg), params=self._params.detach().cpu(), target_params=self._target_params.cpu(),
                  noise=self.noise.cpu(), target_noise=self.target_noise.cpu(), exp_avg=st["exp_avg"].cpu(),
                  exp_avg_sq=st["exp_avg_sq"].cpu(), adam_step=float(st["step"]), rng_seed=int(seed.value),
                  rng_epoch=int(epoch.value), noise_pending=bool(self._noise_pending), training=bool(self.training),
                  target_tau=float(self._target_tau), resets=int(self.resets), recycles=int(self.recycles),
                  horizon=int(self.horizon), discount=float(self.discount))
        if path is not None:
            torch.save(ck, path)
        return ck

    def restore(self, ck):
        """Inverse of checkpoint(): `ck` is the dict or a path."""
        if not isinstance(self.optimiser, _FlatAdam):     # before anything is overwritten
            raise NotImplementedError("restore() covers the library's own Adam (RAINBOW_AMD_FUSED_ADAM=1)")
        self.flush()
        if not isinstance(ck, dict):
            ck = torch.load(ck, map_location="cpu")
        if ck.get("version") != 1 or ck["config"] != bytes(self._cfg):
            raise RuntimeError("checkpoint does not match this Agent's configuration")
        with torch.no_grad():
            self._params.copy_(ck["params"])
            self._target_params.copy_(ck["target_params"])
            self.noise.copy_(ck["noise"])
            self.target_noise.copy_(ck["target_noise"])
            st = self.optimiser.state[self._params]
            st["exp_avg"].copy_(ck["exp_avg"])
            st["exp_avg_sq"].copy_(ck["exp_avg_sq"])
            st["step"].fill_(ck["adam_step"])
            if self._step_dev is not None:
                self._step_dev.fill_(int(ck["adam_step"]))
        L.check(self._lib, self._lib.rb_learner_set_rng(self._h, int(ck["rng_seed"]), int(ck["rng_epoch"]), self._stream()))
        self._noise_pending = bool(ck["noise_pending"])
        self.training = bool(ck["training"])
        self._noise_jobs = {}                       # (the cached jobs carry the old seed: _noise_job re-queries them)
        if "target_tau" in ck:                      # (checkpoints from before the EMA target carry none: the agent keeps its own)
            self.target_tau = ck["target_tau"]
        self.resets = int(ck.get("resets", 0))      # (none before reset_parameters existed: no reset has been done)
        self.recycles = int(ck.get("recycles", 0))  # (likewise for recycle_dormant: the next recycle's draw)
        # (none before set_horizon existed: the horizon and discount of construction, which `config` has just been compared with)
        self.set_horizon(ck.get("horizon", self.n), ck.get("discount", self._cfg.discount))

    def save(self, path, name="model.pth"):
        torch.save(self.state_dict(), os.path.join(path, name))
