"""The flat parameter buffer: its layout, the reference's initial distributions over it, and the optimiser that steps it."""
import ctypes as C
import math
import weakref

import numpy as np
import torch

from . import _lib as L


def _query_layout(lib, cfg, fn):
    n = C.c_int32(0)
    L.check(lib, fn(C.byref(cfg), None, C.byref(n)))
    descs = (L.TensorDesc * n.value)()
    L.check(lib, fn(C.byref(cfg), descs, C.byref(n)))
    return [(d.name.decode(), int(d.offset), tuple(d.shape[i] for i in range(d.ndim))) for d in descs[:n.value]]


def init_parameters_flat(layout, n_params, noisy_std):
    """The reference's initial parameter distributions over the flat layout (a CPU float32 tensor; `layout` = the
    (name, offset, shape) triples of rb_learner_param_layout): Conv2d's default U(+-1/sqrt(fan_in)) for weight and bias
    (model.py:56-62, torch.nn.Conv2d.reset_parameters), and NoisyLinear.reset_parameters (model.py:25-30):
    weight_mu, bias_mu ~ U(+-1/sqrt(in)); weight_sigma = std_init/sqrt(in); bias_sigma = std_init/sqrt(out).
    Drawn from torch's CPU generator."""
    flat = torch.zeros(n_params, dtype=torch.float32)
    shapes = dict((n, s) for n, _o, s in layout)
    fan_in = None
    for name, off, shape in layout:
        numel = int(np.prod(shape))
        if name.startswith("convs"):
            if name.endswith("weight"):
                fan_in = int(np.prod(shape[1:]))
            bound = 1.0 / math.sqrt(fan_in)                   # the bias of a layer follows its weight in the layout
            flat[off:off + numel] = torch.empty(numel).uniform_(-bound, bound)
        else:
            kind = name.split(".")[1]
            out_f, in_f = shapes[name.split(".")[0] + ".weight_mu"]
            if kind in ("weight_mu", "bias_mu"):
                bound = 1.0 / math.sqrt(in_f)                 # model.py:26,28
                flat[off:off + numel] = torch.empty(numel).uniform_(-bound, bound)
            elif kind == "weight_sigma":
                flat[off:off + numel] = noisy_std / math.sqrt(in_f)      # model.py:27
            else:
                flat[off:off + numel] = noisy_std / math.sqrt(out_f)     # model.py:29
    return flat


def takes_plain_adam(optimiser):
    """Whether the library's clip + Adam pass can take this optimiser's step: the library's own _FlatAdam in the reference's
    configuration (rb_learner_clip_adam implements plain Adam: no amsgrad, no weight decay, no maximize)."""
    if not isinstance(optimiser, _FlatAdam):
        return False
    g = optimiser.param_groups[0]
    return not (g["amsgrad"] or g["weight_decay"] != 0 or g["maximize"])


class _FlatAdam(torch.optim.Adam):
    """torch.optim.Adam over the single flat parameter tensor (agent.py:46).  The state is ordinary Adam state
    (step / exp_avg / exp_avg_sq, so state_dict() and load_state_dict() work as usual), but step() runs the library's
    one-pass kernel (rb_learner_clip_adam), optionally with clip_grad_norm_ folded in (max_norm)."""

    def __init__(self, agent, **kw):
        super().__init__([agent._params], **kw)
        self._agent = weakref.ref(agent)
        p = agent._params
        self.state[p] = dict(step=torch.tensor(0.0, dtype=torch.float32),
                             exp_avg=torch.zeros_like(p, memory_format=torch.preserve_format),
                             exp_avg_sq=torch.zeros_like(p, memory_format=torch.preserve_format))

    def state_dict(self):
        ag = self._agent()
        if ag is not None:
            ag.flush()               # a deferred optimiser pass writes the moments
            ag._sync_step()          # the device counts the steps (deferred pass): refresh the host mirror first
        return super().state_dict()

    def load_state_dict(self, state_dict):
        ag = self._agent()
        if ag is not None:
            ag.flush()
        super().load_state_dict(state_dict)
        if ag is not None and ag._step_dev is not None:      # the device-resident step number follows the loaded one
            ag._step_dev.fill_(int(float(self.state[ag._params]["step"])))

    @torch.no_grad()
    def step(self, closure=None, max_norm=float("inf")):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.step_direct(max_norm)
        return loss

    def count_step(self, ag):
        """Counts one step on the host mirror and returns (param group, state, `step` word for the library).  The state is
        looked up every step: load_state_dict replaces these tensors.  With a device-resident step counter (deferred optimiser
        pass) the word is 0: the kernel reads the counter and forms the bias corrections itself, the host copy only mirrors
        it (Agent._sync_step refreshes it)."""
        g = self.param_groups[0]
        st = self.state[g["params"][0]]
        st["step"] += 1
        return g, st, (0 if ag._step_dev is not None else int(st["step"].item()))

    def step_direct(self, max_norm=float("inf"), stream=None, defer=False):
        """What step() does, callable without torch.optim's step wrapper (profiler record + hook dispatch: ~20 us per call,
        a tenth of a batch-32 learn step's host time).  Agent.learn uses this; step() stays for API compatibility."""
        ag = self._agent()
        if ag is None:
            raise RuntimeError("the Agent that owns this optimiser is gone")
        if not takes_plain_adam(self):
            raise NotImplementedError("rb_learner_clip_adam implements plain Adam (the reference's configuration)")
        g, st, step = self.count_step(ag)
        b1, b2 = g["betas"]
        fn = ag._lib.rb_learner_clip_adam_deferred if defer else ag._lib.rb_learner_clip_adam
        rc = fn(
            ag._h, float(max_norm), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), float(g["lr"]), float(b1),
            float(b2), float(g["eps"]), step,
            ag._norm_buf.data_ptr() if math.isfinite(max_norm) else None, ag._stream() if stream is None else stream)
        if rc != 0:
            L.check(ag._lib, rc)
