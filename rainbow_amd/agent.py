"""Drop-in `Agent` for the reference's main.py / test.py (replaces /root/reference/agent.py + model.py).

Same constructor and methods as the reference class (agent.py:12-118).  The networks are not
nn.Modules: online / target parameters, gradients and factorised noise are flat float32 HBM
buffers (torch tensors used purely as memory owners) and every forward / backward kernel is
hand-written HIP behind librainbow_hip.so, the clip + Adam update included (`self.optimiser` is a
torch.optim.Adam whose step() runs the library's one-pass kernel, agent.py:46,97-98); PyTorch-ROCm
owns memory, streams and torch.distributed.

learn(mem):  rainbow_amd.memory.ReplayMemory  -> fully device-resident step, no host sync:
                 sample (+ noise) -> 3 forwards + projection + loss + backward (+ priority
                 write-back) -> [RCCL all-reduce] -> global-norm clip + Adam
             any other object with the reference's sample()/update_priorities() -> compat path.

Multi-GPU (BASELINE config 5): one process per GPU, identical parameters, each replica owns its
replay; between backward and clip every replica obtains the mean gradient of the global batch
(rainbow_amd/dist.py: all-gather of the FC gradient FACTORS + all-reduce of the conv gradients by
default, or one all-reduce of the flat buffer).  Enabled automatically when torch.distributed is
initialised.

This module: construction, the mode flags, the parameter-space properties and operations, and the noise state.  The learn step
is agent_learn.py, the act / evaluate paths agent_act.py, state_dict and checkpoints agent_state.py, the step records and the
held-out loss agent_stats.py, the dormant-unit diagnostic and recycling agent_redo.py, the feature rank and the per-tensor norms
agent_rank.py; the flat layout, its initial distributions and the optimiser are params.py.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import dist as rdist
from ._util import current_stream_handle, u64_pair
from .agent_act import AgentAct
from .agent_learn import AgentLearn
from .agent_rank import AgentRank
from .agent_state import AgentState
from .agent_redo import AgentRedo
from .agent_stats import AgentStats
from .params import _FlatAdam, _query_layout, init_parameters_flat


class Agent(AgentLearn, AgentAct, AgentState, AgentStats, AgentRedo, AgentRank):
    _h = None                  # (so that __del__ is safe on an object whose construction failed early)

    def __init__(self, args, env):
        self.device = torch.device(args.device)
        if self.device.type != "cuda":
            raise RuntimeError("rainbow_amd.Agent runs on MI355X: args.device must be a cuda (ROCm) device, got %s"
                               % self.device)
        self._lib = L.load()
        self.action_space = env.action_space()                       # agent.py:14
        self.atoms = args.atoms
        self.Vmin, self.Vmax = args.V_min, args.V_max
        self.support = torch.linspace(args.V_min, args.V_max, self.atoms).to(device=self.device)   # agent.py:18
        self.delta_z = (args.V_max - args.V_min) / (self.atoms - 1)
        self.batch_size = args.batch_size
        self.n = args.multi_step                                     # n_max: what the learner handle is created with
        self.discount = args.discount
        self.horizon = int(args.multi_step)                          # the effective horizon (set_horizon)
        self.norm_clip = args.norm_clip
        self.training = True

        arch = getattr(args, "architecture", "canonical")
        self._cfg = L.LearnerConfig(batch=int(args.batch_size), atoms=int(args.atoms), actions=int(self.action_space),
                                    history=int(args.history_length), hidden=int(args.hidden_size),
                                    architecture=0 if arch == "canonical" else 1, multi_step=int(args.multi_step),
                                    v_min=float(args.V_min), v_max=float(args.V_max), discount=float(args.discount))
        self._defer_update = False
        self._update_pending = False
        self._hosted_job = L.NoiseJob()
        n_params, n_noise = C.c_int64(0), C.c_int64(0)
        L.check(self._lib, self._lib.rb_learner_sizes(C.byref(self._cfg), C.byref(n_params), C.byref(n_noise)))
        self._layout = _query_layout(self._lib, self._cfg, self._lib.rb_learner_param_layout)
        self._noise_layout = _query_layout(self._lib, self._cfg, self._lib.rb_learner_noise_layout)
        d = self.device
        self._params = torch.zeros(n_params.value, dtype=torch.float32, device=d)          # online, flat
        self._target_params = torch.zeros(n_params.value, dtype=torch.float32, device=d)
        self._grads = torch.zeros(n_params.value, dtype=torch.float32, device=d)
        self.noise = torch.zeros(n_noise.value, dtype=torch.float32, device=d)
        self.target_noise = torch.zeros(n_noise.value, dtype=torch.float32, device=d)
        self._h = C.c_void_p()
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        with torch.cuda.device(d):
            L.check(self._lib, self._lib.rb_learner_create(
                C.byref(self._h), C.byref(self._cfg), self._params.data_ptr(), self._target_params.data_ptr(),
                self._grads.data_ptr(), self.noise.data_ptr(), self.target_noise.data_ptr(), seed))

        self._init_parameters(float(getattr(args, "noisy_std", 0.1)))
        self._noise_pending = False
        self._noise_rows, self._noise_rows_drawn = None, 0           # reset_noise_rows: one noise sample per row
        self._keep = {}                                              # injected operands, alive until the stream has consumed them
        self.reset_noise()                                           # NoisyLinear.__init__ (model.py:23)
        if getattr(args, "model", None):                             # agent.py:26-36
            if os.path.isfile(args.model):
                # load_state_dict restores the epsilon buffers of the checkpoint too (they are registered buffers,
                # model.py:19,22): the noise drawn above is overwritten, exactly as in the reference
                self.load_state_dict(torch.load(args.model, map_location="cpu"))
                print("Loading pretrained model: " + args.model)
            else:
                raise FileNotFoundError(args.model)
        self.update_target_net()                                     # agent.py:41

        self._params.requires_grad_(True)
        self._params.grad = self._grads
        # (hipGraph replay of the step was built in rounds 1-3 and measured 4.5 % SLOWER than eager launches on this platform
        # at this launch count, DESIGN.md §6: removed)
        self._step_dev = None
        kw = dict(lr=args.learning_rate, eps=args.adam_eps)
        if os.environ.get("RAINBOW_AMD_FUSED_ADAM", "1") != "1":     # k_clip_scale + PyTorch's own (fused) Adam
            try:
                self.optimiser = torch.optim.Adam([self._params], fused=True, **kw)
            except (TypeError, RuntimeError):
                self.optimiser = torch.optim.Adam([self._params], **kw)
        else:
            # RAINBOW_AMD_DEFER_UPDATE (default on): learn() leaves its clip + Adam pass pending
            # and the NEXT learn()'s sampler launch hosts it (include/rainbow_hip.h RB_LEARNER_DEFER_UPDATE) — anything
            # else that touches the parameters runs it first (the library's entry points do so themselves; the public
            # tensors `params`, `grads`, `_norm` and the optimiser state go through flush()).  Needs the device-resident
            # step number (rb_learner_set_step_counter: the learn call increments it, the pass reads it).
            self._defer_update = os.environ.get("RAINBOW_AMD_DEFER_UPDATE", "1") == "1"
            if self._defer_update:
                self._step_dev = torch.zeros(1, dtype=torch.int64, device=d)
                L.check(self._lib, self._lib.rb_learner_set_step_counter(self._h, self._step_dev.data_ptr()))
            self.optimiser = _FlatAdam(self, **kw)                   # agent.py:46
        self._noise_jobs = {}
        self._zero_copy_ok = None
        # the whole step as ONE C call (rb_learner_train_step) when nothing needs the interpreter in between
        self._one_call = os.environ.get("RAINBOW_AMD_ONE_CALL", "1") == "1"
        self._ts = self._ts_mem = self._ts_out = None
        self._sink_mem = self._sink_idx = None                       # the memory and index buffer the priority sink points at
        self._sink_watched = set()
        # priority write-back as one extra workgroup of the learner's backward launch (see rb_learner_set_priority_sink)
        self._fuse_update = True
        self._loss = torch.zeros(self.batch_size, dtype=torch.float32, device=d)
        self._norm_buf = torch.zeros(1, dtype=torch.float32, device=d)
        self._act_pin = torch.zeros(2 * self.batch_size, dtype=torch.int32).pin_memory()     # written by the device
        self._q_pin = torch.zeros(2 * self.batch_size, dtype=torch.float32).pin_memory()
        self._act_np, self._q_np = self._act_pin.numpy(), self._q_pin.numpy()
        # the single-state path (act / evaluate_q): (action, q) as ONE 8-byte pinned pair — the head stores both with a single
        # system-scope store (csrc/act_head.h rb_head_act_body) instead of q, a fence, then the action
        self._aq_pin = torch.zeros(2, dtype=torch.int32).pin_memory()
        self._aq_act = self._aq_pin.numpy()
        self._aq_q = self._aq_act.view(np.float32)
        self._aq_ptrs = (self._aq_pin.data_ptr(), self._aq_pin.data_ptr() + 4)
        self._world = rdist.world_size()
        self._dist = rdist.active()
        self._exchange = None
        if self._dist:        # identical replicas: rank 0's initial parameters everywhere
            rdist.broadcast_parameters(self._params.detach(), 0)
            self.update_target_net()
            if rdist.mode() == "factored" and isinstance(self.optimiser, _FlatAdam):
                self._exchange = rdist.FactoredExchange(self._lib, self._h, self._grads)
        # RAINBOW_AMD_FUSED_DW=1 (single device + the library's own Adam): the hidden layer's weight gradient (93 % of the
        # gradient bytes) is never written to HBM — the backward computes it for the norm only, the clip + Adam pass
        # recomputes each tile while it streams that tile's parameters (include/rainbow_hip.h RB_LEARNER_FUSE_FC_H_DW);
        # self._grads then holds every OTHER gradient after learn().  51 MB less HBM traffic per step at the canonical
        # shape, measured 216.7 -> 215.3 us per step on MI355X: an opt-in, the default materialises every gradient as the
        # reference does.
        self._fused_dw = (isinstance(self.optimiser, _FlatAdam) and not self._dist
                          and os.environ.get("RAINBOW_AMD_FUSED_DW", "0") == "1")
        if self._fused_dw:
            self._defer_update = False
        # RAINBOW_AMD_IMPLICIT_SIGMA (default on with the deferred pass, single device): the hidden layer's sigma gradient is
        # g_mu * (eps_out x eps_in) element for element, so the backward does not store it and the hosted optimiser pass forms
        # it itself while it updates the (mu, sigma) pairs (include/rainbow_hip.h RB_LEARNER_IMPLICIT_SIGMA): 25.7 MB less HBM
        # traffic per step, bit-identical parameters; `grads` (which flushes) materialises it.
        self._implicit_sigma = (self._defer_update and not self._dist
                                and os.environ.get("RAINBOW_AMD_IMPLICIT_SIGMA", "1") == "1")
        L.check(self._lib, self._lib.rb_learner_set_flags(
            self._h, (L.LEARNER_FUSE_FC_H_DW if self._fused_dw else 0) | (L.LEARNER_DEFER_UPDATE if self._defer_update else 0)
            | (L.LEARNER_IMPLICIT_SIGMA if self._implicit_sigma else 0)))
        # args.target_tau > 0: the target network follows EVERY optimiser step, target += tau * (online - target), inside the
        # clip + Adam pass (include/rainbow_hip.h rb_learner_set_target_tau; tau = 1: DrQ / SPR, 0.005: SR-SPR / BBF) — the
        # loops of rainbow_amd.loop then skip the periodic hard sync.  0 (the default): nothing changes.
        self._target_tau = 0.0
        tau = float(getattr(args, "target_tau", 0.0) or 0.0)
        if tau != 0.0:
            self.target_tau = tau
        # shrink-and-perturb resets (reset_parameters): the defaults, the seed of the draws and the number of resets done so far,
        # which is the `draw` word of the next one's Philox counter (checkpoint() / restore() carry it)
        self._noisy_std = float(getattr(args, "noisy_std", 0.1))
        enc, head = getattr(args, "reset_shrink_encoder", None), getattr(args, "reset_shrink_head", None)
        self._reset_shrink = (0.5 if enc is None else float(enc), 0.0 if head is None else float(head))
        self._reset_seed = int(getattr(args, "seed", 0) or 0)
        self.resets = 0
        # recycling dormant units (agent_redo.py: dormant_stats / recycle_dormant): the threshold's default and the number of
        # recycles done so far, the `draw` word of the next one (checkpoint() / restore() carry it)
        self._redo_tau = getattr(args, "redo_tau", None)
        self.recycles = 0
        self.last_recycle_counts = None
        # args.step_stats = capacity: one rb_step_stats_t per learn() in a device ring, read with read_stats() (agent_stats.py).
        # Absent or 0 (the default): no ring, no extra launch.
        if int(getattr(args, "step_stats", 0) or 0) > 0:
            self.track_stats(int(args.step_stats))

    # The flat tensors the library borrows.  With a deferred optimiser pass pending they are one update behind: reading them
    # through these names runs the pass first.
    @property
    def params(self):
        self.flush()
        return self._params

    @property
    def grads(self):
        self.flush()
        return self._grads

    @property
    def _norm(self):
        self.flush()
        return self._norm_buf

    @property
    def target_params(self):
        """The target network's flat parameters.  With an EMA target (target_tau > 0) a pending optimiser pass moves them too:
        it runs first, as for `params`; otherwise the tensor is handed out as it always was."""
        if self._target_tau > 0:
            self.flush()
        return self._target_params

    @property
    def target_tau(self):
        return self._target_tau

    @target_tau.setter
    def target_tau(self, tau):
        tau = float(tau)
        if not 0.0 <= tau <= 1.0:                         # (also NaN)
            raise ValueError("target_tau must be in [0, 1], got %r" % tau)
        if tau == self._target_tau:
            return
        # (the library runs a pending pass first: its device-side arguments carry the old tau)
        L.check(self._lib, self._lib.rb_learner_set_target_tau(self._h, tau, self._stream()))
        self._update_pending = False
        self._target_tau = tau

    def target_ema(self, tau):
        """One EMA step of the target towards the online parameters now (rb_learner_target_ema): what learn() does itself, after
        its own optimiser step, when the optimiser is not the library's (RAINBOW_AMD_FUSED_ADAM=0)."""
        L.check(self._lib, self._lib.rb_learner_target_ema(self._h, float(tau), self._stream()))
        self._update_pending = False

    def reset_parameters(self, shrink_encoder=None, shrink_head=None, target=True, restart_step=False, rng=None):
        """Shrink-and-perturb reset (include/rainbow_hip.h rb_learner_shrink_perturb), one launch in stream order and no
        synchronisation: every tensor is pulled towards a FRESH draw phi from its initial distribution,
        theta <- alpha * theta + (1 - alpha) * phi, with alpha = shrink_encoder for convs.* (default args.reset_shrink_encoder, 0.5
        if absent) and alpha = shrink_head for the noisy-linear layers (default args.reset_shrink_head, 0.0 if absent: a full
        re-initialisation); an alpha outside [0, 1] raises ValueError.  A pending optimiser pass runs first.  target=True: the
        target network follows the same draw.  The Adam moments of the touched tensors (alpha < 1) are cleared — those of
        whichever optimiser is active; restart_step=True also sets the Adam step number back to 0 (the default leaves it alone).
        rng = (seed, draw) keys the draw and defaults to (args.seed or 0, self.resets): replicas that pass the same pair draw
        the same phi, and a run resumed from checkpoint() repeats it bit for bit.  self.resets counts the resets done."""
        ae = self._reset_shrink[0] if shrink_encoder is None else float(shrink_encoder)
        ah = self._reset_shrink[1] if shrink_head is None else float(shrink_head)
        for name, a in (("shrink_encoder", ae), ("shrink_head", ah)):
            if not 0.0 <= a <= 1.0:                       # (also NaN)
                raise ValueError("reset_parameters: %s must be in [0, 1], got %r" % (name, a))
        seed, draw = u64_pair((self._reset_seed, self.resets) if rng is None else rng)
        st = self.optimiser.state.get(self._params, {})   # (torch's own Adam has no state before its first step: no moments to clear)
        m, v = st.get("exp_avg"), st.get("exp_avg_sq")
        L.check(self._lib, self._lib.rb_learner_shrink_perturb(
            self._h, ae, ah, self._noisy_std, seed, draw, 1 if target else 0,
            m.data_ptr() if m is not None else None, v.data_ptr() if v is not None else None, self._stream()))
        self._update_pending = False                      # (the library ran a pending pass first)
        if restart_step:
            if self._step_dev is not None:
                self._step_dev.zero_()
            if "step" in st:
                st["step"].zero_()
        self.resets += 1

    def set_horizon(self, n, discount=None):
        """The effective multi-step horizon and discount of the targets (rb_learner_set_horizon; BBF anneals n from 10 to 3 and
        gamma from 0.97 to 0.997 after every reset — rainbow_amd.loop.horizon_at): 1 <= n <= self.n, the multi_step of
        construction, 0 < discount <= 1, None keeps the current discount.  Host state read when the next step is launched: no
        launch, no synchronisation.  The replay must be set to the same pair (ReplayMemory.set_horizon): learn() compares."""
        n = int(n)
        g = float(self.discount if discount is None else discount)
        if not 1 <= n <= int(self.n):
            raise ValueError("set_horizon: n must be in [1, %d] (the multi_step of construction), got %d" % (self.n, n))
        if not 0.0 < g <= 1.0:                            # (also NaN)
            raise ValueError("set_horizon: discount must be in (0, 1], got %r" % g)
        L.check(self._lib, self._lib.rb_learner_set_horizon(self._h, n, g))
        self.horizon, self.discount = n, g

    def flush(self):
        """Run the optimiser pass the last learn() left pending (RAINBOW_AMD_DEFER_UPDATE), if any."""
        if self._update_pending:
            self._update_pending = False
            L.check(self._lib, self._lib.rb_learner_flush(self._h, self._stream()))

    # ------------------------------------------------------------------ plumbing
    def __del__(self):
        try:
            if self._h:
                self._lib.rb_learner_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        return current_stream_handle(self.device)

    def _view(self, flat, name):
        for n, off, shape in self._layout:
            if n == name:
                return flat.detach()[off:off + int(np.prod(shape))].view(shape)
        raise KeyError(name)

    def _noise_view(self, flat, name):
        for n, off, shape in self._noise_layout:
            if n == name:
                return flat[off:off + shape[0]]
        raise KeyError(name)

    def _init_parameters(self, noisy_std):
        with torch.no_grad():
            self._params.copy_(init_parameters_flat(self._layout, self._params.numel(), noisy_std))

    # ------------------------------------------------------------------ reference API
    def reset_noise(self, raw_normals=None):
        """agent.py:49-50 (online net only).  raw_normals: optional float32 device tensor of N(0,1) draws in the
        reference's order (parity hook)."""
        if raw_normals is None:
            # lazily: main.py calls reset_noise() right before learn() every 4th step (main.py:151,164); the draw is
            # deferred so learn() can resample online + target noise in ONE launch.  act()/evaluate_q() flush it first.
            self._noise_pending = True
            return
        self._noise_pending = False
        raw = self._keep["raw_online"] = raw_normals.to(device=self.device, dtype=torch.float32).contiguous()
        L.check(self._lib, self._lib.rb_learner_reset_noise(self._h, 0, raw.data_ptr(), self._stream()))

    def _flush_noise(self):
        if self._noise_pending:
            self._noise_pending = False
            L.check(self._lib, self._lib.rb_learner_reset_noise(self._h, 0, None, self._stream()))

    def _reset_target_noise(self, raw_normals=None):
        ptr = None
        if raw_normals is not None:
            raw = self._keep["raw_target"] = raw_normals.to(device=self.device, dtype=torch.float32).contiguous()
            ptr = raw.data_ptr()
        L.check(self._lib, self._lib.rb_learner_reset_noise(self._h, 1, ptr, self._stream()))   # agent.py:74

    def _sync_step(self):
        """Host mirror of the device-resident optimiser step number (state_dict / checkpoint read it)."""
        if self._step_dev is not None and isinstance(self.optimiser, _FlatAdam):
            self.optimiser.state[self._params]["step"].fill_(float(self._step_dev.item()))

    def update_target_net(self):
        """agent.py:102-103."""
        self._flush_noise()
        L.check(self._lib, self._lib.rb_learner_sync_target(self._h, self._stream()))

    def train(self):
        self.training = True        # agent.py:114-115

    def eval(self):
        self.training = False       # agent.py:117-118 -> mu-only forward (model.py:46)
