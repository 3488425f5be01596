"""Agent.learn: the step's setup (noise job, priority sink, path choice) in one place and its two issuers — the whole step as
one C call (_learn_one_call) or as sample / learn / optimiser calls from here (_learn_eager).  A mixin over the learner handle,
the flat buffers and the optimiser that rainbow_amd.agent.Agent owns."""
import ctypes as C
import math
import weakref

import torch

from . import _lib as L
from . import dist as rdist
from ._util import current_stream_handle
from .memory import ReplayMemory
from .params import _FlatAdam, takes_plain_adam


class AgentLearn:
    def learn(self, mem, _target_raw_normals=None, _unit_uniforms=None):
        """agent.py:61-100.  With a rainbow_amd ReplayMemory the whole step (sample .. priority update) is
        device-resident and launched eagerly.  The injected-randomness arguments are parity-test hooks."""
        device_mem = isinstance(mem, ReplayMemory)
        if device_mem:
            if mem.horizon != self.horizon or mem.discount != self.discount:      # (host values: no synchronisation)
                raise ValueError("Agent.learn: the memory's horizon and discount (%d, %r) differ from the agent's (%d, %r): call "
                                 "set_horizon on both with the same values" % (mem.horizon, mem.discount, self.horizon, self.discount))
            if self._step_dev is None:
                # by-value step numbers (RAINBOW_AMD_DEFER_UPDATE=0): the host's step count must be exact BEFORE the next
                # optimiser pass is issued, so the sampler launches in flight are waited for here (the default mode counts the
                # steps on the device and needs no such sync: a failure is then reported one learn() late, nothing else)
                torch.cuda.current_stream(self.device).synchronize()
            failed = mem.failed_samples()
            if failed:
                self._raise_on_failed_samples(mem, failed)
        stream = current_stream_handle(self.device)   # ONE lookup per step (torch.cuda.current_stream costs ~4 us a call)
        if self._zero_copy_ok is None:                # a property of the learner's configuration: asked once
            self._zero_copy_ok = bool(self._lib.rb_learner_zero_copy_ok(self._h))
        # (a memory with random-shift augmentation — ReplayMemory augment_pad — builds shifted stacks in its gather: the ring
        # holds the un-shifted frames, so the step takes the gathered path)
        zero_copy = (device_mem and self._zero_copy_ok and mem.history == self._cfg.history and mem.n == self.n
                     and not mem.augment_pad)
        if self._can_one_call(zero_copy, _target_raw_normals is not None or _unit_uniforms is not None):
            self._learn_one_call(mem, stream)
        else:
            self._learn_eager(mem, stream, zero_copy, _target_raw_normals, _unit_uniforms)

    def _raise_on_failed_samples(self, mem, failed):
        """The device sampler is bounded where the reference's rejection loop (memory.py:128-132) would spin forever.  A
        launch that gave up left NO trace on the device (zero importance weights; the priority write-back, the optimiser
        update and the device-resident step number are skipped when the header says so): here the host side is put back
        in step — the optimiser's step count is rolled back by the number of skipped updates, the counter is cleared —
        and the failure is raised.  The caller may append more transitions and call learn() again."""
        if isinstance(self.optimiser, _FlatAdam) and self._sink_mem is mem:
            st = self.optimiser.state[self._params]
            st["step"] -= float(min(failed, int(st["step"].item())))
        mem.reset_failed_samples()
        raise RuntimeError("ReplayMemory: %d sampler launch(es) found no valid batch in %d attempts (replay too small for "
                           "batch %d?); those steps were skipped on the device (no priority write-back, no optimiser update)"
                           % (failed, mem.MAX_ATTEMPTS, self.batch_size))

    # ------------------------------------------------------------------ the step's setup
    def _noise_job(self, which=None):
        """The learner's noise job `which` (1: target draw, 2: online then target draw), queried once and cached (restore()
        clears the cache: the jobs carry the generator's seed).  which=None takes the job that rides in this step's sampler
        launch: the target-noise draw (agent.py:74) plus the deferred online draw (main.py:151) when one is pending, which it
        thereby consumes.  The draw does not depend on the batch, only has to precede the forwards, and is the same Philox
        epochs as separate launches (online first, then target)."""
        if which is None:
            which = 2 if self._noise_pending else 1
            self._noise_pending = False
        job = self._noise_jobs.get(which)
        if job is None:
            job = L.NoiseJob()
            L.check(self._lib, self._lib.rb_learner_noise_job(self._h, which, C.byref(job)))
            self._noise_jobs[which] = job
        return job

    def _can_one_call(self, zero_copy, injected):
        """Whether rb_learner_train_step issues exactly what _learn_eager's three calls would for this step."""
        return (self._one_call                                  # RAINBOW_AMD_ONE_CALL=0 asks for the three calls
                and zero_copy                                   # the call reads the frames from the ring of a device memory
                and not injected                                # parity hooks upload their randomness between the calls
                and self._fuse_update                           # the call has no separate priority write-back
                # replicas: only the library's own RCCL all-gather fits between the call's backward and its clip
                and (self._exchange.comm is not None if self._exchange is not None else not self._dist)
                and math.isfinite(float(self.norm_clip))        # the call always clips and reports the norm
                and takes_plain_adam(self.optimiser))           # its optimiser pass is the library's plain Adam

    def _arm_sink(self, mem, idxs):
        """The learner writes the new priorities of the batch at `idxs` into mem's sum-tree itself (one extra workgroup of its
        backward, rb_learner_set_priority_sink); nothing to do while (mem, idxs) is already the sink."""
        if self._sink_mem is not mem or self._sink_idx is not idxs:
            L.check(self._lib, self._lib.rb_learner_set_priority_sink(self._h, mem._h, idxs.data_ptr()))
            self._sink_mem, self._sink_idx = mem, idxs
            self._watch_sink(mem)

    def _disarm_sink(self):
        if self._sink_mem is not None:
            if self._h:
                L.check(self._lib, self._lib.rb_learner_set_priority_sink(self._h, None, None))
            self._sink_mem, self._sink_idx = None, None

    def _watch_sink(self, mem):
        """The library caches raw pointers into `mem` (priority sink): drop them when THAT memory goes away before the agent
        does.  One finalizer per memory, and it only acts if that memory is still the current sink (after a switch from
        memory A to memory B, collecting A must not clear B's sink)."""
        key = id(mem)
        if key in self._sink_watched:
            return
        self._sink_watched.add(key)
        me = weakref.ref(self)

        def gone(key=key):
            ag = me()
            if ag is not None:
                ag._sink_watched.discard(key)
                if ag._sink_key == key:
                    ag._clear_sink()
        weakref.finalize(mem, gone)

    @property
    def _sink_key(self):
        m = self._sink_mem
        return id(m) if m is not None else None

    def _clear_sink(self):
        self._disarm_sink()
        self._ts = self._ts_mem = self._ts_out = None      # the one-call path re-arms the sink on its next step

    # ------------------------------------------------------------------ the two issuers
    def _learn_one_call(self, mem, stream):
        """The whole step through rb_learner_train_step (one C call): same entry points, same arguments, same order as
        _learn_eager's three calls — without the interpreter between the launches (include/rainbow_hip.h says why)."""
        B = self.batch_size
        ts = self._ts
        o = mem.begin_external_draw(B)     # (applies a caller's update_priorities() since the last draw first)
        if ts is None or self._ts_mem is not mem or o is not self._ts_out:
            frames, windows, wlen = mem.frame_source()
            self._arm_sink(mem, o["tree_idxs"])
            ts = L.TrainStep(replay=mem._h, batch=B, max_attempts=mem.MAX_ATTEMPTS, window_len=wlen,
                             tree_idx_dev=o["tree_idxs"].data_ptr(), actions_dev=o["actions"].data_ptr(),
                             returns_dev=o["returns"].data_ptr(), nonterminals_dev=o["nonterminals"].data_ptr(),
                             weights_dev=o["weights"].data_ptr(), frames_dev=frames, windows_dev=windows,
                             loss_dev=self._loss.data_ptr(), norm_dev=self._norm_buf.data_ptr())
            self._ts, self._ts_mem, self._ts_out = ts, mem, o
        job = self._noise_job()
        g, st, ts.step = self.optimiser.count_step(self)
        ts.exp_avg_dev, ts.exp_avg_sq_dev = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        ts.priority_weight = float(mem.priority_weight)
        ts.noise_job = C.addressof(job)
        ts.lr, ts.eps, ts.max_norm = float(g["lr"]), float(g["eps"]), float(self.norm_clip)
        ts.beta1, ts.beta2 = g["betas"]
        if self._exchange is not None:     # replicas: the library's own RCCL all-gather sits between backward and clip
            rc = self._lib.rb_learner_train_step_dist(self._h, C.byref(ts), self._exchange.comm, stream)
        else:
            rc = self._lib.rb_learner_train_step(self._h, C.byref(ts), stream)
        if rc != 0:
            L.check(self._lib, rc)
        self._update_pending = self._defer_update
        if not self._lib.rb_learner_priority_written(self._h):       # (cannot happen with a sink set; keeps agent.py:100)
            # immediately: a lazy write-back would read tree_idxs / _loss after the next step has overwritten them
            mem.update_priorities(o["tree_idxs"], self._loss, _immediate=True)

    def _learn_eager(self, mem, stream, zero_copy, _target_raw_normals=None, _unit_uniforms=None):
        B = self.batch_size
        device_mem = isinstance(mem, ReplayMemory)
        noise_job = None
        overwrite_target = False
        if device_mem and _target_raw_normals is not None and self._update_pending and not self._noise_pending:
            # parity runs (injected normals) keep the product's launch shape: the sampler launch still hosts the pending
            # optimiser pass, carried by a target-noise job whose device-RNG draw the injected normals overwrite below
            noise_job = self._noise_job(1)
            overwrite_target = True
        elif device_mem and _target_raw_normals is None:
            noise_job = self._noise_job()
        if device_mem:
            hosted = 0
            if noise_job is not None and self._update_pending:
                # the previous call's clip + Adam pass rides in this sampler launch (RB_LEARNER_DEFER_UPDATE)
                hosted = self._lib.rb_learner_attach_pending(self._h, C.byref(noise_job), B, C.byref(self._hosted_job))
                if hosted < 0:
                    L.check(self._lib, hosted)
            o = mem.sample_device(B, _unit_uniforms, gather=not zero_copy,
                                  noise_job=self._hosted_job if hosted == 1 else noise_job, stream=stream)   # agent.py:63
            if hosted == 1:
                L.check(self._lib, self._lib.rb_learner_pending_launched(self._h))
                self._update_pending = False
            idxs, states, next_states = o["tree_idxs"], o["states"], o["next_states"]
            actions, returns, nonterminals, weights = o["actions"], o["returns"], o["nonterminals"], o["weights"]
        else:   # foreign replay with the reference's API: float32 /255 states come back; re-quantise (exact for k/255)
            idxs, s, actions, returns, ns, nonterminals, weights = mem.sample(B)
            d = self.device
            states = s.to(d).mul(255).round_().to(torch.uint8).contiguous()
            next_states = ns.to(d).mul(255).round_().to(torch.uint8).contiguous()
            actions = actions.to(device=d, dtype=torch.int64).contiguous()
            returns = returns.to(device=d, dtype=torch.float32).contiguous()
            nonterminals = nonterminals.to(device=d, dtype=torch.float32).reshape(B).contiguous()
            weights = weights.to(device=d, dtype=torch.float32).contiguous()
        if noise_job is None:
            if self._noise_pending and _target_raw_normals is None:
                self._noise_pending = False      # online (main.py:151) and target (agent.py:74) noise in one launch
                L.check(self._lib, self._lib.rb_learner_reset_noise(self._h, 2, None, stream))
            else:
                self._flush_noise()
                self._reset_target_noise(_target_raw_normals)                              # agent.py:74
        elif overwrite_target:
            self._reset_target_noise(_target_raw_normals)                                  # agent.py:74 (injected draw)
        if not device_mem:
            self._disarm_sink()
        elif self._fuse_update:
            self._arm_sink(mem, idxs)
        if zero_copy:   # conv1 reads the frames straight out of the HBM ring: no stack gather at all
            frames, windows, wlen = mem.frame_source()
            rc = self._lib.rb_learner_learn_windows(
                self._h, frames, windows, wlen, actions.data_ptr(), returns.data_ptr(), nonterminals.data_ptr(),
                weights.data_ptr(), self._loss.data_ptr(), stream)
            if rc != 0:
                L.check(self._lib, rc)
        else:
            L.check(self._lib, self._lib.rb_learner_learn(
                self._h, states.data_ptr(), next_states.data_ptr(), actions.data_ptr(), returns.data_ptr(),
                nonterminals.data_ptr(), weights.data_ptr(), self._loss.data_ptr(), stream))   # agent.py:66-96
        fused_update = device_mem and bool(self._lib.rb_learner_priority_written(self._h))
        if self._exchange is not None:
            # replicas, factored exchange (the insert point between agent.py:96 and :97): ONE all-gather of every rank's
            # block — the factors of its FC weight gradients (dY and X rows, its noise vectors) and its conv gradients,
            # 1.0 MB — on this stream, then rb_learner_finish_grads forms the replica-mean gradient of the global batch
            # on every replica (rainbow_amd/dist.py)
            self._exchange.run()
        elif self._dist:      # replicas, plain exchange: one RCCL all-reduce of the flat gradient (4*P bytes)
            rdist.average_gradients(self._grads)
            L.check(self._lib, self._lib.rb_learner_grads_modified(self._h))
        if isinstance(self.optimiser, _FlatAdam):
            defer = self._defer_update and device_mem
            self.optimiser.step_direct(float(self.norm_clip), stream, defer=defer)         # agent.py:97-98, one pass
            if defer:
                self._update_pending = True      # (the library decides; flush() is a no-op when it ran at once)
        else:
            L.check(self._lib, self._lib.rb_learner_clip_grad(self._h, float(self.norm_clip), self._norm_buf.data_ptr(),
                                                              stream))                    # agent.py:97
            self.optimiser.step()                                                          # agent.py:98
            if self._target_tau > 0:             # (torch's own Adam: the library's passes never run, the EMA is a launch of its own)
                L.check(self._lib, self._lib.rb_learner_target_ema(self._h, self._target_tau, stream))
        if device_mem:
            if not fused_update:
                mem.update_priorities(idxs, self._loss, _immediate=True)                   # agent.py:100, no D2H
        else:
            mem.update_priorities(idxs, self._loss.detach().cpu().numpy())                 # agent.py:100
