"""Drop-in `ReplayMemory` for the reference's main.py / test.py (replaces /root/reference/memory.py).

Same constructor, attributes and methods as the reference class (memory.py:91-180), but the ring
buffer, the float32 sum-tree, the stratified sampler, the frame-stack gather and the priority
update all live in HBM behind librainbow_hip.so (C ABI: include/rainbow_hip.h).  Python only
forwards pointers; there is no CPU path.

Two ways to consume a batch:
  * `sample(batch_size)` — the reference's 7-tuple (memory.py:148-155), states as float32 /255.
    Needs one D2H copy of the tree indices because the reference returns them as a numpy array.
  * `sample_device(batch_size)` — device-resident outputs (uint8 frame stacks, no sync); this is
    what rainbow_amd.agent.Agent.learn uses.

Vectorised environments: `ReplayMemory(args, capacity, streams=S)` holds S interleaved environment streams in one ring and
one sum tree (stream s owns the slots s, s + S, s + 2S, ...) and is filled a round at a time with `append_streams` — one
transition per environment, one launch.  Sampling, priorities and IS weights are those of ONE replay over all streams; windows
and n-step returns never cross from one stream into another.  streams=1 is the reference's replay, unchanged.

Random-shift augmentation (DrQ): `args.augment_pad = p` (1..8; absent or 0 = off, today's launches exactly) shifts every sampled
stack by (dy, dx) in [-p, p] with edge replication — `states` and `next_states` independently, all `history` frames of one stack
alike — inside the frame-stack gather (rb_replay_gather_shifted).  Only `sample_device(gather=True)` and `sample()` are shifted;
`__next__`, `state_at` / `states_at` (validation, evaluation) never are.

Annealed update horizon and discount (BBF): `set_horizon(n, discount=None)` changes the effective multi-step horizon (1 <= n <= the
`multi_step` of construction, which `.n` keeps naming) and the discount of the LIVE replay, ring and tree untouched; `.horizon` and
`.discount` are the values in force.  The next batch is the one a replay built with multi_step = n would draw.

This module: construction, sampling and priorities.  The write side (append and its per-stream forms) is memory_append.py; the
column table, save_to / load_from and pickling are memory_state.py.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from ._util import current_stream_handle
from .memory_append import ReplayAppend
from .memory_state import ReplayState


class _TransitionsView:
    """Read-only stand-in for the reference's `mem.transitions` SegmentTree attribute."""

    def __init__(self, owner):
        self._o = owner

    def _hdr(self):
        return self._o._header()

    def _pos(self):
        idx, full = C.c_int64(0), C.c_int32(0)
        L.check(self._o._lib, self._o._lib.rb_replay_position(self._o._h, C.byref(idx), C.byref(full)))
        return int(idx.value), bool(full.value)

    @property
    def index(self):
        """memory.py:14 — from the library's host mirror: no device synchronisation (safe to poll in the env loop)."""
        return self._pos()[0]

    @property
    def full(self):
        """memory.py:16 — host mirror, no synchronisation."""
        return self._pos()[1]

    @property
    def max(self):
        """memory.py:20 — lives on the device (updated by priority write-backs): SYNCHRONISES the stream."""
        return float(self._hdr().max)

    def total(self):
        """memory.py:88-89 — tree root: SYNCHRONISES the stream."""
        return float(self._hdr().total)


class ReplayMemory(ReplayAppend, ReplayState):
    # The reference redraws until the batch is valid (memory.py:128-132).  The device loop is bounded, but generously: a
    # redraw costs ~4 us inside the one sampler launch, and hitting the bound means no valid batch exists at all (buffer
    # too small for the batch).  Then the batch gets zero importance weights (a zero-gradient step) and
    # failed_samples() counts it; Agent.learn raises on the next call.
    MAX_ATTEMPTS = 1024
    # update_priorities() is LAZY (RAINBOW_AMD_LAZY_PRIORITIES=0: immediate): the write-back of learn step k and the draw of
    # step k + 1 are a dependent pair of single-workgroup launches, so the call only records its operands and the next
    # sample_device() issues both as ONE launch (rb_replay_update_sample: bit-identical tree, header and batch).  Anything
    # else that reads or writes the tree — append, the header, state dumps, the raw handle `_h` — applies the pending
    # write-back first.  Operands are copied at the call — numpy arrays (the reference's call site, agent.py:100) by their
    # upload, device tensors into a two-slot staging buffer this object owns (_stage_operands) — so the caller may reuse its
    # loss / index tensors at once, as with the reference's immediate update.
    _pending = None             # (these two: so that __del__ and `_h` are safe on an object whose construction failed early)
    _handle = None
    streams = 1                 # (a pickle written before interleaved streams existed restores as one stream)
    augment_pad = 0             # (a pickle written before the random-shift option existed restores with it off)
    _aug_draw = 0               # batches shifted so far: the `draw` word of the shift RNG's counter (rb_replay_gather_shifted)
    horizon = None              # (a pickle written before set_horizon existed restores at horizon == n: __setstate__)
    MAX_AUGMENT_PAD = 8
    _lazy = os.environ.get("RAINBOW_AMD_LAZY_PRIORITIES", "1") != "0"

    @property
    def _h(self):
        if self._pending is not None:
            self.flush()
        return self._handle

    @_h.setter
    def _h(self, value):
        self._handle = value

    def flush(self):
        """Apply a pending update_priorities() now (a launch of its own)."""
        pend, self._pending = self._pending, None
        if pend is not None:
            L.check(self._lib, self._lib.rb_replay_update_priorities(self._handle, pend[0].data_ptr(), pend[1].data_ptr(),
                                                                     int(pend[0].numel()), self._stream()))

    def __init__(self, args, capacity, seed=None, streams=1):
        self.device = torch.device(args.device)
        if self.device.type != "cuda":
            raise RuntimeError("rainbow_amd.ReplayMemory lives in HBM: args.device must be a cuda (ROCm) device, got %s"
                               % self.device)
        self.capacity = int(capacity)
        self.history = int(args.history_length)
        self.discount = float(args.discount)
        self.n = int(args.multi_step)                           # n_max: allocations and the window table's row stride
        self.horizon = self.n                                   # the effective horizon (set_horizon; learn() reads it every step)
        self.priority_weight = float(args.priority_weight)      # beta, annealed by the caller (main.py:161)
        self.priority_exponent = float(args.priority_exponent)
        self.t = 0                                              # episode timestep counter (memory.py:100)
        self.streams = int(streams)
        self.stream_t = np.zeros(self.streams, dtype=np.int32)  # the same counter per environment stream (append_streams)
        self._seed = int(seed if seed is not None else np.random.randint(0, 2 ** 31 - 1))
        self.augment_pad = self._checked_pad(getattr(args, "augment_pad", 0))
        self._aug_draw = 0
        self._lazy = os.environ.get("RAINBOW_AMD_LAZY_PRIORITIES", "1") != "0"
        self._init_runtime()
        self.current_idx = 0

    def _init_runtime(self):
        """Everything outside the saved state, built by __init__ and again by __setstate__: the library and replay handles, the
        pending write-back and its staging ring, the output buffers and their pointer cache, and `_keep`, which holds every
        operand a launch in flight still reads (injected uniforms and shifts, applied write-backs, the last device round).
        __getstate__ leaves out ReplayState._RUNTIME; `_ptr_cache` alone is pickled as it always was and rebuilt here."""
        self._lib = L.load()
        self._pending = None
        self._stage = {}
        self._keep = {}
        self._out = {}
        self._ptr_cache = {}
        self._bufs = None                                       # frame_source(): the column pointers, asked once
        self._create()
        self.transitions = _TransitionsView(self)
        self._init_beta_source()

    def begin_external_draw(self, batch):
        """For a caller that issues the draw itself (rb_learner_train_step): what sample_device() does before its launch — a
        pending write-back applied, -beta in HBM brought up to date — and the output buffers of `batch`."""
        if self._pending is not None:
            self.flush()
        if float(self.priority_weight) != self._neg_beta_val:
            self._sync_beta()
        o = self._out.get(batch)
        return o if o is not None else self._buffers(batch)

    @classmethod
    def _checked_pad(cls, pad):
        pad = int(pad or 0)
        if not 0 <= pad <= cls.MAX_AUGMENT_PAD:
            raise ValueError("ReplayMemory: augment_pad must be in [0, %d], got %d" % (cls.MAX_AUGMENT_PAD, pad))
        return pad

    def _create(self):
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            if self.streams == 1:
                rc = self._lib.rb_replay_create(C.byref(self._h), self.capacity, self.history, self.n, self.discount,
                                                self.priority_exponent, self._seed)
            else:
                rc = self._lib.rb_replay_create_streams(C.byref(self._h), self.capacity, self.history, self.n, self.discount,
                                                        self.priority_exponent, self._seed, self.streams)
            L.check(self._lib, rc)
            if self.horizon != self.n:      # (a restored state: the handle is created at n_max and the discount in force)
                L.check(self._lib, self._lib.rb_replay_set_horizon(self._handle, self.horizon, self.discount, self._stream()))

    def set_horizon(self, n, discount=None):
        """The effective horizon and discount of the live replay (rb_replay_set_horizon): 1 <= n <= self.n, 0 < discount <= 1,
        None keeps the current discount.  A pending lazy write-back is applied first; one tiny launch in stream order, no
        synchronisation.  The learner that consumes the batches must be set to the same pair (Agent.set_horizon): Agent.learn
        compares and raises."""
        n = int(n)
        g = float(self.discount if discount is None else discount)
        if not 1 <= n <= self.n:
            raise ValueError("set_horizon: n must be in [1, %d] (the multi_step of construction), got %d" % (self.n, n))
        if not 0.0 < g <= 1.0:                                  # (also NaN)
            raise ValueError("set_horizon: discount must be in (0, 1], got %r" % g)
        L.check(self._lib, self._lib.rb_replay_set_horizon(self._h, n, g, self._stream()))
        self.horizon, self.discount = n, g

    def _init_beta_source(self):
        # -beta lives in HBM so a captured hipGraph sees main.py:161's annealing (by-value kernel arguments freeze)
        self._neg_beta_dev = torch.full((1,), -float(self.priority_weight), dtype=torch.float32, device=self.device)
        self._neg_beta_val = float(self.priority_weight)
        L.check(self._lib, self._lib.rb_replay_set_beta_source(self._handle, self._neg_beta_dev.data_ptr()))

    def _sync_beta(self):
        if float(self.priority_weight) != self._neg_beta_val:
            self._neg_beta_val = float(self.priority_weight)
            self._neg_beta_dev.fill_(-self._neg_beta_val)     # float32(-beta): NEP-50 weak scalar, memory.py:153

    # ------------------------------------------------------------------ plumbing
    def __del__(self):
        try:
            self._pending = None
            if self._handle:
                self._lib.rb_replay_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    def _stream(self):
        return current_stream_handle(self.device)

    def _header(self):
        hdr = L.ReplayHeader()
        L.check(self._lib, self._lib.rb_replay_header(self._h, C.byref(hdr), self._stream()))
        return hdr

    def _buffers(self, batch):
        key = int(batch)
        if key not in self._out:
            self._ptr_cache = {k: v for k, v in self._ptr_cache.items() if k[0] != key}
            d, h = self.device, self.history
            self._out[key] = dict(
                tree_idxs=torch.empty(batch, dtype=torch.int64, device=d),
                states=torch.empty(batch, h, 84, 84, dtype=torch.uint8, device=d),
                next_states=torch.empty(batch, h, 84, 84, dtype=torch.uint8, device=d),
                actions=torch.empty(batch, dtype=torch.int64, device=d),
                returns=torch.empty(batch, dtype=torch.float32, device=d),
                nonterminals=torch.empty(batch, dtype=torch.float32, device=d),
                weights=torch.empty(batch, dtype=torch.float32, device=d))
        return self._out[key]

    # ------------------------------------------------------------------ reference API
    def failed_samples(self):
        """Sampler launches completed so far that found no valid batch within MAX_ATTEMPTS (read from pinned host memory
        the kernel writes: no synchronisation)."""
        n = C.c_int64(0)
        rc = self._lib.rb_replay_failed_samples(self._handle, C.byref(n))      # (asked on every learn step)
        if rc != 0:
            L.check(self._lib, rc)
        return int(n.value)

    def dropped_updates(self):
        """Priority write-backs dropped so far because their indices came from a draw that gave up (pinned host word: no
        synchronisation).  Zeroed by reset_failed_samples()."""
        n = C.c_int64(0)
        L.check(self._lib, self._lib.rb_replay_dropped_updates(self._handle, C.byref(n)))
        return int(n.value)

    def expired_waits(self):
        """Cross-stream waits of the early draw (RB_OPTS spec_draw=1, off by default) that hit their ~2 ms bound so far (pinned
        host word: no synchronisation).  Each one failed safe (the waiting launch drew itself / dropped the write-back) and
        switched the early draw off on this replay until reset_failed_samples().  0 on a healthy device."""
        n = C.c_int64(0)
        L.check(self._lib, self._lib.rb_replay_expired_waits(self._handle, C.byref(n)))
        return int(n.value)

    def reset_failed_samples(self):
        """Zero those counters (the failure has been reported to the caller); allows the early draw again."""
        L.check(self._lib, self._lib.rb_replay_reset_failed_samples(self._handle))

    def frame_source(self):
        """(frames_ptr, windows_ptr, window_len): lets the learner read frames straight from the ring (zero-copy)."""
        if self._bufs is None:
            b = L.ReplayBuffers()
            L.check(self._lib, self._lib.rb_replay_buffers(self._h, C.byref(b)))
            self._bufs = b
        return self._bufs.frames_dev, self._bufs.window_dev, int(self._bufs.window_len)

    def sample_device(self, batch_size, unit_uniforms=None, gather=True, noise_job=None, stream=None, shifts=None):
        """Device-resident batch: dict(tree_idxs i64[B], states u8[B,h,84,84], next_states u8, actions i64[B],
        returns f32[B], nonterminals f32[B], weights f32[B]).  Asynchronous.  unit_uniforms (float64 device
        tensor [attempts,B]) injects the sampler's random numbers for parity tests.  gather=False skips the
        frame-stack copies (states/next_states are then stale): the consumer reads the ring via frame_source().
        noise_job (rainbow_amd._lib.NoiseJob from the learner) lets the launch also carry the noise resample.
        With augment_pad > 0 and gather=True the stacks come out of the shifted gather (one launch behind the sampler's, which
        then builds no stacks itself) and the dict also holds `shifts` (int8 [B,2,2]: [i][state, next] -> (dy, dx), the shifts
        used).  `shifts` (int8 [B,2,2]) injects them for parity tests; otherwise they are the device draw number `_aug_draw`,
        which every augmented batch advances by one."""
        if self.augment_pad and gather:
            return self._sample_device_shifted(batch_size, unit_uniforms, noise_job, stream, shifts)
        o = self._buffers(batch_size)
        if float(self.priority_weight) != self._neg_beta_val and not torch.cuda.is_current_stream_capturing():
            self._sync_beta()
        uu_ptr, attempts = None, self.MAX_ATTEMPTS
        if unit_uniforms is not None:
            uu = self._keep["uu"] = unit_uniforms.to(device=self.device, dtype=torch.float64).contiguous()
            uu_ptr, attempts = uu.data_ptr(), int(uu.shape[0])
        # the output buffers are persistent: their addresses are looked up once per (batch, gather), not per call (the
        # host side of a learn step is about as long as its GPU side at batch 32 — every microsecond here is on the clock)
        key = (int(batch_size), bool(gather))
        ptrs = self._ptr_cache.get(key)
        if ptrs is None:
            ptrs = (o["tree_idxs"].data_ptr(), o["states"].data_ptr() if gather else None,
                    o["next_states"].data_ptr() if gather else None, o["actions"].data_ptr(), o["returns"].data_ptr(),
                    o["nonterminals"].data_ptr(), o["weights"].data_ptr())
            self._ptr_cache[key] = ptrs
        if stream is None:
            stream = self._stream()
        pend = self._pending
        if noise_job is not None:
            if pend is not None:      # (the noise-carrying launch has no write-back slot: apply it first, in stream order)
                self.flush()
            rc = self._lib.rb_replay_sample_fused_noise(self._h, key[0], float(self.priority_weight), uu_ptr, attempts, *ptrs,
                                                        C.byref(noise_job), stream)
        elif pend is not None:        # the pending write-back and this draw as one launch
            self._pending = None
            rc = self._lib.rb_replay_update_sample(self._handle, pend[0].data_ptr(), pend[1].data_ptr(), int(pend[0].numel()), key[0],
                                                   float(self.priority_weight), uu_ptr, attempts, *ptrs, stream)
            self._keep["applied"] = pend      # (its operands stay alive until the launch after this one)
        else:
            rc = self._lib.rb_replay_sample(self._handle, key[0], float(self.priority_weight), uu_ptr, attempts, *ptrs, stream)
        if rc != 0:
            L.check(self._lib, rc)
        return o

    def _sample_device_shifted(self, batch_size, unit_uniforms, noise_job, stream, shifts):
        """sample_device(gather=True) under augment_pad > 0: the draw with NULL stacks (gather=False: the same three-way choice of
        launch, update and noise fusions as they are), then the shifted gather of that draw's window table."""
        if stream is None:
            stream = self._stream()
        o = self.sample_device(batch_size, unit_uniforms, gather=False, noise_job=noise_job, stream=stream)
        B = int(batch_size)
        sh = o.get("shifts")
        if sh is None:
            sh = o["shifts"] = torch.zeros(B, 2, 2, dtype=torch.int8, device=self.device)
        in_ptr = None
        if shifts is not None:
            sh_in = self._keep["shifts_in"] = torch.as_tensor(shifts).to(device=self.device, dtype=torch.int8).contiguous()
            if tuple(sh_in.shape) != (B, 2, 2):
                raise ValueError("sample_device: shifts must be [%d, 2, 2], got %s" % (B, tuple(sh_in.shape)))
            in_ptr = sh_in.data_ptr()
        rc = self._lib.rb_replay_gather_shifted(self._handle, B, int(self.augment_pad), int(self._aug_draw), in_ptr,
                                                o["states"].data_ptr(), o["next_states"].data_ptr(), sh.data_ptr(), stream)
        if rc != 0:
            L.check(self._lib, rc)
        self._aug_draw += 1
        return o

    def sample(self, batch_size):
        """memory.py:148-155 7-tuple: (tree_idxs ndarray, states f32, actions i64, returns f32, next_states f32,
        nonterminals f32[B,1], weights f32)."""
        o = self.sample_device(batch_size)
        states = torch.empty(o["states"].shape, dtype=torch.float32, device=self.device)
        next_states = torch.empty_like(states)
        n = states.numel()
        L.check(self._lib, self._lib.rb_u8_to_unit_f32(o["states"].data_ptr(), states.data_ptr(), n, self._stream()))
        L.check(self._lib, self._lib.rb_u8_to_unit_f32(o["next_states"].data_ptr(), next_states.data_ptr(), n, self._stream()))
        tree_idxs = o["tree_idxs"].cpu().numpy()      # the reference hands indices back as numpy (memory.py:155)
        hdr = self._header()
        if hdr.last_status != 0:
            raise RuntimeError("ReplayMemory.sample: no valid batch in %d attempts (buffer too small for batch?)"
                               % hdr.last_attempts)
        return (tree_idxs, states, o["actions"].clone(), o["returns"].clone(), next_states,
                o["nonterminals"].clone().unsqueeze(1), o["weights"].clone())

    def _stage_operands(self, idxs, priorities, stage_i, stage_p):
        """The operands of a deferred write-back in memory THIS object owns: `.to()` / `.contiguous()` hand a matching device
        tensor back as it is, and the reference's semantics are immediate (memory.py:157-159) — a caller may reuse its loss
        or index tensor right after the call.  Two slots per length, used in turn; an asynchronous device-to-device copy of
        <= 3 KB per operand that needs one (each costs the PER-only loop ~1.7 us per batch: `donate=True` skips them)."""
        n = int(idxs.numel())
        ring = self._stage.get(n)
        if ring is None:
            ring = self._stage[n] = [[torch.empty(n, dtype=torch.int64, device=self.device),
                                      torch.empty(n, dtype=torch.float32, device=self.device)] for _ in range(2)] + [0]
        slot = ring[ring[2]]
        ring[2] ^= 1
        if stage_i:
            slot[0].copy_(idxs.reshape(-1), non_blocking=True)
            idxs = slot[0]
        if stage_p:
            slot[1].copy_(priorities.reshape(-1), non_blocking=True)
            priorities = slot[1]
        return idxs, priorities

    def update_priorities(self, idxs, priorities, _immediate=False, donate=False):
        """memory.py:157-159.  Accepts numpy arrays (reference call site agent.py:100) or device tensors.  By default the
        write-back is recorded and rides in the next sample_device() launch (RAINBOW_AMD_LAZY_PRIORITIES); caller-owned device
        operands are copied at the call, so the caller's tensors are free again when this returns, as in the reference.
        donate=True (an extension): the caller will not modify its device operands before the next sample_device() / flush() —
        they are read in place when the write-back runs (no staging copy)."""
        d = self.device
        if not torch.is_tensor(idxs):
            idxs = torch.as_tensor(np.asarray(idxs, dtype=np.int64))
        if not torch.is_tensor(priorities):
            priorities = torch.as_tensor(np.asarray(priorities, dtype=np.float32))
        if self._pending is not None:
            self.flush()
        lazy = self._lazy and not _immediate and not torch.cuda.is_current_stream_capturing()
        if lazy:
            own_i = idxs.device != d or idxs.dtype != torch.int64 or not idxs.is_contiguous()
            own_p = priorities.device != d or priorities.dtype != torch.float32 or not priorities.is_contiguous()
            i_d = idxs.to(device=d, dtype=torch.int64).contiguous()
            p_d = priorities.to(device=d, dtype=torch.float32).contiguous()
            # (the index buffer sample_device() hands out is this object's: the launch that applies the write-back reads it
            # before its sampler part refills it)
            stage_i = not own_i and not donate and not any(o["tree_idxs"] is idxs for o in self._out.values())
            stage_p = not own_p and not donate
            if stage_i or stage_p:          # an operand is still the caller's own device tensor
                i_d, p_d = self._stage_operands(i_d, p_d, stage_i, stage_p)
            self._keep["upd"] = self._pending = (i_d, p_d)
            return
        i_d, p_d = self._keep["upd"] = (idxs.to(device=d, dtype=torch.int64).contiguous(),
                                        priorities.to(device=d, dtype=torch.float32).contiguous())
        L.check(self._lib, self._lib.rb_replay_update_priorities(self._handle, i_d.data_ptr(), p_d.data_ptr(), int(i_d.numel()),
                                                                 self._stream()))

    # validation iterator (memory.py:162-180)
    def __iter__(self):
        self.current_idx = 0
        return self

    def __next__(self):
        if self.current_idx == self.capacity:
            raise StopIteration
        out = torch.empty(self.history, 84, 84, dtype=torch.float32, device=self.device)
        L.check(self._lib, self._lib.rb_replay_state_at(self._handle, int(self.current_idx), out.data_ptr(), self._stream()))
        self.current_idx += 1
        return out

    next = __next__

    def states_at(self, indices):
        """[__next__ at index i for i in indices] as ONE launch: float32 [n, h, 84, 84] on the device (memory.py:167-178).
        `indices`: int64 device tensor or anything torch.as_tensor accepts, each in [0, capacity)."""
        idx = torch.as_tensor(indices, dtype=torch.int64).to(self.device).contiguous()
        n = int(idx.numel())
        if n and (int(idx.min()) < 0 or int(idx.max()) >= self.capacity):
            raise IndexError("states_at: index out of range")
        out = torch.empty(n, self.history, 84, 84, dtype=torch.float32, device=self.device)
        self._keep["idx"] = idx
        L.check(self._lib, self._lib.rb_replay_states_at(self._handle, idx.data_ptr(), n, out.data_ptr(), self._stream()))
        return out

    def priority_stats(self):
        """The shape of the priority distribution (rb_replay_priority_stats: one streamed pass over the leaves, on the device).
        A pending lazy update_priorities() is applied first, as a draw does; then the stream is synchronised.  Returns a dict:
        nonzero / invalid (leaf counts; invalid = NaN, inf or negative, excluded from the rest), sum, sumsq, max, min_pos (0 for
        an empty memory), ess = sum^2 / sumsq (the effective sample size; 0.0 when empty), hist (int32 [64]: bin k counts the
        leaves with floor(log2 p) == hist_lo_exp + k, clamped at both ends) and hist_lo_exp = -40."""
        if self._pending is not None:
            self.flush()
        out = self._keep.get("pstats")
        if out is None:
            out = self._keep["pstats"] = torch.empty(C.sizeof(L.PriorityStats), dtype=torch.uint8, device=self.device)
        L.check(self._lib, self._lib.rb_replay_priority_stats(self._h, out.data_ptr(), self._stream()))
        s = L.PriorityStats.from_buffer_copy(out.cpu().numpy().tobytes())      # (the copy synchronises)
        return dict(nonzero=int(s.nonzero), invalid=int(s.invalid), sum=float(s.sum), sumsq=float(s.sumsq), max=float(s.max),
                    min_pos=float(s.min_pos), ess=(s.sum * s.sum / s.sumsq) if s.sumsq > 0 else 0.0,
                    hist=np.array(s.hist, dtype=np.int32), hist_lo_exp=L.PRIORITY_HIST_LO_EXP)
