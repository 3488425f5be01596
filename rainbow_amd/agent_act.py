"""Agent's act and evaluate paths (agent.py:53-59,110-112 and their batched forms): a mixin over the learner handle, the pinned
result buffers and the noise state that rainbow_amd.agent.Agent owns."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._util import current_stream_handle, f32_on, u64_pair


class AgentAct:
    def _forward_single(self, state):
        """One state through the act path; the action / value land in PINNED host memory the kernel writes directly
        (no device-to-host copy): they are final after the stream synchronize below."""
        if self._noise_pending:
            self._flush_noise()
        st = f32_on(state, self.device)
        pins = self._aq_ptrs
        # launch + wait in ONE C call: completion = the pinned action word changes (the head writes action and q as one 8-byte word);
        # the library polls it in a compiled loop (a Python loop over a numpy scalar sees the store a microsecond or two late),
        # falls back to a stream synchronise, and retries once when the one-launch path reports an expired in-launch wait
        rc = self._lib.rb_learner_act_wait(self._h, st.data_ptr(), 1 if self.training else 0, pins[0], pins[1], None, None,
                                           current_stream_handle(self.device))
        if rc != 0:
            L.check(self._lib, rc)

    def act(self, state):
        """agent.py:53-55: greedy action on the expected value of the (noisy) online distribution."""
        self._forward_single(state)
        return int(self._aq_act[0])

    def reset_noise_rows(self, rows, rng=(0, 0), raw_normals=None):
        """One noise sample per ROW for act_batch(per_row_noise=True): fills the agent-owned [rows, n_noise] device tensor
        (regrown when `rows` grows), a launch in stream order and no synchronisation.  rng = (seed, round): row r is drawn
        from Philox(key = seed, counter = (hi = round, lo = (r << 32) | pair)) — it depends on (seed, round, r) only; the
        learner's own noise generator (reset_noise, learn) is neither read nor advanced.  raw_normals (parity hook): float32
        [rows, noise draws] of N(0,1) in the reference's order, one block per row.  The rows are redrawn before use and are
        not part of state_dict / checkpoints."""
        rows = int(rows)
        if rows < 1:
            raise ValueError("reset_noise_rows: rows must be >= 1, got %d" % rows)
        n_noise = int(self.noise.numel())
        if self._noise_rows is None or int(self._noise_rows.shape[0]) < rows:
            self._noise_rows = torch.zeros((rows, n_noise), dtype=torch.float32, device=self.device)
        raw = None
        if raw_normals is not None:
            raw = raw_normals.to(device=self.device, dtype=torch.float32).contiguous()
            draws = int(self._lib.rb_learner_noise_draws(C.byref(self._cfg)))
            if tuple(raw.shape) != (rows, draws):
                raise ValueError("reset_noise_rows: raw_normals must be [%d, %d], got %s" % (rows, draws, tuple(raw.shape)))
            self._keep["raw_rows"] = raw              # kept alive until the stream has consumed it
        seed, rnd = u64_pair(rng)
        for lo in range(0, rows, 256):
            m = min(256, rows - lo)
            rc = self._lib.rb_learner_noise_rows(self._h, m, lo, seed, rnd, raw[lo:lo + m].data_ptr() if raw is not None else None,
                                                 self._noise_rows[lo:lo + m].data_ptr(), self._stream())
            if rc != 0:
                L.check(self._lib, rc)
        self._noise_rows_drawn = rows

    def _run_chunked(self, st, device_out, cap, read_q, call):
        """The batched act path over `st`, at most `cap` states per C call: call(state_ptr, m, lo, action_ptr, q_ptr) issues the
        call for states [lo, lo + m) and returns its status.  device_out: the actions go straight into an int32 device tensor, q is
        not asked for and nothing synchronises.  Otherwise both land in the pinned buffers, the stream is synchronised once per
        chunk and the pinned actions (int64) or, with read_q, the pinned q (float32) are copied out."""
        n = int(st.shape[0])
        acts = torch.empty(n, dtype=torch.int32, device=self.device) if device_out else None
        out = None if device_out else np.empty(n, dtype=np.float32 if read_q else np.int64)
        for lo in range(0, n, cap):
            m = min(cap, n - lo)
            if device_out:
                rc = call(st[lo:lo + m].data_ptr(), m, lo, acts[lo:lo + m].data_ptr(), None)
            else:
                rc = call(st[lo:lo + m].data_ptr(), m, lo, self._act_pin.data_ptr(), self._q_pin.data_ptr())
            if rc != 0:
                L.check(self._lib, rc)
            if not device_out:
                torch.cuda.current_stream(self.device).synchronize()
                out[lo:lo + m] = (self._q_np if read_q else self._act_np)[:m]
        return acts if device_out else out

    def act_batch(self, states, device_out=False, epsilon=None, rng=(0, 0), row0=0, per_row_noise=False):
        """Vectorised actors: `states` f32 [n, h, 84, 84] on the device (processed 2*batch_size at a time).
        Returns the n greedy actions (numpy int64), i.e. [self.act(s) for s in states] in one forward.
        device_out=True: the actions stay on the device — an int32 [n] tensor, final in stream order — and the call does NOT
        synchronise (for an environment that lives on the device: rainbow_amd.envs, ReplayMemory.append_streams).
        epsilon (None = the greedy path, as before): act_e_greedy (agent.py:58-59) for every state, drawn in the head kernel
        (rb_learner_act_batch_eps): state i explores iff its uniform from Philox(key = rng[0], counter = (lo = rng[1], hi = i))
        is below epsilon, and then takes that block's second word modulo the action count.  rng = (seed, round): the caller
        advances `round` once per call; a state's draw depends on (seed, round, row0 + i) only, not on the chunking here, and
        a caller that splits one round's states over several calls passes the number of each part's first state as row0.
        per_row_noise=True (training mode): state i runs the noisy layers under noise row row0 + i of the last
        reset_noise_rows() (rb_learner_act_batch_rows: every stream of a vectorised actor explores with its own draw); the
        result does not depend on the chunking.  In eval() mode the flag is ignored (no noise at all); together with
        `epsilon`, or with fewer rows drawn than states passed, it raises ValueError."""
        if per_row_noise and epsilon is not None:
            raise ValueError("act_batch: per_row_noise and epsilon cannot be combined")
        lib, h = self._lib, self._h
        cap = int(self._act_np.shape[0])               # 2 * batch_size images fit the learner's activation buffers
        if per_row_noise and self.training:
            row0 = int(row0)
            st = f32_on(states, self.device)           # (no _flush_noise: the learner's own sample is not read)
            n = int(st.shape[0])
            if row0 < 0:
                raise ValueError("act_batch: row0 must be >= 0, got %d" % row0)
            if row0 + n > self._noise_rows_drawn:
                raise ValueError("act_batch(per_row_noise=True): states %d .. %d need noise rows, reset_noise_rows drew %d"
                                 % (row0, row0 + n - 1, self._noise_rows_drawn))
            cap = min(cap, 256)

            def call(sp, m, lo, ap, qp):
                return lib.rb_learner_act_batch_rows(h, sp, m, self._noise_rows[row0 + lo:row0 + lo + m].data_ptr(), ap, qp, self._stream())
        else:
            if epsilon is not None:
                epsilon, row0 = float(epsilon), int(row0)
                seed, rnd = u64_pair(rng)
            self._flush_noise()
            st = f32_on(states, self.device)
            noisy = 1 if self.training else 0

            def call(sp, m, lo, ap, qp):
                if epsilon is None:
                    return lib.rb_learner_act_batch(h, sp, m, noisy, ap, qp, self._stream())
                return lib.rb_learner_act_batch_eps(h, sp, m, noisy, epsilon, seed, rnd, row0 + lo, ap, qp, None, self._stream())
        return self._run_chunked(st, device_out, cap, False, call)

    def act_e_greedy(self, state, epsilon=0.001):
        """agent.py:58-59."""
        return np.random.randint(0, self.action_space) if np.random.random() < epsilon else self.act(state)

    def evaluate_q(self, state):
        """agent.py:110-112."""
        self._forward_single(state)
        return float(self._aq_q[1])

    def evaluate_q_batch(self, states, chunk=512):
        """Batched agent.py:110-112: `states` f32 [n, h, 84, 84] on the device -> numpy float32 [n],
        [self.evaluate_q(s) for s in states] as ONE forward per `chunk` states (6 launches for a 500-state validation
        memory, test.py:38-39, instead of 500 single-state launch chains with a stream sync each)."""
        self._flush_noise()
        st = f32_on(states, self.device)
        noisy = 1 if self.training else 0
        chunk = max(1, min(int(chunk), 4096))
        need = min(int(st.shape[0]), chunk)
        if self._q_pin.numel() < need:
            self._act_pin = torch.zeros(need, dtype=torch.int32).pin_memory()
            self._q_pin = torch.zeros(need, dtype=torch.float32).pin_memory()
            self._act_np, self._q_np = self._act_pin.numpy(), self._q_pin.numpy()
        return self._run_chunked(st, False, chunk, True,
                                 lambda sp, m, lo, ap, qp: self._lib.rb_learner_act_batch(self._h, sp, m, noisy, ap, qp, self._stream()))

    def evaluate_q_memory(self, val_mem, chunk=512):
        """test.py:38-39 in one call: Q of every state the reference's `for state in val_mem` visits — ALL `capacity` slots
        (memory.py:166-168 walks data indices 0 .. capacity-1 whether or not they were ever written; unwritten slots are
        blank states) — built on the device by rb_replay_states_at."""
        n = val_mem.capacity
        qs = np.empty(n, dtype=np.float32)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            qs[lo:hi] = self.evaluate_q_batch(val_mem.states_at(torch.arange(lo, hi, device=self.device)), chunk)
        return qs
