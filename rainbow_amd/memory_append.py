"""ReplayMemory's write side: append (memory.py:105-108), its batched and per-stream forms, and the per-stream episode
timesteps.  A mixin over the handle and the keep-alive container that rainbow_amd.memory.ReplayMemory owns."""
import numpy as np
import torch

from . import _lib as L
from ._util import f32_on


class ReplayAppend:
    def append(self, state, action, reward, terminal):
        """memory.py:105-108.  `state` float32 [h,84,84] in [0,1] on the device (env.py:52,77)."""
        self._one_stream("append")
        if self._stream_t_dev is not None:      # device rounds came before: fetch the episode timestep they left
            self.stream_t
        st = f32_on(state, self.device)
        rc = self._lib.rb_replay_append(self._h, st.data_ptr(), int(self.t), int(action), float(reward),
                                        0 if terminal else 1, self._stream())
        if rc != 0:
            L.check(self._lib, rc)
        self.t = 0 if terminal else self.t + 1
        self.stream_t[0] = self.t

    def _one_stream(self, what):
        if self.streams != 1:
            raise RuntimeError("ReplayMemory.%s: this memory interleaves %d environment streams; append whole rounds with "
                               "append_streams(states, actions, rewards, terminals)" % (what, self.streams))

    def append_streams(self, states, actions, rewards, terminals=None, nonterminals=None):
        """One round of memory.py:105-108 for every environment stream at once (one launch): `states` float32 [S,h,84,84] on
        the device (the batch Agent.act_batch just acted on), actions / rewards / terminals length-S sequences.  Stream s
        keeps its own episode timestep (stream_t[s]).  The same ring, tree and header as S appends in stream order.
        When actions, rewards and terminals are all torch tensors on this memory's device (Agent.act_batch(device_out=True),
        a rainbow_amd.envs environment) the round stays on the device: nothing is read back and nothing synchronises; the
        per-stream timesteps then live in a device vector (`stream_t` reads it back on demand).  On that path `terminals`
        (bool / uint8) is inverted on the device, or pass `nonterminals=` (uint8 device tensor, 1 = the episode goes on: what
        a rainbow_amd.envs environment keeps as `env.nonterminals`) instead and save that launch.  Host and device rounds
        may be mixed freely and give the same replay bit for bit."""
        S = self.streams
        st = f32_on(states, self.device)
        if tuple(st.shape) != (S, self.history, 84, 84):
            raise ValueError("append_streams: states must be [%d, %d, 84, 84], got %s" % (S, self.history, tuple(st.shape)))
        flags = nonterminals if nonterminals is not None else terminals
        if flags is None:
            raise ValueError("append_streams: give terminals or nonterminals")
        if all(torch.is_tensor(x) and x.is_cuda and (self.device.index is None or x.device.index == self.device.index)
               for x in (actions, rewards, flags)):
            return self._append_streams_device(st, actions, rewards, terminals, nonterminals)
        if nonterminals is not None:
            terminals = ~np.asarray(nonterminals.cpu() if torch.is_tensor(nonterminals) else nonterminals, dtype=bool)
        terminals = np.asarray(terminals.cpu() if torch.is_tensor(terminals) else terminals, dtype=bool).reshape(-1)
        ac = np.ascontiguousarray(np.asarray(actions.cpu() if torch.is_tensor(actions) else actions, dtype=np.int32).reshape(-1))
        rw = np.ascontiguousarray(np.asarray(rewards.cpu() if torch.is_tensor(rewards) else rewards, dtype=np.float32).reshape(-1))
        if len(terminals) != S or len(ac) != S or len(rw) != S:
            raise ValueError("append_streams: actions, rewards and terminals need %d entries each" % S)
        ts = self.stream_t              # (reads the device vector back first when device rounds came before)
        nt = (~terminals).astype(np.uint8)
        L.check(self._lib, self._lib.rb_replay_append_streams(self._h, st.data_ptr(), ts.ctypes.data, ac.ctypes.data, rw.ctypes.data,
                                                              nt.ctypes.data, self._stream()))
        self.stream_t = np.where(terminals, 0, ts + 1).astype(np.int32)       # memory.py:108, per stream
        if S == 1:
            self.t = int(self.stream_t[0])

    def _append_streams_device(self, st, actions, rewards, terminals, nonterminals):
        S = self.streams
        if actions.numel() != S or rewards.numel() != S or (nonterminals if nonterminals is not None else terminals).numel() != S:
            raise ValueError("append_streams: actions, rewards and terminals need %d entries each" % S)
        ac = actions if actions.dtype == torch.int32 and actions.is_contiguous() else actions.to(torch.int32).contiguous()
        rw = rewards if rewards.dtype == torch.float32 and rewards.is_contiguous() else rewards.to(torch.float32).contiguous()
        if nonterminals is not None:
            nt = nonterminals if nonterminals.dtype == torch.uint8 and nonterminals.is_contiguous() else (nonterminals != 0).contiguous()
        else:
            nt = (terminals == 0).contiguous()                  # nonterminal = 1 - terminal on the device (a bool tensor is one 0 / 1 byte each)
        if self._stream_t_dev is None:                          # host rounds (or none) came before: continue from their counters
            if not np.any(self._stream_t_host):                 # (a fresh memory: a fill, no synchronising upload)
                self._stream_t_dev = torch.zeros(S, dtype=torch.int32, device=self.device)
            else:
                self._stream_t_dev = torch.from_numpy(np.ascontiguousarray(self._stream_t_host, dtype=np.int32)).to(self.device)
        self._keep["dev_round"] = (st, ac, rw, nt)              # operands stay alive until the next round replaces them
        rc = self._lib.rb_replay_append_streams_dev(self._h, st.data_ptr(), self._stream_t_dev.data_ptr(), ac.data_ptr(),
                                                    rw.data_ptr(), nt.data_ptr(), self._stream())
        if rc != 0:
            L.check(self._lib, rc)

    # the per-stream episode timesteps: a host array while rounds come with host operands, a device vector (updated by the
    # append kernel) while they come with device operands.  Reading `stream_t` is always truthful: it fetches the device
    # vector (one small synchronising copy) and hands the counters back to the host side; save_to and pickling go through it.
    @property
    def stream_t(self):
        if self._stream_t_dev is not None:
            self._stream_t_host = self._stream_t_dev.cpu().numpy().astype(np.int32)
            self._stream_t_dev = None
            if self.streams == 1:
                self.t = int(self._stream_t_host[0])
        return self._stream_t_host

    @stream_t.setter
    def stream_t(self, value):
        self._stream_t_host = value
        self._stream_t_dev = None

    def append_batch(self, frames_u8, actions, rewards, terminals):
        """n sequential appends of already-quantised last frames (uint8 [n,84,84], device)."""
        self._one_stream("append_batch")
        if self._stream_t_dev is not None:
            self.stream_t
        n = int(frames_u8.shape[0])
        terminals = np.asarray(terminals, dtype=bool)
        ts = np.empty(n, dtype=np.int32)
        t = self.t
        for i in range(n):
            ts[i] = t
            t = 0 if terminals[i] else t + 1
        self.t = t
        self.stream_t[0] = t
        d = self.device
        fr = frames_u8.to(device=d, dtype=torch.uint8).contiguous()
        ts_d = torch.from_numpy(ts).to(d)
        ac_d = torch.as_tensor(np.asarray(actions, dtype=np.int32)).to(d)
        rw_d = torch.as_tensor(np.asarray(rewards, dtype=np.float32)).to(d)
        nt_d = torch.from_numpy((~terminals).astype(np.uint8)).to(d)
        L.check(self._lib, self._lib.rb_replay_append_batch(self._h, fr.data_ptr(), ts_d.data_ptr(), ac_d.data_ptr(),
                                                            rw_d.data_ptr(), nt_d.data_ptr(), n, self._stream()))
        torch.cuda.current_stream(d).synchronize()   # the temporaries above must outlive the kernels
