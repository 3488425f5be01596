"""ReplayMemory's saved state: the table of its device columns, the streaming dump / restore (save_to / load_from) and
pickling (main.py:94-100,118).  A mixin over the handle that rainbow_amd.memory.ReplayMemory owns."""
import ctypes as C
import json
import struct
import types

import numpy as np
import torch

from . import _lib as L

FRAME_BYTES = 84 * 84          # one uint8 frame of the ring

# the device columns in the order save_to streams them: name, ReplayBuffers field, bytes per row, numpy dtype (the tree has
# tree_len rows, every other column `capacity`)
_COLUMNS = (("tree", "sum_tree_dev", 4, np.float32), ("frames", "frames_dev", FRAME_BYTES, np.uint8),
            ("timestep", "timestep_dev", 4, np.int32), ("action", "action_dev", 4, np.int32),
            ("reward", "reward_dev", 4, np.float32), ("nonterminal", "nonterminal_dev", 1, np.uint8))


class ReplayState:
    # what _init_runtime() builds: library handles, caches and keep-alives, none of it part of the saved state
    _RUNTIME = ("_lib", "_handle", "_pending", "_stage", "_keep", "_out", "_bufs", "_neg_beta_dev", "_neg_beta_val", "transitions",
                "_stream_t_dev", "_stream_t_host")

    def _columns(self):
        """(ReplayBuffers, {name: (device pointer, bytes per row, numpy dtype, rows)}); applies a pending write-back first."""
        b = L.ReplayBuffers()
        L.check(self._lib, self._lib.rb_replay_buffers(self._h, C.byref(b)))
        return b, {name: (getattr(b, field), row, dtype, b.tree_len if name == "tree" else self.capacity)
                   for name, field, row, dtype in _COLUMNS}

    def _to_host(self, ptr, nbytes):
        host = np.empty(nbytes, dtype=np.uint8)
        L.check(self._lib, self._lib.rb_copy_to_host(host.ctypes.data, ptr, nbytes, self._stream()))
        return host

    def _upload_header(self, b, raw):
        hdr = np.frombuffer(raw, dtype=np.uint8).copy()
        L.check(self._lib, self._lib.rb_copy_to_device(b.header_dev, hdr.ctypes.data, hdr.nbytes, self._stream()))

    # ------------------------------------------------------------------ streaming dump / restore
    def save_to(self, fileobj, chunk_bytes=64 << 20):
        """Streams the replay to a binary file object in `chunk_bytes` pieces (64 MB of host staging instead of the 7 GB
        a pickle of a 1M-capacity memory needs; main.py:94-100 `pickle.dump(memory, bz2 file)` still works through
        __getstate__, this is the scalable alternative: `with bz2.open(path, 'wb') as f: mem.save_to(f)`)."""
        b, cols = self._columns()
        hdr = self._header()
        self.stream_t             # (fetches the device-resident counters after device rounds; refreshes self.t)
        meta = dict(version=1, capacity=self.capacity, history=self.history, n=self.n, discount=self.discount,
                    horizon=int(self.horizon), priority_weight=self.priority_weight, priority_exponent=self.priority_exponent, t=self.t,
                    streams=self.streams, stream_t=[int(x) for x in self.stream_t], seed=self._seed,
                    augment_pad=int(self.augment_pad), aug_draw=int(self._aug_draw),
                    columns={k: rows * row for k, (_p, row, _d, rows) in cols.items()}, header=bytes(hdr).hex())
        blob = json.dumps(meta).encode()
        fileobj.write(b"RBRPLY01" + struct.pack("<q", len(blob)) + blob)
        stage = np.empty(chunk_bytes, dtype=np.uint8)
        for ptr, row, _dtype, rows in cols.values():
            nbytes = rows * row
            for lo in range(0, nbytes, chunk_bytes):
                m = min(chunk_bytes, nbytes - lo)
                L.check(self._lib, self._lib.rb_copy_to_host(stage.ctypes.data, ptr + lo, m, self._stream()))
                fileobj.write(stage[:m].tobytes() if m < chunk_bytes else stage.data)

    @classmethod
    def load_from(cls, fileobj, device, chunk_bytes=64 << 20):
        """Inverse of save_to: builds a ReplayMemory on `device` from the stream."""
        magic = fileobj.read(8)
        if magic != b"RBRPLY01":
            raise ValueError("not a rainbow_amd replay stream")
        (n,) = struct.unpack("<q", fileobj.read(8))
        meta = json.loads(fileobj.read(n).decode())
        args = types.SimpleNamespace(device=device, history_length=meta["history"], discount=meta["discount"],
                                     multi_step=meta["n"], priority_weight=meta["priority_weight"],
                                     priority_exponent=meta["priority_exponent"],
                                     augment_pad=meta.get("augment_pad", 0))                  # (older streams: no augmentation)
        mem = cls(args, meta["capacity"], seed=meta["seed"], streams=meta.get("streams", 1))   # (older streams: one stream)
        mem._aug_draw = int(meta.get("aug_draw", 0))
        horizon = int(meta.get("horizon", meta["n"]))            # (older streams: the horizon of construction)
        if horizon != mem.n:
            mem.set_horizon(horizon)                             # (meta["discount"] is the discount that was in force)
        mem.t = meta["t"]
        mem.stream_t = np.array(meta.get("stream_t", [meta["t"]]), dtype=np.int32)
        b, cols = mem._columns()
        for k, (ptr, row, _dtype, rows) in cols.items():
            nbytes = rows * row
            if nbytes != meta["columns"][k]:
                raise ValueError("replay stream column %s has %d bytes, expected %d" % (k, meta["columns"][k], nbytes))
            for lo in range(0, nbytes, chunk_bytes):
                m = min(chunk_bytes, nbytes - lo)
                buf = fileobj.read(m)
                if len(buf) != m:
                    raise EOFError("replay stream truncated in column %s" % k)
                a = np.frombuffer(buf, dtype=np.uint8)
                L.check(mem._lib, mem._lib.rb_copy_to_device(ptr + lo, a.ctypes.data, m, mem._stream()))
        mem._upload_header(b, bytes.fromhex(meta["header"]))
        return mem

    # ------------------------------------------------------------------ pickling (main.py:94-100,118)
    def _grab(self, field, start=0, count=None):
        """Copies rows [start, start+count) of one device column to a numpy array (tests / partial dumps)."""
        ptr, row, dtype, rows = self._columns()[1][field]
        count = rows - start if count is None else count
        out = self._to_host(ptr + start * row, count * row).view(dtype)
        return out.reshape(count, 84, 84) if field == "frames" else out

    def _dump(self):
        b, cols = self._columns()
        hdr = self._header()
        dump = {k: self._to_host(ptr, rows * row).view(dtype) for k, (ptr, row, dtype, rows) in cols.items()}
        dump["header"] = bytes(hdr)
        return dump

    def __getstate__(self):
        dump = self._dump()       # (applies a pending priority write-back first)
        stream_t = self.stream_t  # (fetches the device-resident counters after device rounds)
        st = {k: v for k, v in self.__dict__.items() if k not in self._RUNTIME}
        st["device"] = str(self.device)
        st["stream_t"] = stream_t
        st["_dump"] = dump
        return st

    def __setstate__(self, st):
        dump = st.pop("_dump")
        stream_t = st.pop("stream_t", None)
        self.__dict__.update(st)
        self.augment_pad = self._checked_pad(st.get("augment_pad", 0))      # (a pickle from before the option: off, draw 0)
        self._aug_draw = int(st.get("_aug_draw", 0))
        if self.horizon is None:                                             # (a pickle from before set_horizon: the horizon of construction)
            self.horizon = self.n
        self.device = torch.device(self.device)
        # (a pickle from before interleaved streams: one stream)
        self.stream_t = np.array([self.t], dtype=np.int32) if stream_t is None else np.asarray(stream_t, dtype=np.int32)
        self._init_runtime()
        b, cols = self._columns()
        for k, (ptr, _row, _dtype, _rows) in cols.items():
            a = np.ascontiguousarray(dump[k])
            L.check(self._lib, self._lib.rb_copy_to_device(ptr, a.ctypes.data, a.nbytes, self._stream()))
        self._upload_header(b, dump["header"])
        self._header()   # resynchronise the library's host mirror of index/full
