"""Frame preprocessing of the reference's environment wrapper on the device.

env.py:27-29   `_get_state`: cv2.resize(ale.getScreenGrayscale(), (84, 84), INTER_LINEAR) -> float32 / 255
env.py:57-69   `step`: the observation is the element-wise max of the states after frames 3 and 4 of the action repeat

`FramePreprocessor.observe(frame_a, frame_b)` takes the raw u8 grayscale screens (torch uint8 tensors on the device, or
numpy arrays / CPU tensors, which are uploaded as 33 KB of bytes instead of 28 KB of float32 per state after a host-side
resize) and returns the float32 [84, 84] observation on the device, ready for the state deque of env.py:25,70 and for
`ReplayMemory.append`.  The resize is OpenCV's fixed-point 8-bit INTER_LINEAR restated (include/rainbow_hip.h
rb_frame_preprocess): parity with cv2 itself is UNPINNED because cv2 is absent from the build container."""
import numpy as np
import torch

from . import _lib as L


class FramePreprocessor:
    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rainbow_amd.frames runs on MI355X: device must be a cuda (ROCm) device, got %s" % self.device)
        self._lib = L.load()

    def _dev_u8(self, f):
        if f is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
        if t.dtype != torch.uint8:
            raise TypeError("raw frames are uint8 grayscale screens (ale.getScreenGrayscale()), got %s" % t.dtype)
        return t.to(self.device).contiguous()

    def observe(self, frame_a, frame_b=None):
        """[H, W] u8 (+ optional second frame) -> float32 [84, 84];  [n, H, W] batches -> [n, 84, 84] (vectorised actors)."""
        a, b = self._dev_u8(frame_a), self._dev_u8(frame_b)
        if b is not None and b.shape != a.shape:
            raise ValueError("the two frames of a max-pool pair must have the same shape")
        batched = a.dim() == 3
        if a.dim() not in (2, 3):
            raise ValueError("frames are [H, W] or [n, H, W]")
        n = int(a.shape[0]) if batched else 1
        H, W = int(a.shape[-2]), int(a.shape[-1])
        out = torch.empty((n, 84, 84), dtype=torch.float32, device=self.device)
        L.check(self._lib, self._lib.rb_frame_preprocess(a.data_ptr(), b.data_ptr() if b is not None else None, H, W, n,
                                                         out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
        self._keep = (a, b)            # inputs stay alive until the stream has consumed them
        return out if batched else out[0]


class FrameStackVec:
    """The frame stacks of S host emulators, on the device.  Per round the caller fills `.screens` (u8 [S, 2, H, W]: the
    screens after frames 3 and 4 of each stream's action repeat; `screens[s, 0]` and `screens[s, 1]` are contiguous [H, W]
    arrays an emulator can write `getScreenGrayscale` straight into) and calls `step(flags)` with one flag byte per stream:

        STEP = FRAME_A | FRAME_B    env.py:58-68, the whole repeat ran
        RESET = BLANK | FRAME_A     env.py:40-52, a new game: history - 1 blank frames, then the first observation
        LIFE_RESET = FRAME_A        env.py:36-38,49-52, the no-op after a lost life (no blanking); also a repeat that was cut
                                    after its third frame (env.py:60-66)
        0                           a repeat cut before its third frame: the observation is zeros (env.py:56,67)

    `step` uploads the slot with one non-blocking copy on the current stream, launches once, and returns the device tensor
    [S, h, 84, 84] (also with one stream: Agent.act_batch and ReplayMemory.append_streams take that shape).  It never
    synchronises the stream.  Two stack buffers are used in turn: what a step hands out stays valid until the step after the
    next one, so `states` can still be appended after `next_states` was produced.  The staging has two slots as well: the
    `.screens` view for the next call may be filled as soon as `step` returns."""
    BLANK, FRAME_A, FRAME_B = L.OBS_BLANK, L.OBS_FRAME_A, L.OBS_FRAME_B
    STEP = FRAME_A | FRAME_B
    RESET = BLANK | FRAME_A
    LIFE_RESET = FRAME_A

    def __init__(self, streams, device, history_length=4, height=210, width=160):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rainbow_amd.frames runs on MI355X: device must be a cuda (ROCm) device, got %s" % self.device)
        self._lib = L.load()
        self.streams, self.history, self.height, self.width = int(streams), int(history_length), int(height), int(width)
        S, H, W = self.streams, self.height, self.width
        if not 1 <= S <= 64:
            raise ValueError("FrameStackVec: streams must be in [1, 64], got %d" % S)
        if not 1 <= self.history <= 16:
            raise ValueError("FrameStackVec: history_length must be in [1, 16], got %d" % self.history)
        if not (2 <= H <= 4096 and 2 <= W <= 4096):
            raise ValueError("FrameStackVec: the screen size must be in [2, 4096]^2, got %d x %d" % (H, W))
        self._stacks = [torch.zeros(S, self.history, 84, 84, dtype=torch.float32, device=self.device) for _ in range(2)]
        self._cur = 0
        # a slot is stored [2, S, H, W] (all A screens, then all B screens: the [S][H][W] arrays the kernel takes, one
        # contiguous upload) and handed out as the [S, 2, H, W] view
        self._host = [torch.zeros(2, S, H, W, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._views = [h.numpy().transpose(1, 0, 2, 3) for h in self._host]
        self._dev = [torch.zeros(2, S, H, W, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._uploaded = [None, None]         # per slot: the event behind its last upload
        self._slot = 0
        self._flags = np.zeros(S, dtype=np.uint8)

    @property
    def screens(self):
        """numpy u8 [S, 2, H, W]: the staging slot the next step / reset_all uploads."""
        return self._views[self._slot]

    def _fill(self, screens):
        src = screens.numpy() if torch.is_tensor(screens) else np.asarray(screens)
        if src.dtype != np.uint8:
            raise TypeError("raw frames are uint8 grayscale screens (ale.getScreenGrayscale()), got %s" % src.dtype)
        S, H, W = self.streams, self.height, self.width
        if src.shape == (S, 2, H, W):
            np.copyto(self._views[self._slot], src)
        elif src.shape == (S, H, W):
            np.copyto(self._views[self._slot][:, 0], src)
        else:
            raise ValueError("screens must be [%d, 2, %d, %d] or [%d, %d, %d], got %s" % (S, H, W, S, H, W, tuple(src.shape)))

    def _launch(self, flags, a_ptr, b_ptr):
        self._flags[:] = flags                # (raises on a wrong length; values above 7 are refused by the library)
        cur, nxt = self._cur, self._cur ^ 1
        rc = self._lib.rb_obs_stack_step(a_ptr, b_ptr, self.height, self.width, self.streams, self.history,
                                         self._flags.ctypes.data, self._stacks[cur].data_ptr(), self._stacks[nxt].data_ptr(),
                                         torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            L.check(self._lib, rc)
        self._cur = nxt
        return self._stacks[nxt]

    def step(self, flags, screens=None):
        """flags: one int for every stream, or S of them.  -> f32 [S, h, 84, 84] on the device, final in stream order."""
        if screens is not None:
            self._fill(screens)
        k = self._slot
        self._dev[k].copy_(self._host[k], non_blocking=True)
        ev = self._uploaded[k] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._uploaded[k] = ev
        out = self._launch(flags, self._dev[k][0].data_ptr(), self._dev[k][1].data_ptr())
        self._slot = k ^ 1
        # the slot handed out next was uploaded by the call before this one: wait for THAT copy (an event, not the stream;
        # it is a round old and normally long done) so that the caller may overwrite the view at once
        prev = self._uploaded[k ^ 1]
        if prev is not None and not prev.query():
            prev.synchronize()
        return out

    def step_device(self, flags, frames_a, frames_b=None):
        """The same round from screens that are already on the device (u8 [S, H, W] each, contiguous): no upload."""
        for f in (frames_a, frames_b):
            if f is not None and (f.dtype != torch.uint8 or f.device != self._dev[0].device or not f.is_contiguous()
                                  or tuple(f.shape) != (self.streams, self.height, self.width)):
                raise ValueError("step_device: frames are contiguous uint8 [%d, %d, %d] tensors on %s"
                                 % (self.streams, self.height, self.width, self.device))
        self._frames = (frames_a, frames_b)   # inputs stay alive until the stream has consumed them
        return self._launch(flags, frames_a.data_ptr() if frames_a is not None else None,
                            frames_b.data_ptr() if frames_b is not None else None)

    def reset_all(self, screens=None):
        """Every stream starts a new game from `screens[:, 0]` (env.py:40-52)."""
        return self.step(self.RESET, screens)
