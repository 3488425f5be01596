"""Small host-side helpers the package's modules share (no library handle, no state)."""
import torch

# torch.cuda.current_stream(device).cuda_stream builds a Stream object per call (~4 us: a tenth of one act()); the raw handle
# of the same current stream is one C call (what torch's own compiled-kernel launchers use)
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_handle(device):
    if _RAW_STREAM is not None:
        return _RAW_STREAM(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def f32_on(t, device):
    """`t` as a contiguous float32 tensor on `device` (itself when it already is one: env.py hands over exactly this)."""
    if t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    return t


_U64 = 0xFFFFFFFFFFFFFFFF


def u64_pair(rng):
    """rng = (seed, round) as the two 64-bit words of a Philox key / counter (negative values wrap)."""
    return int(rng[0]) & _U64, int(rng[1]) & _U64
