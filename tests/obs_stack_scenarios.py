"""Checks of rb_obs_stack_step (the S-stream observation front end) shared by the host-interpreter tests
(test_obs_stack_emu.py) and the device tests (test_obs_stack_gpu.py): the same code drives either build through the C ABI;
tests/obs_stack_oracle.py (env.py's deque per stream over oracle/frame_oracle.py's resize) is the oracle.  Every comparison is
bit-exact: the newest frame is integer arithmetic divided by 255, the others are copies."""
import numpy as np

import obs_stack_oracle as OO
from rainbow_amd import _lib as L

from oracle import frame_oracle as F

ROUNDS = 40
# The resized states of a script's screens do not depend on the history length: the cases that differ only in it run one after
# the other and share them (the reference is computed once).  One script's states are kept at a time.
_memo = {"key": None, "states": {}}


def _memoised_get_state(key):
    if _memo["key"] != key:
        _memo["key"], _memo["states"] = key, {}
    states = _memo["states"]

    def get_state(screen):
        k = screen.tobytes()[:64], int(screen.sum())          # (a screen of this script: 64 random bytes and the sum name it)
        if k not in states:
            states[k] = F.get_state(screen)
        return states[k]
    return get_state


def make_screens(rs, S, H, W):
    """Random u8 screens with a flat patch, as test_frames._screens."""
    a = rs.randint(0, 256, size=(S, H, W)).astype(np.uint8)
    a[:, H // 4:H // 2 + 10, W // 5:W // 2 + 10] = rs.randint(0, 256, size=(S, 1, 1)).astype(np.uint8)
    return a


def build_script(S, seed, rounds=ROUNDS):
    """u8 [rounds, S] of flag bytes: mostly STEP, every one of the eight values for every stream (so for both stream-index
    parities), a RESET of every stream in rounds 0 and 1 (several streams in one round; a RESET directly after a RESET)."""
    rs = np.random.RandomState(seed)
    flags = np.where(rs.random_sample((rounds, S)) < 0.6, OO.STEP, rs.randint(0, 8, size=(rounds, S))).astype(np.uint8)
    for s in range(S):
        for v in range(8):
            flags[5 * v + 2 + s % 3, s] = v
    flags[0, :] = OO.RESET
    flags[1, :] = OO.RESET
    for parity in range(min(S, 2)):
        seen = set(int(x) for x in flags[:, parity::2].reshape(-1))
        assert seen == set(range(8)), (parity, seen)
    for s in range(S):
        assert set(int(x) for x in flags[:, s]) == set(range(8))
    assert (flags[0] == OO.RESET).all() and (flags[1] == OO.RESET).all()
    if S > 1:
        assert int((flags[0] == OO.RESET).sum()) > 1
    return flags


def scripted_rounds(S, history, H, W, seed, fill=0.5):
    """Yields (flags u8 [S], frames_a, frames_b u8 [S, H, W], expected stacks f32 [S, history, 84, 84]) round by round.  The
    stacks start from a non-zero fill, so a BLANK that did nothing shows."""
    script = build_script(S, seed)
    rs = np.random.RandomState(seed + 1)
    ora = OO.StackOracle(S, history, fill)
    get_state = _memoised_get_state((S, H, W, seed))
    for r in range(len(script)):
        a, b = make_screens(rs, S, H, W), make_screens(rs, S, H, W)
        yield script[r], a, b, ora.apply(script[r], a, b, get_state)


class StackPair:
    """Two caller-owned stack buffers used in turn, as FrameStackVec does."""

    def __init__(self, lib, mem, S, history, H, W, fill=0.5):
        self.lib, self.mem, self.S, self.history, self.H, self.W = lib, mem, S, history, H, W
        self.bufs = [mem.upload(np.full((S, history, 84, 84), fill, dtype=np.float32)) for _ in range(2)]
        self.cur = 0

    def step(self, flags, a, b):
        m = self.mem
        da = m.upload(a) if a is not None else None
        db = m.upload(b) if b is not None else None
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        L.check(self.lib, self.lib.rb_obs_stack_step(m.ptr(da), m.ptr(db), self.H, self.W, self.S, self.history, fl.ctypes.data,
                                                     m.ptr(self.bufs[self.cur]), m.ptr(self.bufs[self.cur ^ 1]), m.stream))
        fl[:] = 255                       # the flags travelled by value: the caller's array is free again
        m.sync()
        self.cur ^= 1
        return m.download(self.bufs[self.cur])


def check_scripted(lib, mem, S, history, H=210, W=160, seed=0):
    """40 scripted rounds: the stacks after every round equal the oracle's."""
    pair = StackPair(lib, mem, S, history, H, W)
    for r, (flags, a, b, want) in enumerate(scripted_rounds(S, history, H, W, seed)):
        got = pair.step(flags, a, b)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(got, want), (S, history, H, W, r, [int(f) for f in flags])


def check_newest_frame_equals_frame_preprocess(lib, mem):
    """The newest frame of a STEP is rb_frame_preprocess on the same screens, bit for bit."""
    S, H, W = 3, 210, 160
    rs = np.random.RandomState(77)
    a, b = make_screens(rs, S, H, W), make_screens(rs, S, H, W)
    got = StackPair(lib, mem, S, 4, H, W).step([OO.STEP] * S, a, b)
    da, db, out = mem.upload(a), mem.upload(b), mem.empty((S, 84, 84), np.float32)
    L.check(lib, lib.rb_frame_preprocess(mem.ptr(da), mem.ptr(db), H, W, S, mem.ptr(out), mem.stream))
    mem.sync()
    assert np.array_equal(got[:, -1], mem.download(out))


def check_null_frames(lib, mem):
    """frames_b_dev == NULL with rounds that only name FRAME_A; frames_a_dev == NULL (and both NULL) with rounds of 0 / BLANK."""
    S, history, H, W = 3, 4, 210, 160
    rs = np.random.RandomState(5)
    pair, ora = StackPair(lib, mem, S, history, H, W), OO.StackOracle(S, history, 0.5)
    script = [([3, 2, 3], "a"), ([2, 2, 2], "a"), ([0, 1, 0], "b"), ([2, 3, 2], "a"), ([1, 0, 0], None), ([0, 0, 1], "b"),
              ([2, 2, 3], "a"), ([0, 0, 0], None)]
    for r, (flags, present) in enumerate(script):
        scr = make_screens(rs, S, H, W)
        a = scr if present == "a" else None
        b = scr if present == "b" else None                   # (a B pointer whose frames no flag names is never read)
        got = pair.step(flags, a, b)
        assert np.array_equal(got, ora.apply(flags, a, b)), r


def check_refusals(lib, mem):
    """Every refusal of include/rainbow_hip.h: RB_ERR_INVALID, the entry point and the argument named, nothing launched."""
    S, h, H, W = 2, 4, 210, 160
    n = S * h * 84 * 84
    big = mem.upload(np.full(2 * n + 84 * 84 + 8, 0.25, dtype=np.float32))
    base = mem.ptr(big)
    assert base % 16 == 0
    sin, sout = base, base + 4 * (n + 84 * 84)
    a, b = mem.upload(np.zeros((S, H, W), np.uint8)), mem.upload(np.zeros((S, H, W), np.uint8))
    fl = np.full(S, OO.STEP, dtype=np.uint8)

    def call(fa=mem.ptr(a), fb=mem.ptr(b), H_=H, W_=W, S_=S, h_=h, flags=fl, i=sin, o=sout):
        f = np.ascontiguousarray(flags, dtype=np.uint8) if flags is not None else None
        return lib.rb_obs_stack_step(fa, fb, H_, W_, S_, h_, f.ctypes.data if f is not None else None, i, o, mem.stream)

    def refused(words, **kw):
        assert call(**kw) == -1, kw
        err = lib.rb_last_error()
        assert b"rb_obs_stack_step" in err, err
        for wd in words:
            assert wd in err, (wd, err)

    refused([b"stacks_in_dev", b"NULL"], i=None)
    refused([b"stacks_out_dev", b"NULL"], o=None)
    refused([b"flags_host", b"NULL"], flags=None)
    refused([b"stacks_in_dev", b"aligned"], i=sin + 4)
    refused([b"stacks_out_dev", b"aligned"], o=sout + 8)
    refused([b"stacks_out_dev", b"overlaps"], o=sin)
    refused([b"stacks_out_dev", b"overlaps"], o=sin + 4 * 84 * 84)                # one frame further: still inside the input
    refused([b"stacks_out_dev", b"overlaps"], i=sin + 4 * 84 * 84, o=sin)
    for bad in (0, -1, 65):
        refused([b"streams"], S_=bad)
    for bad in (0, -3, 17):
        refused([b"history"], h_=bad)
    for bad in (1, 0, 4097):
        refused([b"height"], H_=bad)
        refused([b"width"], W_=bad)
    refused([b"flags_host[1]", b"above 7"], flags=[OO.STEP, 8])
    refused([b"flags_host[0]", b"above 7"], flags=[255, OO.STEP])
    refused([b"frames_a_dev", b"NULL"], fa=None)
    refused([b"frames_b_dev", b"NULL"], fb=None)
    refused([b"frames_a_dev", b"NULL"], fa=None, flags=[0, OO.RESET])
    refused([b"frames_b_dev", b"NULL"], fb=None, flags=[OO.FRAME_B, 0])
    mem.sync()
    assert (mem.download(big) == np.float32(0.25)).all()                           # nothing ran
    assert call() == 0                                                             # and the good call goes through
    mem.sync()


def check_guarded(lib, gmem):
    """The S = 3, history = 4 scenario with every caller-owned buffer between canaries: no band was written into."""
    check_scripted(lib, gmem, 3, 4, seed=3)
    count, bad = gmem.check()
    assert count > 2 * ROUNDS and bad == [], bad
