"""Numpy restatement of the random-shift augmentation of the replay's frame-stack gather (include/rainbow_hip.h,
rb_replay_gather_shifted).  TEST INFRASTRUCTURE: the product path (rainbow_amd/) never imports it.

  out[i][w][c][y][x] = stack[i][w][c][clip(y + dy)][clip(x + dx)],  clip onto [0, 83]  — the un-shifted stack padded by `pad` pixels
  of edge replication and cropped at offset (pad + dy, pad + dx); one (dy, dx) per (sample i, stack w), shared by its frames.
  Device draws: Philox4x32-10, key = seed ^ 0x5348494654, counter (hi = draw, lo = i); words 0, 1 -> the state's (dy, dx), words
  2, 3 -> the next state's; each word v gives ((v * (2 pad + 1)) >> 32) - pad."""
import numpy as np

from catch_oracle import philox4x32_10

KEY_TAG = 0x5348494654
SIDE = 84


def draw_shifts(seed, draw, batch, pad):
    """int8 [batch, 2, 2]: [i][w] -> (dy, dx) of the device's draw number `draw` on a replay created with `seed`."""
    out = np.zeros((batch, 2, 2), dtype=np.int8)
    for i in range(batch):
        v = philox4x32_10((int(seed) ^ KEY_TAG) & 0xFFFFFFFFFFFFFFFF, int(draw), i)
        out[i] = np.array([((int(x) * (2 * pad + 1)) >> 32) - pad for x in v], dtype=np.int8).reshape(2, 2)
    return out


def shift_stacks(stacks, shifts_w):
    """stacks u8 [B, h, 84, 84] (un-shifted), shifts_w int [B, 2] = (dy, dx) per sample -> the shifted stacks.  A blanked (all-zero)
    frame stays all zero under any shift, so blanking needs no special case here."""
    stacks = np.asarray(stacks)
    out = np.empty_like(stacks)
    ar = np.arange(SIDE)
    for i in range(stacks.shape[0]):
        dy, dx = int(shifts_w[i][0]), int(shifts_w[i][1])
        rows, cols = np.clip(ar + dy, 0, SIDE - 1), np.clip(ar + dx, 0, SIDE - 1)
        out[i] = stacks[i][:, rows][:, :, cols]
    return out


def shift_batch(states, next_states, shifts):
    """Both stacks of a batch under shifts int8 [B, 2, 2]."""
    shifts = np.asarray(shifts)
    return shift_stacks(states, shifts[:, 0]), shift_stacks(next_states, shifts[:, 1])
