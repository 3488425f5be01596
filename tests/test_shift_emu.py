"""Random-shift augmentation in the replay's frame-stack gather (rb_replay_gather_shifted, csrc/replay_shift.h) on the host
interpreter: the SAME kernel source as librainbow_hip.so against tests/shift_oracle.py.  The device runs the same checks in
test_shift_gpu.py."""
import pytest

import shift_scenarios as SH
from cabi_adapter import NumpyMem
from guarded_mem import GuardedNumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.mark.parametrize("pad", [1, 4, 8])
@pytest.mark.parametrize("history,n,streams", [(4, 3, 1), (1, 1, 1), (3, 20, 1), (4, 3, 3)],
                         ids=["h4-n3", "h1-n1", "h3-n20", "h4-n3-3streams"])
def test_every_shift_matches_the_oracle(emu, history, n, streams, pad):
    SH.check_injected_enumeration(emu, NumpyMem(), history, n, pad, streams=streams)


def test_pad_zero_is_the_plain_gather(emu):
    SH.check_pad_zero_is_the_plain_gather(emu, NumpyMem())


@pytest.mark.parametrize("seed", [7, 0x9E3779B97F4A7C15])
def test_device_draws_match_the_oracle_and_leave_the_header_alone(emu, seed):
    SH.check_philox_path(emu, NumpyMem(), seed)


def test_gather_stays_inside_the_callers_buffers(emu):
    SH.check_guard_bands(emu, GuardedNumpyMem())


def test_refusals_name_the_argument_and_launch_nothing(emu):
    SH.check_refusals(emu, NumpyMem())


def test_learn_step_on_shifted_stacks_matches_the_oracle(emu):
    SH.check_learn_step(emu, NumpyMem())
