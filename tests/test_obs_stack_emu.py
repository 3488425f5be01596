"""The S-stream observation front end (rb_obs_stack_step, csrc/obs_stack.h) on the host interpreter, from the SAME kernel
sources as librainbow_hip.so, against env.py's deque restated in tests/obs_stack_oracle.py.  The device runs the same checks
in test_obs_stack_gpu.py."""
import pytest

import obs_stack_scenarios as OS
from cabi_adapter import NumpyMem
from guarded_mem import GuardedNumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


# S: 1 and 64 are the ends of the range, 3 is neither a power of two nor a lane multiple; history 1 has nothing to shift, 4 is
# the shape every agent here uses
@pytest.mark.parametrize("S", [1, 3, 64])
@pytest.mark.parametrize("history", [1, 4])
def test_scripted_rounds_match_the_deque_oracle(emu, S, history):
    OS.check_scripted(emu, NumpyMem(), S, history, seed=3)


def test_scripted_rounds_at_the_longest_history(emu):
    OS.check_scripted(emu, NumpyMem(), 2, 16, seed=4)


def test_scripted_rounds_on_another_screen_geometry(emu):
    OS.check_scripted(emu, NumpyMem(), 3, 4, H=97, W=131, seed=5)


def test_newest_frame_is_frame_preprocess(emu):
    OS.check_newest_frame_equals_frame_preprocess(emu, NumpyMem())


def test_null_frame_pointers(emu):
    OS.check_null_frames(emu, NumpyMem())


def test_refusals(emu):
    OS.check_refusals(emu, NumpyMem())


def test_scripted_rounds_between_guard_bands(emu):
    OS.check_guarded(emu, GuardedNumpyMem())
