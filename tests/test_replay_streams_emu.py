"""S interleaved environment streams in one replay (rb_replay_create_streams / rb_replay_append_streams) on the host
interpreter: the SAME kernel sources as librainbow_hip.so against tests/streams_oracle.py.  The device runs the same checks
in test_replay_streams_gpu.py."""
import pytest

import streams_scenarios as SS
from cabi_adapter import NumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


def test_one_stream_is_todays_replay(emu):
    SS.check_s1_identity(emu, NumpyMem())


@pytest.mark.parametrize("S", [2, 7, 16, 64])
def test_append_rounds_equal_sequential_appends(emu, S):
    SS.check_append_rounds(emu, NumpyMem(), S, seed=100 + S)


@pytest.mark.parametrize("n", [3, 20])
@pytest.mark.parametrize("S", [2, 16, 64])
def test_sampling_matches_the_restatement_and_each_stream(emu, S, n):
    SS.check_sampling(emu, NumpyMem(), S, n, seed=10 * S + n)


def test_draw_rejected_near_the_write_head(emu):
    SS.check_reject_near_head(emu, NumpyMem())


@pytest.mark.parametrize("S", [3, 8])
def test_validation_states_follow_the_stream(emu, S):
    SS.check_states_at(emu, NumpyMem(), S, seed=S)


def test_create_refuses_bad_stream_layouts(emu):
    SS.check_create_refusals(emu)
