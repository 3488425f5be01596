"""The learn step and the act path over the history / hidden table of shape_range_scenarios.py on the host interpreter, from the
SAME kernel sources as librainbow_hip.so: the rows at batch 4 (the batch-33 and batch-1024 rows are the device's,
test_shape_range_gpu.py, which runs the same bodies on every row)."""
import pytest

import shape_range_scenarios as SR
from cabi_adapter import NumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.mark.parametrize("case", SR.EMU_CASES)
def test_learn_steps_over_history_and_hidden_sizes(emu, case):
    SR.check_learn(emu, NumpyMem(), case, where="emu")


@pytest.mark.parametrize("case", SR.EMU_CASES)
def test_act_paths_over_history_and_hidden_sizes(emu, monkeypatch, case):
    SR.check_act(emu, NumpyMem(), case, monkeypatch, where="emu")
