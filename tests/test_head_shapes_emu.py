"""The C51 head and the output layer over the (atoms, actions) table of head_shapes_scenarios.py on the host interpreter, from
the SAME kernel sources as librainbow_hip.so.  The device runs the same bodies in test_head_shapes_gpu.py."""
import pytest

import head_shapes_scenarios as HS
from cabi_adapter import NumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.mark.parametrize("case", sorted(HS.CASES))
def test_head_learn_over_atom_and_action_counts(emu, case):
    HS.check_learn(emu, NumpyMem(), case)


@pytest.mark.parametrize("case", sorted(HS.CASES))
def test_head_act_over_atom_and_action_counts(emu, monkeypatch, case):
    HS.check_act(emu, NumpyMem(), case, monkeypatch)
