"""The C51 head and the output layer over the (atoms, actions) table of head_shapes_scenarios.py on the MI355X: k_head<1 / 2 / 4>,
both projection scatters, more softmax tasks than waves, NZ at RB_HEAD_MAX_NZ, and the one-launch act path with more
output-layer units than workgroups — each against the float64 head on the device's own logits and against the oracle."""
import pytest

import head_shapes_scenarios as HS
from cabi_adapter import TorchMem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", sorted(HS.CASES))
def test_head_learn_over_atom_and_action_counts_on_device(hip, case):
    HS.check_learn(hip, TorchMem(), case)


@pytest.mark.parametrize("case", sorted(HS.CASES))
def test_head_act_over_atom_and_action_counts_on_device(hip, monkeypatch, case):
    HS.check_act(hip, TorchMem(), case, monkeypatch)
