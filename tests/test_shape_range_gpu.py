"""The learn step and the act path over the history / hidden table of shape_range_scenarios.py on the MI355X: the split-K first
conv layer at a partly filled reduction, the generic convs and the act path's scalar units up to K = RB_ACT_KMAX, 1 / 2 / 3 / 4
row splits of the hidden layer's input gradient, both sides of the fast_fc limit and of the fused norm's slot limit, the accepted
maximum, and the tiled forward GEMM beyond its split-K tile cap — two learn steps and about a dozen act calls per row against
the oracle."""
import pytest

import shape_range_scenarios as SR
from cabi_adapter import TorchMem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case,flagset", SR.LEARN_RUNS, ids=["%s-%s" % r for r in SR.LEARN_RUNS])
def test_learn_steps_over_history_and_hidden_sizes_on_device(hip, case, flagset):
    SR.check_learn(hip, TorchMem(), case, flagset)


@pytest.mark.parametrize("case", list(SR.CASES))
def test_act_paths_over_history_and_hidden_sizes_on_device(hip, monkeypatch, case):
    SR.check_act(hip, TorchMem(), case, monkeypatch)
