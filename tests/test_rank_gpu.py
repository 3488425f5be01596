"""Feature rank and per-tensor norms on the MI355X: the bodies of tests/rank_scenarios.py on the real library (its docstring has
the tolerances; the host interpreter runs the same bodies in tests/test_rank_emu.py), and Agent.feature_rank / Agent.tensor_norms
(rainbow_amd/agent_rank.py) on the fixture of tests/test_param_reset_gpu.py (data-efficient, hidden 64, batch 16, replay 2048)."""
import numpy as np
import pytest

import rank_scenarios as K
import redo_scenarios as RS

pytestmark = pytest.mark.gpu

ROWS = sorted(RS.ROWS)


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.fixture
def Mem():
    from cabi_adapter import TorchMem
    return TorchMem


# ----------------------------------------------------------------------------------------------------- kernel level --
@pytest.mark.parametrize("shape", K.GRAM_SHAPES, ids=lambda s: "n%d-d%d-ld%d" % s)
def test_gram_is_inside_the_bound_of_the_exact_sum(hip, Mem, shape):
    K.gram_check(hip, Mem, shape)


def test_gram_bits(hip, Mem):
    K.gram_bits_check(hip, Mem)


def test_gram_refusals(hip, Mem):
    K.gram_refusals_check(hip, Mem)


@pytest.mark.parametrize("n,d", K.SPECTRUM_SHAPES)
def test_planted_ranks_through_the_device_gram(hip, Mem, n, d):
    K.end_to_end_check(hip, Mem, n, d)


@pytest.mark.parametrize("row", ROWS)
def test_captured_rows_equal_debug_read(hip, Mem, row):
    K.capture_check(hip, Mem, row)


def test_measuring_has_no_side_effects(hip, Mem):
    K.no_side_effects_check(hip, Mem())


def test_capture_refuses_while_gradients_wait_for_the_exchange(hip, Mem):
    K.refusal_check(hip, Mem())


@pytest.mark.parametrize("row", ROWS)
def test_tensor_norms_equal_the_reference(hip, Mem, row):
    K.norms_check(hip, Mem, row)


@pytest.mark.parametrize("row", ROWS)
def test_tensor_sums_add_up_to_the_learners_gradient_norm(hip, Mem, row):
    K.grad_norm_check(hip, Mem(), row)


# ------------------------------------------------------------------------------------------------------ Agent level --
def _fresh():
    from test_param_reset_gpu import fresh
    return fresh()


def _steps(agent, mem, ks):
    from test_param_reset_gpu import steps
    return steps(agent, mem, ks)


def test_agent_feature_rank_and_its_repeat():
    from test_redo_agent_gpu import _tensors
    a, ma = _fresh()
    b, mb = _fresh()                            # a twin: the same replay, the same draw state
    _steps(a, ma, range(2))
    _steps(b, mb, range(2))
    assert a.last_feature_rank is None
    before = _tensors(a, ma)
    for layer, dim in (("hidden", 128), ("conv", 576)):
        ra, rb = a.feature_rank(ma, batches=8, layer=layer), b.feature_rank(mb, batches=8, layer=layer)
        assert ra["samples"] == 8 * 16 == 128 and ra["dim"] == dim == a.feature_dim(layer) and ra["layer"] == layer and ra["finite"]
        assert a.last_feature_rank is ra
        sv = ra["singular_values"]
        assert sv.shape == (min(128, dim),) and sv.dtype == np.float64 and np.all(np.diff(sv) <= 0) and sv[0] > 0
        assert 1 <= ra["srank"] <= sv.size and 0 <= ra["feature_rank"] <= sv.size and 1.0 <= ra["effective_rank"] <= sv.size
        assert ra["mean_sq_norm"] > 0 and 0 < ra["top_share"] <= 1
        assert np.array_equal(sv.view(np.uint64), rb["singular_values"].view(np.uint64)), "a repeat on the same draw state must be bit-equal"
        assert all(ra[k] == rb[k] for k in ("srank", "feature_rank", "effective_rank", "mean_sq_norm", "top_share"))
    after = _tensors(a, ma)
    for k in before:
        if k != "tree":                         # (nothing updates priorities; the draws advance ma's own draw state only)
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), "feature_rank changed %s" % k
    assert np.array_equal(before["tree"].view(np.uint8), after["tree"].view(np.uint8)), "feature_rank must not update priorities"
    # measured while a pass is pending, the run goes on as its twin's
    _steps(a, ma, [2])
    _steps(b, mb, [2])
    a.feature_rank(ma, batches=1)
    b.feature_rank(mb, batches=1)
    assert np.array_equal(_steps(a, ma, [3]), _steps(b, mb, [3]))


def test_agent_feature_rank_refusals():
    a, ma = _fresh()
    with pytest.raises(ValueError, match="4096"):
        a.feature_rank(ma, batches=257)         # 257 * 16 = 4112 samples
    with pytest.raises(ValueError, match="batches"):
        a.feature_rank(ma, batches=0)
    with pytest.raises(ValueError, match="layer"):
        a.feature_rank(ma, layer="logits")
    assert a.last_feature_rank is None


def test_agent_tensor_norms():
    import torch
    a, ma = _fresh()
    _steps(a, ma, range(2))
    t = a.tensor_norms()
    names = [n for n, _o, _s in a._layout]
    assert t["names"] == names and len(names) == 20
    for k in ("param_norm", "param_absmax", "target_dist", "grad_norm"):
        assert t[k].shape == (20,) and t[k].dtype == np.float64 and np.isfinite(t[k]).all(), k
    assert float(t["grad_norm"].sum()) > 0 and float(t["target_dist"].sum()) > 0
    a.flush()
    torch.cuda.synchronize()
    for i, name in enumerate(names):
        p, q, g = (a._view(x, name).double() for x in (a._params, a._target_params, a._grads))
        want = (float(p.norm()), float(p.abs().max()), float((p - q).norm()), float(g.norm()))
        got = (t["param_norm"][i], t["param_absmax"][i], t["target_dist"][i], t["grad_norm"][i])
        # two float64 sums of p.numel() terms in two different orders: (numel + 2) 2^-53 each on the sum, halved by the root
        np.testing.assert_allclose(got, want, rtol=(p.numel() + 2) * 2.0 ** -53, atol=0, err_msg=name)
    only = a.tensor_norms(grads=False, target=False)
    assert only["grad_norm"] is None and only["target_dist"] is None
    assert np.array_equal(only["param_norm"].view(np.uint64), t["param_norm"].view(np.uint64))
