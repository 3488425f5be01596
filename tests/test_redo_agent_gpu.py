"""Agent.dormant_stats / Agent.recycle_dormant on the MI355X (rainbow_amd/agent_redo.py), on the fixture of
tests/test_param_reset_gpu.py (data-efficient, hidden 64, batch 16, replay 2048): the diagnostic changes nothing, a recycle equals
the oracle's result from the device's own mask, a checkpointed run repeats the next recycle bit for bit, two replicas that pass the
same rng draw the same parameters, and a bad tau is refused."""
import io

import numpy as np
import pytest
import torch

import redo_oracle as RD
import reset_scenarios as R
from test_param_reset_gpu import MODES, _mode, fresh, layout_of, moments, same_agents, snapshot, steps

pytestmark = pytest.mark.gpu
TAU = 0.1


def _tensors(agent, mem):
    agent.flush()
    m, v = moments(agent)
    torch.cuda.synchronize()
    out = dict(p=agent._params.detach(), t=agent._target_params, g=agent._grads, m=m, v=v, noise=agent.noise, tnoise=agent.target_noise,
               loss=agent._loss)
    out = {k: x.cpu().numpy().copy() for k, x in out.items()}
    out["tree"] = np.array(mem._grab("tree"), copy=True)
    if agent._step_dev is not None:
        out["step"] = agent._step_dev.cpu().numpy().copy()
    return out


def test_dormant_stats_changes_nothing():
    a, ma = fresh()
    _spare, held_out = fresh()                # the batches come from a memory of their own: `ma` draws what its twin's draws
    steps(a, ma, range(2))
    before = _tensors(a, ma)
    st = a.dormant_stats(held_out, batches=2, tau=TAU)
    after = _tensors(a, ma)
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), "dormant_stats changed %s" % k
    names, units = a.unit_layers()
    assert st["layers"] == names == ["convs.0", "convs.2", "fc_h_v", "fc_h_a"] and st["units"] == units == [32, 64, 64, 64]
    assert len(st["dormant"]) == 4 and all(0 <= d <= u for d, u in zip(st["dormant"], units))
    assert st["fraction"] == sum(st["dormant"]) / 224.0 and st["scores"].shape == (224,) and st["scores"].dtype == np.float32
    # the counts are those of the scores: no unit sits within a relative 1e-6 of the threshold, so the float32 scores decide alike
    sc = st["scores"].astype(np.float64)
    assert np.all(np.abs(sc - TAU) > 1e-6 * TAU), "ill-conditioned draw: a score at the threshold"
    f = np.concatenate([[0], np.cumsum(units)])
    assert st["dormant"] == [int((sc[f[k]:f[k + 1]] <= TAU).sum()) for k in range(4)]
    assert a.recycles == 0 and a.last_recycle_counts is None and a.dormant_fraction() is None
    # asked while a pass is pending, the run goes on as its twin's
    b, mb = fresh()
    steps(b, mb, range(2))
    steps(a, ma, [2])
    a.dormant_stats(held_out)
    steps(b, mb, [2])
    la, lb = steps(a, ma, [3]), steps(b, mb, [3])
    assert np.array_equal(la, lb)
    same_agents(a, b, "after dormant_stats")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_recycle_equals_the_oracle_from_the_device_mask(monkeypatch, mode):
    _mode(monkeypatch, mode)
    a, ma = fresh()
    steps(a, ma, range(2))
    if mode == "hosted":
        assert a._update_pending
    a.flush()
    st = snapshot(a)
    torch.cuda.synchronize()
    a.recycle_dormant(ma, tau=0.5, target=True, rng=(9, 2 ** 32 + 1))
    assert a.recycles == 1 and not a._update_pending
    mask = a._keep["redo_mask"].cpu().numpy()
    counts = a.last_recycle_counts.cpu().numpy()
    f = np.concatenate([[0], np.cumsum(a.unit_layers()[1])])
    assert counts.tolist() == [int(mask[f[k]:f[k + 1]].sum()) for k in range(4)] and 0 < mask.sum() < mask.size
    assert a.dormant_fraction() == float(mask.sum()) / mask.size
    want, kind, _both = RD.recycle(layout_of(a), st, mask, 0.1, 9, 2 ** 32 + 1)
    got = snapshot(a)
    for k in "ptmv":
        assert np.array_equal(R._bits(got[k]), R._bits(want[k])), (mode, k)
    # target=False (the default, the paper's rule) leaves the target alone
    t_before = got["t"]
    a.recycle_dormant(ma, tau=0.5)
    assert np.array_equal(R._bits(snapshot(a)["t"]), R._bits(t_before)) and a.recycles == 2
    losses = steps(a, ma, range(2, 4))
    assert np.isfinite(losses).all()


def test_bad_tau_is_refused():
    a, ma = fresh()
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            a.dormant_stats(ma, tau=bad)
        with pytest.raises(ValueError, match="tau"):
            a.recycle_dormant(ma, tau=bad)
    with pytest.raises(ValueError, match="batches"):
        a.dormant_stats(ma, batches=0)
    assert a.recycles == 0


def test_replicas_with_the_same_rng_draw_the_same_parameters(monkeypatch):
    _mode(monkeypatch, "hosted")
    a, ma = fresh()
    b, mb = fresh()
    steps(a, ma, range(2))
    steps(b, mb, range(2))
    a.recycle_dormant(ma, tau=0.5, target=True, rng=(3, 7))
    b.recycle_dormant(mb, tau=0.5, target=True, rng=(3, 7))
    same_agents(a, b, "replicas")
    c, mc = fresh()
    steps(c, mc, range(2))
    c.recycle_dormant(mc, tau=0.5, target=True, rng=(3, 8))
    assert not np.array_equal(snapshot(c)["p"], snapshot(a)["p"])


def test_checkpoint_restore_repeats_the_next_recycle(monkeypatch, tmp_path):
    from rainbow_amd.memory import ReplayMemory
    _mode(monkeypatch, "hosted")
    a1, m1 = fresh()
    steps(a1, m1, range(2))
    a1.recycle_dormant(m1, tau=0.5)                     # recycle #1: rng = (args.seed or 0, 0)
    assert a1.recycles == 1
    ck = a1.checkpoint(str(tmp_path / "agent.ck"))
    assert ck["recycles"] == 1
    buf = io.BytesIO()
    m1.save_to(buf, chunk_bytes=1 << 20)
    tail1 = steps(a1, m1, [2])
    a1.recycle_dormant(m1, tau=0.5)                     # recycle #2: draw 1
    a2, _unused = fresh()
    a2.restore(str(tmp_path / "agent.ck"))
    assert a2.recycles == 1
    buf.seek(0)
    m2 = ReplayMemory.load_from(buf, torch.device("cuda:0"), chunk_bytes=1 << 20)
    tail2 = steps(a2, m2, [2])
    a2.recycle_dormant(m2, tau=0.5)
    assert a1.recycles == a2.recycles == 2
    assert np.array_equal(tail1, tail2)
    same_agents(a1, a2, "resumed")
    assert np.array_equal(a1.last_recycle_counts.cpu().numpy(), a2.last_recycle_counts.cpu().numpy())
    old = {k: v for k, v in ck.items() if k != "recycles"}
    a2.restore(old)                                     # a checkpoint from before the counter existed
    assert a2.recycles == 0
