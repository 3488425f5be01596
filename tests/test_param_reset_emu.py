"""Shrink-and-perturb resets on the host interpreter (tests/reset_scenarios.py has the nets and the checks, tests/reset_oracle.py the
rule), the oracle's own Philox, the reference's initial draw inside the same statistical bands, the order against a pending
optimiser pass, and the loops' replay ratio and reset cadence against hand-made traces."""

import numpy as np
import pytest

import catch_oracle
import optimizer_scenarios as S
import reset_oracle as RO
import reset_scenarios as R
from cabi_adapter import NumpyMem
from hipemu import loader
from rainbow_amd import _lib as L
from rainbow_amd import loop

NETS = sorted(R.NETS)


@pytest.fixture(scope="module")
def emu():
    return loader.load()


# ----------------------------------------------------------------------------------------------------------- oracle --
def test_oracle_philox_equals_the_scalar_one():
    seeds = (0, 7, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0)
    los = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 63 + 9, 2 ** 64 - 1], dtype=np.uint64)
    for seed in seeds:
        for hi in (0, 5, 2 ** 32 + 1, 2 ** 64 - 1):
            got = RO.philox4x32_10(seed, hi, los)
            for row, lo in zip(got, los):
                assert tuple(int(x) for x in row) == tuple(int(x) for x in catch_oracle.philox4x32_10(seed, hi, int(lo))), (seed, hi, int(lo))


def test_oracle_uniform_is_symmetric_and_inside_the_unit_interval():
    r = RO.symmetric_uniform(3, 4, 1 << 16)
    assert r.dtype == np.float32 and float(r.min()) >= -1.0 and float(r.max()) < 1.0
    R.in_bands(r, 1.0, "oracle")


# ----------------------------------------------------------------------------------------------------- kernel level --
@pytest.mark.parametrize("net", NETS)
def test_result_equals_the_oracle_bit_for_bit(emu, net):
    R.oracle_check(emu, NumpyMem, net)


@pytest.mark.parametrize("net", NETS)
def test_full_reset_does_not_read_non_finite_parameters(emu, net):
    R.bad_inputs_check(emu, NumpyMem, net)


@pytest.mark.parametrize("net", NETS)
def test_target_and_moments_can_be_left_out(emu, net):
    R.target_off_check(emu, NumpyMem, net)


@pytest.mark.parametrize("net", NETS)
def test_draw_is_keyed_by_seed_and_draw_only(emu, net):
    R.keys_check(emu, NumpyMem, net)


@pytest.mark.parametrize("net", NETS)
def test_largest_tensor_is_uniform_inside_its_bound(emu, net):
    R.distribution_check(emu, NumpyMem, net)


@pytest.mark.parametrize("net", NETS)
def test_reference_initial_draw_sits_inside_the_same_bands(emu, net):
    """rainbow_amd.agent.init_parameters_flat (torch's CPU generator) on the same tensor, and its constants against the oracle's."""
    import torch
    from rainbow_amd.agent import init_parameters_flat
    rig = R.Rig(emu, NumpyMem, net)
    triples = [(name, off, shape) for name, (off, shape) in sorted(rig.layout.items(), key=lambda kv: kv[1][0])]
    torch.manual_seed(11)
    flat = init_parameters_flat(triples, rig.n, R.STD).numpy()
    rules = RO.tensor_rules(rig.layout, R.STD)
    name, off, numel = R.largest_uniform_tensor(rig.layout)
    R.in_bands(flat[off:off + numel], rules[name][3], (net, name, "reference"))
    for tname, (toff, tnumel, uniform, val, _enc) in rules.items():
        if uniform:
            assert float(np.max(np.abs(flat[toff:toff + tnumel]))) <= float(val), tname
        else:       # (the C ABI carries noisy_std as a float32: the constant may differ from the double's by an ulp)
            assert np.all(np.abs(flat[toff:toff + tnumel] - val) <= 2.0 ** -23 * float(val)), tname
    rig.close()


def test_alpha_outside_the_unit_interval_is_refused_by_name(emu):
    R.invalid_args_check(emu, NumpyMem)


def test_a_pending_pass_runs_before_the_reset(emu):
    """Rig A: a deferred clip + Adam pass is pending when the reset is called.  Rig B: the same pass, rb_learner_flush, then the
    reset.  Bit-identical; the alpha = 0 tensors hold the oracle's phi exactly (phi plus an Adam step had the pass run late) and
    the pass did run (the encoder, alpha = 0.5, is the shrunk UPDATED one); nothing is left pending."""
    lib = emu
    res = {}
    for tag in ("pending", "flushed"):
        rig = S.build_rig(lib, NumpyMem, "dataeff", False, L.LEARNER_DEFER_UPDATE)
        m, ad = rig.mem, rig.ad
        g = S.make_grad(ad.layout, ad.n_params, 5, "scales")
        S._store(ad.grads, g)
        L.check(lib, lib.rb_learner_grads_modified(ad.h))
        S._store(rig.ctr, np.array([3], np.int64))
        before = S.state(rig)
        S._clip_adam(rig, lib.rb_learner_clip_adam_deferred, 10.0, 0, m.ptr(rig.norm))
        S.same_state(before, S.state(rig), "the pass is pending")
        if tag == "flushed":
            L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
            stepped = S.state(rig)
            assert not np.array_equal(stepped["p"], before["p"])
        L.check(lib, lib.rb_learner_shrink_perturb(ad.h, 0.5, 0.0, R.STD, 9, 1, 1, m.ptr(ad.adam_m), m.ptr(ad.adam_v), m.stream))
        after = S.state(rig)
        after["t"] = S._dl(m, ad.p_tg)
        L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
        S.same_state(after, S.state(rig), (tag, "nothing may be left pending"))
        res[tag] = after
        if tag == "flushed":
            st = dict(p=stepped["p"], t=np.zeros_like(stepped["p"]), m=stepped["m"], v=stepped["v"])
            want, touched = RO.shrink_perturb(ad.layout, st, 0.5, 0.0, R.STD, 9, 1)
            for k in "pmv":
                assert np.array_equal(R._bits(after[k]), R._bits(want[k])), k
            head = np.zeros(ad.n_params, bool)
            for name, (off, numel, _u, _v, enc) in RO.tensor_rules(ad.layout, R.STD).items():
                head[off:off + numel] = not enc
            phi, _ = RO.phi_flat(ad.layout, ad.n_params, R.STD, 9, 1)
            assert np.array_equal(R._bits(after["p"][head]), R._bits(phi[head]))
            assert np.array_equal(R._bits(after["t"][head]), R._bits(phi[head]))
        S.close_rig(rig)
    for k in ("p", "m", "v", "g", "t"):
        assert np.array_equal(R._bits(res["pending"][k]), R._bits(res["flushed"][k])), k


# --------------------------------------------------------------------------------------------------- loop cadence --
def _run_loop(which, monkeypatch, **fields):
    import test_loop_cadence as LC

    class Agent(LC.FakeAgent):
        target_tau = 0.005

        def reset_parameters(self, *args, **kw):
            self.trace.add("agent.reset_parameters", *args, **kw)

    args = LC._args()
    for k, v in fields.items():
        setattr(args, k, v)
    monkeypatch.setattr(LC, "FakeAgent", Agent)
    monkeypatch.setattr(LC, "_args", lambda: args)
    return LC.run_train(loop, which, 2, False)


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_replay_ratio_and_reset_interval_by_hand(which, monkeypatch):
    """S = 2, T_max = 13, learn_start = 5: rounds start at T = 1, 3, .., 13; the five from T = 5 on learn.  replay_ratio = 1.5 owes
    2 * 1.5 = 3 learn steps per round: 15 in all, in runs of three.  reset_interval = 4: a reset right after learn 4, 8 and 12, i.e.
    after the 1st learn of round 2, the 2nd of round 3 and the 3rd of round 4.  target_tau > 0: no hard target update."""
    trace = _run_loop(which, monkeypatch, replay_ratio=1.5, reset_interval=4)
    calls = [name for name, _, _ in trace if name in ("agent.learn", "agent.reset_parameters", "mem.append_streams")]
    L_, R_, A_ = "agent.learn", "agent.reset_parameters", "mem.append_streams"
    want = [A_, A_,                                   # T = 1, 3: before learn_start
            A_, L_, L_, L_,                           # T = 5:  learns 1-3
            A_, L_, R_, L_, L_,                       # T = 7:  4 (reset), 5, 6
            A_, L_, L_, R_, L_,                       # T = 9:  7, 8 (reset), 9
            A_, L_, L_, L_, R_,                       # T = 11: 10, 11, 12 (reset)
            A_, L_, L_, L_]                           # T = 13: 13-15
    assert calls == want
    assert [a for name, a, kw in trace if name == R_] == [[], [], []] and all(kw == {} for name, _, kw in trace if name == R_)
    assert not any(name == "agent.update_target_net" for name, _, _ in trace)
    assert trace[-1][0] == "returned" and trace[-1][1] == [15]


@pytest.mark.parametrize("which", ["train_device", "train_host_vec"])
def test_no_reset_without_the_two_fields(which, monkeypatch):
    """The same arguments without replay_ratio / reset_interval: replay_frequency = 4 decides (2 / 4 owed per round from T = 5 on:
    learns in the rounds T = 7 and 11), and reset_parameters is never called; reset_interval = 0 means never as well."""
    for fields in ({}, dict(reset_interval=0), dict(replay_ratio=0)):
        trace = _run_loop(which, monkeypatch, **fields)
        assert not any(name == "agent.reset_parameters" for name, _, _ in trace)
        assert sum(name == "agent.learn" for name, _, _ in trace) == 2 and trace[-1][1] == [2]
