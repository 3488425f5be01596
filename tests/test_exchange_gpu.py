"""GPU parity of BASELINE config 5's exchange kernels on ONE device (no RCCL needed): N learner handles stand for N
replicas (own batch, own noise, identical parameters) — N = 2, and N = 8 = config 5's world size (M = 8 x 32 = 256 gathered
rows, scale 1/8, the 8-block rank-order fold of k_finish_grads_tiled); the collectives are replaced by device-side copies — a torch.cat
for the all-gather of the per-rank blocks, an elementwise mean for the flat all-reduce — so that what runs on the GPU is exactly
rb_learner_learn with the exchange armed (k_pack_factors, deferred FC weight gradients), rb_learner_finish_grads
(k_finish_grads_tiled) and, in the 'allreduce' mode, rb_learner_grads_modified -> k_sumsq, followed by the one-pass clip + Adam.
Insert point in the reference: between agent.py:96 (backward) and agent.py:97 (clip_grad_norm_).
Required: both handles bit-identical, and gradients / parameters == the oracle fed with the MEAN gradient."""
import ctypes as C

import numpy as np
import pytest
import torch

import scenarios
from helpers import assert_learn_trace_matches
from oracle import learner_oracle as O
from test_learner_gpu import BASELINE_SHAPES

pytestmark = pytest.mark.gpu

SHAPES = ["cfg2-canonical-h512-b32-a6", "cfg4-dataeff-h256-n20-b32-a6"]


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


class LocalFactoredExchange:
    """What rainbow_amd.dist.FactoredExchange does per rank, for N handles in one process."""

    def __init__(self, lib, ads):
        from rainbow_amd import _lib as L
        self.lib, self.ads, self.L = lib, ads, L
        f, off, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(lib, lib.rb_learner_exchange_layout(ads[0].h, C.byref(f), C.byref(off), C.byref(n)))
        self.f, self.off, self.n = f.value, off.value, n.value
        dev = ads[0].grads.device
        self.local = [torch.zeros(self.f, dtype=torch.float32, device=dev) for _ in ads]
        self.all = [torch.zeros(len(ads) * self.f, dtype=torch.float32, device=dev) for _ in ads]
        for ad, lo, al in zip(ads, self.local, self.all):
            L.check(lib, lib.rb_learner_set_exchange(ad.h, len(ads), lo.data_ptr(), al.data_ptr()))

    def run(self):
        L, lib = self.L, self.lib
        stream = self.ads[0].mem.stream
        gathered = torch.cat(self.local)                       # the all-gather (FC factors, noise AND conv gradients of every rank)
        for ad, al in zip(self.ads, self.all):
            al.copy_(gathered)
            L.check(lib, lib.rb_learner_finish_grads(ad.h, stream))

    def close(self):
        for ad in self.ads:
            self.lib.rb_learner_set_exchange(ad.h, 1, None, None)


@pytest.mark.parametrize("mode", ["factored", "allreduce"])
@pytest.mark.parametrize("shape,world", [(SHAPES[0], 2), (SHAPES[1], 2), (SHAPES[0], 8)],
                         ids=[SHAPES[0] + "-world2", SHAPES[1] + "-world2", SHAPES[0] + "-world8"])
def test_replica_exchange_kernels_match_oracle_on_mean_gradient(hip, monkeypatch, shape, world, mode):
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    from rainbow_amd import _lib as L
    cfgd = BASELINE_SHAPES[shape]
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, shape, cfgd)
    cfg = O.Config(**cfgd)
    hy = scenarios.LEARN_HYPER
    ads = [CAbiLearnAdapter(hip, TorchMem(), shape) for _ in range(world)]
    online, target = O.init_params(cfg, 611), O.init_params(cfg, 612)
    for ad in ads:
        ad.load(online, target)
    exch = LocalFactoredExchange(hip, ads) if mode == "factored" else None
    adam = O.AdamOracle(online, hy["lr"], hy["adam_eps"])
    draws = O.noise_draw_count(cfg)
    got_t, want_t = {}, {}
    # (world 8's sixteen learn calls on the world-2 seeds contain one ill-conditioned batch — rank 6 of step 1: a hidden
    # pre-activation of +2.8e-9 in the f32 oracle, -8.1e-10 in float64 — where relu'(x) and with it 4 % of that unit's
    # gradients depend on the summation order, oracle.learner_oracle.learn; its seeds start at 1000, and the margin is asserted)
    base = 0 if world == 2 else 1000
    for k in range(2):
        per_rank = []
        for r, ad in enumerate(ads):
            rs = np.random.RandomState(base + 100 + 10 * k + r)          # per-replica noise and data
            raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
            batch = scenarios.make_batch(cfgd, base + 200 + 10 * k + r)
            ad.reset_noise_online(raw_on)
            ad.learn_only(batch, raw_tg)
            per_rank.append(O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch))
            assert per_rank[-1]["hidden_relu_margin"] > 3e-8, "ill-conditioned seed (step %d rank %d)" % (k, r)
        if exch is not None:
            exch.run()
        else:
            mean = ads[0].grads.clone()                                  # the flat all-reduce (mean), rank order
            for ad in ads[1:]:
                mean += ad.grads
            mean /= world
            for ad in ads:
                ad.grads.copy_(mean)
                L.check(hip, hip.rb_learner_grads_modified(ad.h))
        outs = [ad.finish_step() for ad in ads]
        # replicas: identical bits
        for r in range(1, world):
            assert torch.equal(ads[0].grads, ads[r].grads), "step %d: gradients of replica %d differ" % (k, r)
            assert torch.equal(ads[0].p_on.detach(), ads[r].p_on.detach()), "step %d: parameters of replica %d differ" % (k, r)
            assert outs[0]["grad_norm"] == outs[r]["grad_norm"]
        # oracle on the mean gradient
        gmean = {n: sum(pr["grads"][n].astype(np.float64) for pr in per_rank).astype(np.float32) / np.float32(world)
                 for n in per_rank[0]["grads"]}
        total, clipped = O.clip_grads(gmean, hy["norm_clip"])
        online = adam.step(clipped)
        for r in range(world):
            got_t["s%d_r%d_loss" % (k, r)], want_t["s%d_r%d_loss" % (k, r)] = outs[r]["loss"], per_rank[r]["loss"]
        got_t["s%d_grad_norm" % k], want_t["s%d_grad_norm" % k] = np.float32(outs[0]["grad_norm"]), np.float32(total)
        for name in clipped:
            got_t["s%d_grad/%s" % (k, name)], want_t["s%d_grad/%s" % (k, name)] = outs[0]["grads"][name], clipped[name]
        for name, p in ads[0].params().items():
            got_t["s%d_param/%s" % (k, name)], want_t["s%d_param/%s" % (k, name)] = p, online[name]
    assert_learn_trace_matches(got_t, want_t, label="exchange-%s/%s/world%d" % (mode, shape, world))
    if exch is not None:
        exch.close()
    for ad in ads:
        ad.close()


def test_library_rccl_exchange_equals_the_host_gathered_one(hip, monkeypatch):
    """rb_comm_* + rb_learner_exchange_rccl (the library's own ncclAllGather on a communicator it created: librccl through
    dlopen, no torch.distributed) on a ONE-rank communicator — all this box can host — against the same step whose block
    was 'gathered' by a device copy: bit-identical gradients, norm partials and post-Adam parameters.  The lone block stands
    for both replicas of a two-block exchange buffer, as in the RAINBOW_AMD_FORCE_DIST plumbing run."""
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    from rainbow_amd import _lib as L
    shape = "cfg2-canonical-h512-b32-a6"
    cfgd = BASELINE_SHAPES[shape]
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, shape, cfgd)
    cfg = O.Config(**cfgd)
    ident = (C.c_ubyte * 128)()
    L.check(hip, hip.rb_comm_unique_id(ident))
    comm = C.c_void_p()
    L.check(hip, hip.rb_comm_create(C.byref(comm), ident, 1, 0))
    ads = [CAbiLearnAdapter(hip, TorchMem(), shape) for _ in range(2)]
    online, target = O.init_params(cfg, 711), O.init_params(cfg, 712)
    f = C.c_int64(0)
    L.check(hip, hip.rb_learner_exchange_layout(ads[0].h, C.byref(f), None, None))
    bufs = []
    for ad in ads:
        ad.load(online, target)
        local = torch.zeros(f.value, dtype=torch.float32, device=ad.grads.device)
        both = torch.zeros(2 * f.value, dtype=torch.float32, device=ad.grads.device)
        L.check(hip, hip.rb_learner_set_exchange(ad.h, 2, local.data_ptr(), both.data_ptr()))
        bufs.append((local, both))
    draws = O.noise_draw_count(cfg)
    for k in range(2):
        rs = np.random.RandomState(300 + k)
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        batch = scenarios.make_batch(cfgd, 400 + k)
        for ad in ads:
            ad.reset_noise_online(raw_on)
            ad.learn_only(batch, raw_tg)
        local, both = bufs[0]                                      # host-side 'gather': the block, twice
        both[:f.value].copy_(local)
        both[f.value:].copy_(local)
        L.check(hip, hip.rb_learner_finish_grads(ads[0].h, ads[0].mem.stream))
        L.check(hip, hip.rb_learner_exchange_rccl(ads[1].h, comm, ads[1].mem.stream))     # ncclAllGather + copy + finish
        outs = [ad.finish_step() for ad in ads]
        assert torch.equal(bufs[0][1], bufs[1][1]), "step %d: gathered blocks differ" % k
        assert torch.equal(ads[0].grads, ads[1].grads), "step %d: gradients differ" % k
        assert torch.equal(ads[0].p_on.detach(), ads[1].p_on.detach()), "step %d: parameters differ" % k
        assert outs[0]["grad_norm"] == outs[1]["grad_norm"]
    for ad in ads:
        hip.rb_learner_set_exchange(ad.h, 1, None, None)
        ad.close()
    L.check(hip, hip.rb_comm_destroy(comm))
