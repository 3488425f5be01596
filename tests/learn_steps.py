"""Two consecutive learn steps of one configuration on the CPU oracle, and the judgement of conv ReLU decisions that differ from
the oracle's own: shared by test_learner_batches_gpu.py (the batch axis), shape_range_scenarios.py (the history and hidden axes)
and tools/ladder_seeds.py (their seeds).  test_learner_batches_gpu.py's docstring has the reasoning behind the ReLU treatment."""
import numpy as np
import torch

import scenarios
from oracle import learner_oracle as O

RELU_MARGIN = 3e-8      # test_learner_gpu.RELU_MARGIN: ~10x the f32 rounding noise of a hidden pre-activation


def two_step_inputs(cfgd, seed):
    """The seeded inputs of a configuration: both nets' parameters and, per step, the raw noise draws and the batch."""
    cfg = O.Config(**cfgd)
    draws = O.noise_draw_count(cfg)
    rs = np.random.RandomState(1000 + seed)
    steps = []
    for k in range(2):
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        steps.append(dict(raw_on=raw_on, raw_tg=raw_tg, batch=scenarios.make_batch(cfgd, 7000 + 10 * seed + k)))
    return dict(cfg=cfg, online=O.init_params(cfg, 901 + 2 * seed), target=O.init_params(cfg, 902 + 2 * seed), steps=steps)


class OracleRun:
    """The oracle's two steps, one at a time (a masked case feeds it the device's ReLU decisions of each step)."""

    def __init__(self, inp):
        hy = scenarios.LEARN_HYPER
        self.inp, self.hy, self.online = inp, hy, inp["online"]
        self.adam = O.AdamOracle(inp["online"], hy["lr"], hy["adam_eps"])

    def near_zero(self, k):
        """How many hidden pre-activations of step k's differentiated forward lie inside RELU_MARGIN (oracle forward only)."""
        st, probe = self.inp["steps"][k], {}
        x = torch.from_numpy(st["batch"]["states"]).to(torch.float32).div(255)
        with torch.no_grad():
            O.forward(self.inp["cfg"], {n: torch.from_numpy(v) for n, v in self.online.items()},
                      O.make_noise(self.inp["cfg"], st["raw_on"]), x, log=True, probe=probe)
        return int((np.abs(probe["hidden_pre"]) < RELU_MARGIN).sum())

    def step(self, k, hidden_mask=None, conv_masks=None):
        cfg, st = self.inp["cfg"], self.inp["steps"][k]
        params = self.online                     # (the parameters this step's forward ran on: conv_flips judges against them)
        want = O.learn(cfg, self.online, self.inp["target"], O.make_noise(cfg, st["raw_on"]), O.make_noise(cfg, st["raw_tg"]),
                       st["batch"], hidden_mask=hidden_mask, conv_masks=conv_masks)
        if conv_masks is not None:
            want["conv_flips"] = conv_flips(cfg, params, want.pop("conv_pre"), want.pop("conv_in"), conv_masks)
        total, clipped = O.clip_grads(want["grads"], self.hy["norm_clip"])
        self.online = self.adam.step(clipped)
        exact = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in want["grads"].values()))
        return dict(want=want, total=total, clipped=clipped, exact=exact, params={n: v.copy() for n, v in self.online.items()})


def conv_flips(cfg, params, conv_pre, conv_in, conv_masks):
    """Per conv layer: (decisions that differ from the oracle's own, the largest |pre-activation| among them, the largest ratio of
    such a |pre-activation| to the rounding bound of its element — 2 (K + 1) 2^-24 (sum_k |w_k x_k| + |b|), Higham eq. 3.5, once
    for each of the two dot products that decided it; a ratio of 1 or more fails the case)."""
    out = []
    for i, (_c, ks, stride) in enumerate(cfg.convs[0]):
        pre, mask = conv_pre[i], np.asarray(conv_masks[i], dtype=bool)
        diff = (pre > 0) != mask
        if not diff.any():
            out.append((0, 0.0, 0.0))
            continue
        w, b = params["convs.%d.weight" % (2 * i)], params["convs.%d.bias" % (2 * i)]
        mag = torch.nn.functional.conv2d(torch.from_numpy(np.abs(conv_in[i])).double(), torch.from_numpy(np.abs(w)).double(),
                                         torch.from_numpy(np.abs(b)).double(), stride=stride).numpy()
        bound = 2.0 * (w[0].size + 1) * 2.0 ** -24 * mag
        out.append((int(diff.sum()), float(np.abs(pre[diff]).max()), float((np.abs(pre[diff]) / bound[diff]).max())))
    return out


def conv_shapes(cfg, B):
    """[B, cout, oh, ow] of each conv layer's output."""
    shapes, ih = [], 84
    for cout, ks, stride in cfg.convs[0]:
        ih = (ih - ks) // stride + 1
        shapes.append((B, cout, ih, ih))
    return shapes
