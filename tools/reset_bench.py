"""What a shrink-and-perturb reset costs (a measurement, not a test): Agent.reset_parameters() at the headline config and the
data-efficient config against the two ways a caller had to compose it before, timed as tools/loop_bench.py times its pieces
(device drained, perf_counter around N calls, device drained).  Encoder alpha 0.5, head alpha 0, target included, moments cleared.

  lib     agent.reset_parameters(): rb_learner_shrink_perturb, one launch over the four flat arrays
  torch   the same operation from torch device ops, behind flush(): per named tensor a torch.rand-based phi, lerp_ (or copy_ where
          alpha = 0) into the online and the target view, zero_ of both moment views
  host    agent.init_parameters_flat on the host (torch's CPU generator) + upload, then one lerp per network with a per-element
          alpha vector (built once, outside the timed region) and zero_ of the moments

  python tools/reset_bench.py                  both configs, one JSON line per variant, then the table
"""
import argparse
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("pong-canonical-b32", "data-efficient-b32")
AE, AH = 0.5, 0.0


def one(config, calls, warmup, repeats):
    import numpy as np
    import torch
    import bench
    import __graft_entry__
    __graft_entry__.build()
    from rainbow_amd.agent import Agent, init_parameters_flat
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[config])
    args = bench.make_args(cfg, dev)
    env = types.SimpleNamespace(action_space=lambda: cfg["actions"])
    np.random.seed(123)
    torch.manual_seed(123)
    agent = Agent(args, env)
    std = float(getattr(args, "noisy_std", 0.1))
    st = agent.optimiser.state[agent._params]
    n = agent._params.numel()
    p, t, m, v = agent._params.detach(), agent._target_params, st["exp_avg"], st["exp_avg_sq"]
    shapes = {name: shape for name, _o, shape in agent._layout}
    rules = []                                   # (slice, alpha, bound or None, constant or None)
    fan_in = None
    for name, off, shape in agent._layout:
        numel = int(np.prod(shape))
        sl = slice(off, off + numel)
        if name.startswith("convs"):
            if name.endswith("weight"):
                fan_in = int(np.prod(shape[1:]))
            rules.append((sl, AE, 1.0 / math.sqrt(fan_in), None))
        else:
            out_f, in_f = shapes[name.split(".")[0] + ".weight_mu"]
            kind = name.split(".")[1]
            if kind in ("weight_mu", "bias_mu"):
                rules.append((sl, AH, 1.0 / math.sqrt(in_f), None))
            else:
                rules.append((sl, AH, None, std / math.sqrt(in_f if kind == "weight_sigma" else out_f)))
    alpha_vec = torch.ones(n, device=dev)
    for sl, a, _b, _c in rules:
        alpha_vec[sl] = a
    touched = alpha_vec < 1
    # what the library's launch moves: 4 stores per touched element (online, target, two moments), 2 loads where alpha > 0
    lib_bytes = 4 * (4 * int(touched.sum()) + 2 * int((touched & (alpha_vec > 0)).sum()))

    def lib():
        agent.reset_parameters(AE, AH)

    def composed():
        agent.flush()
        for sl, a, bound, const in rules:
            k = sl.stop - sl.start
            phi = (torch.rand(k, device=dev) * 2 - 1) * bound if const is None else torch.full((k,), const, device=dev)
            for x in (p, t):
                if a == 0:
                    x[sl].copy_(phi)
                else:
                    x[sl].lerp_(phi, 1 - a)
            m[sl].zero_()
            v[sl].zero_()

    def host():
        agent.flush()
        phi = init_parameters_flat(agent._layout, n, std).to(dev)
        for x in (p, t):
            x.copy_(torch.lerp(phi, x, alpha_vec))
        m.masked_fill_(touched, 0.0)
        v.masked_fill_(touched, 0.0)

    def timed(fn, k):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / k * 1e6

    rows = []
    for tag, fn, k in (("lib", lib, calls), ("torch", composed, max(1, calls // 10)), ("host", host, max(1, calls // 100))):
        with torch.no_grad():
            for _ in range(max(1, warmup * k // calls)):
                fn()
            us = sorted(timed(fn, k) for _ in range(repeats))
        row = dict(variant=tag, config=config, params=n, bytes_moved=lib_bytes if tag == "lib" else None,
                   calls=k, repeats=repeats, us_per_call_min=round(us[0], 2), us_per_call_median=round(us[len(us) // 2], 2),
                   us_per_call_max=round(us[-1], 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    rows = []
    for config in ([a.config] if a.config else CONFIGS):
        rows += one(config, a.calls, a.warmup, a.repeats)
    print("\n%-20s %-6s %12s %12s %12s   %s" % ("config", "how", "min us", "median us", "max us", "GB/s (lib: 4 stores per touched element + 2 loads where alpha > 0)"))
    for r in rows:
        gbs = "%.0f" % (r["bytes_moved"] / r["us_per_call_median"] / 1e3) if r["bytes_moved"] else ""
        print("%-20s %-6s %12.2f %12.2f %12.2f   %s" % (r["config"], r["variant"], r["us_per_call_min"], r["us_per_call_median"],
                                                        r["us_per_call_max"], gbs))


if __name__ == "__main__":
    main()
