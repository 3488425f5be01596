"""What the dormant-unit diagnostic and the targeted reset cost (a measurement, not a test), at the headline config and the
data-efficient config, timed as tools/reset_bench.py times its pieces (device drained, perf_counter around N calls, device drained).

  stats     agent.dormant_stats(mem), one batch: draw + gather, eval-mode forward, k_unit_activity, k_dormant_mask, one synchronise
  recycle   agent.recycle_dormant(mem), one batch: the same launches and k_recycle_units behind the device's own mask, no synchronise
  lib-P     rb_learner_recycle_units alone on a PLANTED mask with P % of every layer's units dormant (0, about 10, 100); online
            parameters and both moments (target=False, the paper's rule)
  torch-P   the same recycle composed from torch device ops on the named tensors' views: uniform draws into the incoming rows,
            index_fill of the outgoing slices, the moments' views zeroed (zero wins: outgoing after incoming)

  python tools/redo_bench.py [--out profiles/redo_bench.txt]     both configs; one JSON line per variant, then the table, to the file
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("pong-canonical-b32", "data-efficient-b32")
SHARES = (0, 10, 100)


def one(config, calls, warmup, repeats, emit):
    import numpy as np
    import torch
    import bench
    import __graft_entry__
    __graft_entry__.build()
    from rainbow_amd import _lib as L
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[config])
    args = bench.make_args(cfg, dev)
    env = types.SimpleNamespace(action_space=lambda: cfg["actions"])
    np.random.seed(123)
    torch.manual_seed(123)
    agent = Agent(args, env)
    mem = ReplayMemory(args, 8192, seed=5)
    g, rs = torch.Generator(device=dev).manual_seed(3), np.random.RandomState(3)
    for _ in range(3):
        mem.append_batch(torch.randint(0, 256, (4096, 84, 84), dtype=torch.uint8, device=dev, generator=g), rs.randint(0, cfg["actions"], 4096),
                         rs.choice([-1.0, 0.0, 1.0], size=4096), rs.random_sample(4096) < 0.001)
    lib, std = agent._lib, agent._noisy_std
    st = agent.optimiser.state[agent._params]
    flat = dict(p=agent._params.detach(), m=st["exp_avg"], v=st["exp_avg_sq"])
    names, units = agent.unit_layers()
    nconv = len(units) - 2
    first = np.concatenate([[0], np.cumsum(units)])
    shapes = {name: shape for name, _o, shape in agent._layout}
    view = {k: {name: agent._view(x, name) for name in shapes} for k, x in flat.items()}

    def planted(share):
        mask = np.zeros(int(first[-1]), np.uint8)
        for k, n in enumerate(units):
            mask[first[k]:first[k] + (n * share + 99) // 100] = 1
        return mask

    def written_elements(mask):
        n = 0
        for k in range(len(units)):
            d = int(mask[first[k]:first[k + 1]].sum())
            if k < nconv:
                w = shapes["convs.%d.weight" % (2 * k)]
                n += d * (int(np.prod(w[1:])) + 1)
                if k + 1 < nconv:
                    nw = shapes["convs.%d.weight" % (2 * k + 2)]
                    n += d * nw[0] * nw[2] * nw[3]
                else:
                    H, F = shapes["fc_h_v.weight_mu"]
                    n += d * 2 * (2 * H) * (F // w[0])
            else:
                z = "fc_z_v" if k == nconv else "fc_z_a"
                n += d * (2 * shapes["fc_h_v.weight_mu"][1] + 2 + 2 * shapes[z + ".weight_mu"][0])
        return n                                             # (elements two dormant units share are counted twice: both store them)

    def torch_recycle(idx):
        def put(name, sel, value):                           # value: None = a uniform draw at the tensor's bound
            tgt = view["p"][name][sel]
            if value is None:
                fan = int(np.prod(shapes[name.replace("bias", "weight")][1:])) if name.startswith("convs") else shapes[name.split(".")[0] + ".weight_mu"][1]
                tgt = (torch.rand(tgt.shape, device=dev) * 2 - 1) / math.sqrt(fan)
            view["p"][name][sel] = tgt if value is None else value
            view["m"][name][sel] = 0.0
            view["v"][name][sel] = 0.0
        H, F = shapes["fc_h_v.weight_mu"]
        for k in range(len(units)):                          # incoming
            i = idx[k]
            if i.numel() == 0:
                continue
            if k < nconv:
                put("convs.%d.weight" % (2 * k), i, None)
                put("convs.%d.bias" % (2 * k), i, None)
            else:
                s = "fc_h_v" if k == nconv else "fc_h_a"
                put(s + ".weight_mu", i, None)
                put(s + ".bias_mu", i, None)
                put(s + ".weight_sigma", i, std / math.sqrt(F))
                put(s + ".bias_sigma", i, std / math.sqrt(H))
        for k in range(len(units)):                          # outgoing afterwards: zero wins
            i = idx[k]
            if i.numel() == 0:
                continue
            if k < nconv - 1:
                put("convs.%d.weight" % (2 * k + 2), (slice(None), i), 0.0)
            elif k == nconv - 1:
                P = F // units[k]
                cols = (i[:, None] * P + torch.arange(P, device=dev)[None, :]).reshape(-1)
                for s in ("fc_h_v", "fc_h_a"):
                    put(s + ".weight_mu", (slice(None), cols), 0.0)
                    put(s + ".weight_sigma", (slice(None), cols), std / math.sqrt(F))
            else:
                z = "fc_z_v" if k == nconv else "fc_z_a"
                put(z + ".weight_mu", (slice(None), i), 0.0)
                put(z + ".weight_sigma", (slice(None), i), std / math.sqrt(H))

    def timed(fn, k):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / k * 1e6

    variants = [("stats", lambda: agent.dormant_stats(mem), calls, None), ("recycle", lambda: agent.recycle_dormant(mem), calls, None)]
    keep = []
    for share in SHARES:
        mask = planted(share)
        mbuf = torch.from_numpy(mask).to(dev)
        idx = [torch.from_numpy(np.flatnonzero(mask[first[k]:first[k + 1]])).to(dev) for k in range(len(units))]
        keep.append((mbuf, idx))
        stream = agent._stream()

        def lib_call(mbuf=mbuf):
            L.check(lib, lib.rb_learner_recycle_units(agent._h, mbuf.data_ptr(), std, 1, 2, 0, flat["m"].data_ptr(), flat["v"].data_ptr(), stream))

        variants.append(("lib-%d" % share, lib_call, calls, mask))
        variants.append(("torch-%d" % share, lambda idx=idx: torch_recycle(idx), max(1, calls // 10), mask))
    rows = []
    agent.flush()
    for tag, fn, k, mask in variants:
        with torch.no_grad():
            for _ in range(max(1, warmup * k // calls)):
                fn()
            us = sorted(timed(fn, k) for _ in range(repeats))
        row = dict(variant=tag, config=config, params=int(agent._params.numel()), units=int(first[-1]),
                   dormant=int(mask.sum()) if mask is not None else None,
                   bytes_stored=12 * written_elements(mask) if mask is not None else None, calls=k, repeats=repeats,
                   us_per_call_min=round(us[0], 2), us_per_call_median=round(us[len(us) // 2], 2), us_per_call_max=round(us[-1], 2))
        if tag == "recycle":
            row["dormant_fraction_found"] = agent.dormant_fraction()
        emit(json.dumps(row))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redo_bench.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit("tools/redo_bench.py --calls %d --warmup %d --repeats %d: us per call, device drained before and after every timed run" % (a.calls, a.warmup, a.repeats))
    rows = []
    for config in ([a.config] if a.config else CONFIGS):
        rows += one(config, a.calls, a.warmup, a.repeats, emit)
    emit("\n%-20s %-10s %8s %12s %12s %12s   %s" % ("config", "how", "dormant", "min us", "median us", "max us", "GB/s stored (lib: online + both moments)"))
    for r in rows:
        gbs = "%.0f" % (r["bytes_stored"] / r["us_per_call_median"] / 1e3) if r["bytes_stored"] and r["variant"].startswith("lib") else ""
        emit("%-20s %-10s %8s %12.2f %12.2f %12.2f   %s" % (r["config"], r["variant"], "" if r["dormant"] is None else r["dormant"],
                                                          r["us_per_call_min"], r["us_per_call_median"], r["us_per_call_max"], gbs))
    out.close()


if __name__ == "__main__":
    main()
