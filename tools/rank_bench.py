"""What the feature-rank and per-tensor-norm read-outs cost (a measurement, not a test), timed as tools/redo_bench.py times its pieces
(device drained, perf_counter around N calls, device drained).

  gram        rb_gram_f64 alone at (n, d) = (256, 1024), (2048, 1024), (2048, 3136), (256, 576) against torch.mm(Phi, Phi.T) of the
              same Phi in float64 (the cast included: the library reads the f32 rows itself) and in float32, alternating in one process;
              the useful work is the upper triangle, n (n + 1) d FLOP, and its share of the f64 matrix peak (78.6 TFLOP/s, the vendor's
              figure for the MI355X) is computed from that
  rank        agent.feature_rank(mem) end to end at 8 and 64 batches, hidden layer, at the headline and the data-efficient config, and
              the host part (feature_rank.spectrum_metrics: eigvalsh of the [n, n] matrix) on its own
  norms       agent.tensor_norms() against the same four norms per tensor composed from torch device ops on the tensors' views

  python tools/rank_bench.py [--out profiles/feature_rank_bench.txt]     one JSON line per variant, to the file
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("pong-canonical-b32", "data-efficient-b32")
GRAM_SHAPES = ((256, 1024), (2048, 1024), (2048, 3136), (256, 576))
F64_MATRIX_PEAK = 78.6e12


def timed(torch, fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def stats(us):
    us = sorted(us)
    return dict(us_min=round(us[0], 2), us_median=round(us[len(us) // 2], 2), us_max=round(us[-1], 2))


def gram(calls, warmup, repeats, emit):
    import torch
    from rainbow_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for n, d in GRAM_SHAPES:
        torch.manual_seed(n + d)
        phi = torch.randn(n, d, device=dev)
        K = torch.empty(n, n, dtype=torch.float64, device=dev)
        variants = {"lib-f64-mfma": lambda: L.check(lib, lib.rb_gram_f64(phi.data_ptr(), n, d, d, K.data_ptr(), stream)),
                    "torch-mm-f64": lambda: torch.mm(phi.double(), phi.double().T),
                    "torch-mm-f32": lambda: torch.mm(phi, phi.T)}
        us = {k: [] for k in variants}
        for fn in variants.values():
            for _ in range(warmup):
                fn()
        for _ in range(repeats):                                  # alternating: every repeat times each variant once
            for k, fn in variants.items():
                us[k].append(timed(torch, fn, calls))
        ref = torch.mm(phi.double(), phi.double().T)
        variants["lib-f64-mfma"]()
        torch.cuda.synchronize()
        for k in variants:
            row = dict(section="gram", variant=k, n=n, d=d, calls=calls, repeats=repeats, **stats(us[k]))
            if k == "lib-f64-mfma":
                row["upper_triangle_tflops"] = round(n * (n + 1) * d / row["us_median"] / 1e6, 2)
                row["share_of_f64_matrix_peak"] = round(n * (n + 1) * d / (row["us_median"] * 1e-6) / F64_MATRIX_PEAK, 4)
                row["max_abs_diff_vs_torch_f64"] = float((K - ref).abs().max())
            emit(json.dumps(row))


def agent_level(config, calls, warmup, repeats, emit):
    import numpy as np
    import torch
    import bench
    from rainbow_amd.agent import Agent
    from rainbow_amd.feature_rank import spectrum_metrics
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
    for _ in range(3):
        agent.learn(mem)
    agent.flush()
    for batches in (8, 64):
        k = max(1, calls // (4 * batches))
        out = agent.feature_rank(mem, batches=batches)
        us = [timed(torch, lambda: agent.feature_rank(mem, batches=batches), k) for _ in range(repeats)]
        n, d = out["samples"], out["dim"]
        Kh = np.random.RandomState(0).randn(n, d)
        Kh = Kh @ Kh.T
        t0 = time.perf_counter()
        for _ in range(k):
            spectrum_metrics(Kh, n, d)
        host = (time.perf_counter() - t0) / k * 1e6
        emit(json.dumps(dict(section="rank", config=config, batches=batches, samples=n, dim=d, calls=k, repeats=repeats, **stats(us),
                             host_spectrum_us=round(host, 2), srank=out["srank"], feature_rank=out["feature_rank"],
                             effective_rank=round(out["effective_rank"], 2))))
    names = [nm for nm, _o, _s in agent._layout]
    views = [(agent._view(agent._params, nm), agent._view(agent._target_params, nm), agent._view(agent._grads, nm)) for nm in names]

    def torch_norms():
        rows = [torch.stack([p.double().norm(), p.abs().max().double(), (p.double() - q.double()).norm(), g_.double().norm()]) for p, q, g_ in views]
        return torch.stack(rows).cpu()

    variants = {"lib": agent.tensor_norms, "torch": torch_norms}
    us = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():
            for _ in range(warmup):
                fn()
        for _ in range(repeats):
            for k, fn in variants.items():
                us[k].append(timed(torch, fn, calls))
    for k in variants:
        emit(json.dumps(dict(section="norms", config=config, variant=k, tensors=len(names), params=int(agent._params.numel()), calls=calls,
                             repeats=repeats, **stats(us[k]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_rank_bench.txt"))
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    out = open(a.out, "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit("tools/rank_bench.py --calls %d --warmup %d --repeats %d: us per call, device drained before and after every timed run" % (a.calls, a.warmup, a.repeats))
    gram(a.calls, a.warmup, a.repeats, emit)
    for config in CONFIGS:
        agent_level(config, a.calls, a.warmup, a.repeats, emit)
    out.close()


if __name__ == "__main__":
    main()
