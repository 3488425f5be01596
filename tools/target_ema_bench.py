"""What a target network that follows every optimiser step costs (a measurement, not a test): back-to-back learn() at the headline
config and the data-efficient config, one PROCESS per variant, timed as tools/loop_bench.py times its pieces (device drained,
perf_counter around N calls, device drained; the pass the last call left pending runs inside the region).

  a   target_tau = 0                               today's step
  b   target_tau = 0.005, inside the optimiser pass
  c   target_tau = 1, inside the optimiser pass    (the target is only written)
  d   target_tau = 0 + rb_learner_target_ema(0.005) after every learn()     what a caller had without the in-pass EMA ...
  e   target_tau = 0 + update_target_net() after every learn()              ... and the only thing the library offered before

  python tools/target_ema_bench.py                        every variant at both configs, one child process each
  python tools/target_ema_bench.py --parent-lib PATH      also variant a, twice, on another build of the library (the parent
                                                          commit's: the spread of the two is the noise variant a has to lie within)
  python tools/target_ema_bench.py --variant b --config pong-canonical-b32      one variant in this process, one JSON line
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("pong-canonical-b32", "data-efficient-b32")
VARIANTS = ("a", "b", "c", "d", "e")
NEW_SYMBOLS = ("rb_learner_set_target_tau", "rb_learner_target_ema")


def one(variant, config, steps, warmup, repeats, old_abi):
    import numpy as np
    import torch
    import bench
    from rainbow_amd import _lib as L
    if old_abi:                       # a build from before the two entry points: bind the rest (variant a never calls them)
        assert variant == "a"
        for name in NEW_SYMBOLS:
            L.SIGNATURES.pop(name, None)
    else:
        import __graft_entry__
        __graft_entry__.build()
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[config])
    args = bench.make_args(cfg, dev)
    args.target_tau = {"b": 0.005, "c": 1.0}.get(variant, 0.0)
    env = types.SimpleNamespace(action_space=lambda: cfg["actions"])
    np.random.seed(123)
    torch.manual_seed(123)
    agent = Agent(args, env)
    mem = ReplayMemory(args, cfg["capacity"], seed=1000)
    bench.fill_replay(mem, cfg["capacity"], cfg["actions"], seed=0)

    def step():
        agent.reset_noise()
        agent.learn(mem)
        if variant == "d":
            agent.target_ema(0.005)
        elif variant == "e":
            agent.update_target_net()

    def timed(n):
        agent.flush()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        agent.flush()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e6

    for _ in range(warmup):
        step()
    us = sorted(timed(steps) for _ in range(repeats))
    print(json.dumps(dict(variant=variant, config=config, lib=os.environ.get("RAINBOW_AMD_LIB", "in-tree"), steps=steps, repeats=repeats,
                          us_per_step_min=round(us[0], 2), us_per_step_median=round(us[len(us) // 2], 2), us_per_step_max=round(us[-1], 2),
                          library_source_hash=L.source_hash(L.load()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--old-abi", action="store_true")
    a = ap.parse_args()
    if a.variant:
        return one(a.variant, a.config, a.steps, a.warmup, a.repeats, a.old_abi)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
    for config in ([a.config] if a.config else CONFIGS):
        runs = [("a", None)] + ([("a", a.parent_lib)] if a.parent_lib else []) + [(v, None) for v in VARIANTS[1:]]
        runs += [("a", a.parent_lib)] if a.parent_lib else []          # the parent build again, at the other end of the series
        runs += [("a", None)]
        for variant, lib in runs:
            env = dict(os.environ)
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", variant, "--config", config] + common
            if lib:
                env["RAINBOW_AMD_LIB"] = os.path.abspath(lib)
                cmd.append("--old-abi")
            p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)     # a fresh process per variant
            if p.returncode != 0:
                sys.stdout.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit("variant %s at %s failed with status %d: nothing more is started" % (variant, config, p.returncode))
            sys.stdout.write(p.stdout.strip().splitlines()[-1] + "\n")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
