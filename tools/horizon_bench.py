"""What the annealed update horizon costs (a measurement, not a test), at the headline config and the data-efficient config, both
built with multi_step = n_max = 10 (everything else bench.py's: replay capacity, fill, network, batch):

  (a) one set_horizon pair — Agent.set_horizon (host state) + ReplayMemory.set_horizon (one 64-thread launch that stores the
      gamma^k table in stream order) — timed as tools/reset_bench.py times its calls: device drained, perf_counter around N pairs
      that alternate between (10, 0.97) and (3, 0.997), device drained;
  (b) the learn step (bench.py's step: reset_noise + learn) at n_eff = 10 and at n_eff = 3 of n_max = 10: K steps per leg, the legs
      interleaved (10, 3, 10, 3, ...), device drained around each;
  (c) bench.py's own figure (--gpus 1 --steps K --warmup W --config <config>, the default path: no set_horizon call anywhere) on
      this tree against the parent commit on the same box: the parent twice — the difference of the two is the box's run-to-run
      spread — then this tree twice.  The default path launches the same kernels with the same arguments, so the tree's figure has
      to lie within that spread of the parent's; the four numbers are recorded, and the verdict with them.

  python tools/horizon_bench.py --parent DIR [--out profiles/horizon_bench.txt]
        DIR: a checkout of the parent commit with its library built (python DIR/__graft_entry__.py); without --parent (c) is left out.
Every bench.py leg runs in a process of its own, one at a time."""
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
N_MAX = 10
HI, LO = (10, 0.97), (3, 0.997)


def one(config, steps, warmup, legs, pairs):
    import numpy as np
    import torch
    import bench
    import __graft_entry__
    __graft_entry__.build()
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[config], multi_step=N_MAX)
    args = bench.make_args(cfg, dev)
    args.discount = HI[1]
    env = types.SimpleNamespace(action_space=lambda: cfg["actions"])
    np.random.seed(123)
    torch.manual_seed(123)
    agent = Agent(args, env)
    mem = ReplayMemory(args, cfg["capacity"], seed=1000)
    bench.fill_replay(mem, cfg["capacity"], cfg["actions"], seed=0)

    def drain():
        agent.flush()
        torch.cuda.synchronize(dev)

    def set_both(hz):
        agent.set_horizon(*hz)
        mem.set_horizon(*hz)

    def run(k):
        for _ in range(k):
            agent.reset_noise()
            agent.learn(mem)
        drain()

    rows = []
    # ---- (b)
    times = {HI: [], LO: []}
    for leg in range(legs):
        for hz in (HI, LO):
            set_both(hz)
            run(warmup)
            t0 = time.perf_counter()
            run(steps)
            times[hz].append((time.perf_counter() - t0) / steps * 1e6)
    assert mem.failed_samples() == 0 and bool(torch.isfinite(agent._loss).all())
    for hz in (HI, LO):
        us = sorted(times[hz])
        rows.append(dict(what="learn step", config=config, n_max=N_MAX, n_eff=hz[0], discount=hz[1], steps=steps, legs=legs,
                         us_per_step_min=round(us[0], 2), us_per_step_median=round(us[len(us) // 2], 2), us_per_step_max=round(us[-1], 2)))
        print(json.dumps(rows[-1]), flush=True)
    # ---- (a)
    drain()
    us = []
    for _ in range(5):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(pairs):
            set_both(LO if i & 1 else HI)
        torch.cuda.synchronize(dev)
        us.append((time.perf_counter() - t0) / pairs * 1e6)
    us.sort()
    rows.append(dict(what="set_horizon pair", config=config, n_max=N_MAX, pairs=pairs, repeats=5, us_per_pair_min=round(us[0], 2),
                     us_per_pair_median=round(us[2], 2), us_per_pair_max=round(us[-1], 2)))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_figure(tree, config, steps, warmup):
    """bench.py's result line from a process of its own in `tree`."""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--config", config],
                         cwd=tree, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout      # (a hung run ends the script)
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: adds (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "horizon_bench.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for config in ([a.config] if a.config else CONFIGS) if a.parent else ():     # first, before this process opens the device
        say("(c) bench.py --gpus 1 --steps %d --warmup %d --config %s, one process per run" % (a.steps, a.warmup, config))
        res = []
        for who, tree in (("parent", a.parent), ("parent", a.parent), ("tree", ROOT), ("tree", ROOT)):
            r = bench_figure(tree, config, a.steps, a.warmup)
            res.append((who, r))
            say("    %-6s %10.2f gradient-steps/s  %8.2f us/step   library %s" % (who, r["value"], r["ms_per_step"] * 1e3, r["library_source_hash"]))
        p = [r["value"] for who, r in res if who == "parent"]
        t = [r["value"] for who, r in res if who == "tree"]
        spread = abs(p[0] - p[1])
        mean = sum(p) / 2
        lo, hi = mean - spread, mean + spread
        say("    parent's run-to-run spread %.2f steps/s (%.3f %%): the tree must lie within it of the parent's mean, in [%.2f, %.2f]"
            % (spread, 100 * spread / max(p), lo, hi))
        for v in t:
            verdict = "within" if lo <= v <= hi else ("ABOVE the band (faster)" if v > hi else "BELOW the band (slower)")
            say("    tree %.2f: %s (%+.3f %% against the parent's mean)" % (v, verdict, 100 * (v / mean - 1)))
        say()
    rows = []
    for config in ([a.config] if a.config else CONFIGS):
        rows += one(config, a.steps, a.warmup, a.legs, a.pairs)
    say("(b) the learn step at n_eff of n_max = %d (%d steps per leg, %d interleaved legs each)" % (N_MAX, a.steps, a.legs))
    say("    %-20s %6s %9s %10s %10s %10s" % ("config", "n_eff", "discount", "min us", "median us", "max us"))
    for r in rows:
        if r["what"] == "learn step":
            say("    %-20s %6d %9.3f %10.2f %10.2f %10.2f" % (r["config"], r["n_eff"], r["discount"], r["us_per_step_min"],
                                                              r["us_per_step_median"], r["us_per_step_max"]))
    say()
    say("(a) one set_horizon pair, agent + memory (%d pairs per repeat, 5 repeats, device drained around each)" % a.pairs)
    say("    %-20s %10s %10s %10s" % ("config", "min us", "median us", "max us"))
    for r in rows:
        if r["what"] == "set_horizon pair":
            say("    %-20s %10.2f %10.2f %10.2f" % (r["config"], r["us_per_pair_min"], r["us_per_pair_median"], r["us_per_pair_max"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
