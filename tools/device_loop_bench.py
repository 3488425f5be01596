"""Host-driven round against device-resident round of the vectorised actor loop, same box, same process, interleaved A/B, for
S in {1, 4, 16, 64} at the headline config (bench.py's pong-canonical-b32 network; 3 actions: the game's).

  A (host-driven, tools/vec_loop_bench.py's shape):  Agent.act_batch -> numpy (stream synchronise) -> host environment
     stand-in (rewards / terminals from a table) -> ReplayMemory.append_streams with host operands (by value in the launch)
  B (device round):  Agent.act_batch(device_out=True) -> CatchVec.step_device -> append_streams with device operands

Both sides launch the same Catch step kernel for their next frame stacks (A feeds it a fixed device action vector: a host
environment would upload whole frames instead, which A is not charged for), so the difference is the per-round synchronise,
the D2H / by-value operand marshalling and the interpreter work around them.  Measured twice: the acting round alone, and the
whole loop with reset_noise + learn at the reference's ratio (one learn per 4 env steps).  Blocks of rounds alternate
A, B, A, B, ...; the figure is the median block.  Prints a small table and one JSON line.  Not the headline metric (bench.py is).

  --per-stream-noise: instead, the device round against ITSELF with one noisy-net sample per stream (run_noise below).
  --env {catch,breakout}: the device environment of either mode (default catch: what this tool always measured).
  --compare-envs: instead, the device round on CatchVec against the same round on BreakoutVec (training mode), S in {1, 16, 64},
     interleaved as above, plus the environment's step launch alone (run_envs below): Catch is the yardstick of the new game."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import vec_loop_bench  # noqa: E402

REPLAY_FREQUENCY = 4
BLOCKS = 7
ENV = "catch"


def make_env(S, dev, seed, name=None):
    from rainbow_amd.envs import BreakoutVec, CatchVec
    return {"catch": CatchVec, "breakout": BreakoutVec}[name or ENV](S, dev, seed=seed)


def block(fn, n, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e6


def run(S, capacity, rounds, dev):
    from rainbow_amd import _lib as L
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    cfg = dict(bench.CONFIGS["pong-canonical-b32"])
    args = bench.make_args(cfg, dev)
    lib = L.load()
    envs = {k: make_env(S, dev, 11) for k in "AB"}
    agent = Agent(args, envs["A"])
    mems = {k: ReplayMemory(args, capacity, seed=7, streams=S) for k in "AB"}
    for m in mems.values():
        vec_loop_bench.fill(m, lib, L, capacity, envs["A"].action_space(), seed=0)
    rs = np.random.RandomState(4)
    rewards = [rs.choice([-1.0, 0.0, 1.0], size=S) for _ in range(8)]
    no_end = np.zeros(S, dtype=bool)
    fixed_actions = torch.zeros(S, dtype=torch.int32, device=dev)
    st = {k: {"stacks": envs[k].reset().reshape(S, 4, 84, 84), "k": 0, "owed": 0.0} for k in "AB"}

    def learn_owed(s, mem):
        s["owed"] += S / REPLAY_FREQUENCY
        while s["owed"] >= 1.0:
            agent.reset_noise()
            agent.learn(mem)
            s["owed"] -= 1.0

    def round_a(learn):
        s = st["A"]
        s["k"] += 1
        a = agent.act_batch(s["stacks"])                                   # synchronises; numpy
        rw, te = rewards[s["k"] & 7], no_end                               # the host environment stand-in
        nxt, _, _ = envs["A"].step_device(fixed_actions)
        mems["A"].append_streams(s["stacks"], a, rw, te)
        s["stacks"] = nxt
        if learn:
            learn_owed(s, mems["A"])

    def round_b(learn):
        s = st["B"]
        a = agent.act_batch(s["stacks"], device_out=True)
        nxt, rw, nt = envs["B"].step_device(a)
        mems["B"].append_streams(s["stacks"], a, rw, nonterminals=nt)
        s["stacks"] = nxt
        if learn:
            learn_owed(s, mems["B"])

    out = {}
    for learn, tag in ((False, "act_round"), (True, "loop_round")):
        for _ in range(20):
            round_a(learn); round_b(learn)
        ta, tb = [], []
        for _ in range(BLOCKS):
            ta.append(block(lambda: round_a(learn), rounds, dev))
            tb.append(block(lambda: round_b(learn), rounds, dev))
        out[tag + "_host_us"], out[tag + "_device_us"] = statistics.median(ta), statistics.median(tb)
        out[tag + "_host_spread_us"] = max(ta) - min(ta)
        out[tag + "_device_spread_us"] = max(tb) - min(tb)
    out["env_steps_per_s_host"] = S * 1e6 / out["loop_round_host_us"]
    out["env_steps_per_s_device"] = S * 1e6 / out["loop_round_device_us"]
    for e in envs.values():
        e.close()
    return out


def run_noise(S, capacity, rounds, dev):
    """--per-stream-noise: the DEVICE round with the one shared noisy-net sample (A) against the same round with one sample per
    stream (B: Agent.reset_noise_rows at train_device's cadence + act_batch(per_row_noise=True)), interleaved as above."""
    from rainbow_amd import _lib as L
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    cfg = dict(bench.CONFIGS["pong-canonical-b32"])
    args = bench.make_args(cfg, dev)
    lib = L.load()
    envs = {k: make_env(S, dev, 11) for k in "AB"}
    agent = Agent(args, envs["A"])
    mems = {k: ReplayMemory(args, capacity, seed=7, streams=S) for k in "AB"}
    for m in mems.values():
        vec_loop_bench.fill(m, lib, L, capacity, envs["A"].action_space(), seed=0)
    st = {k: {"stacks": envs[k].reset().reshape(S, 4, 84, 84), "T": 1, "owed": 0.0} for k in "AB"}
    agent.reset_noise_rows(S, rng=(0, 0))

    def one_round(k, learn):
        s = st[k]
        rows = k == "B"
        if rows and s["T"] % REPLAY_FREQUENCY < S:
            agent.reset_noise_rows(S, rng=(0, s["T"]))
        a = agent.act_batch(s["stacks"], device_out=True, per_row_noise=rows)
        nxt, rw, nt = envs[k].step_device(a)
        mems[k].append_streams(s["stacks"], a, rw, nonterminals=nt)
        s["stacks"] = nxt
        s["T"] += S
        if learn:
            s["owed"] += S / REPLAY_FREQUENCY
            while s["owed"] >= 1.0:
                agent.reset_noise()
                agent.learn(mems[k])
                s["owed"] -= 1.0

    out = {}
    for learn, tag in ((False, "act_round"), (True, "loop_round")):
        for _ in range(20):
            one_round("A", learn); one_round("B", learn)
        ta, tb = [], []
        for _ in range(BLOCKS):
            ta.append(block(lambda: one_round("A", learn), rounds, dev))
            tb.append(block(lambda: one_round("B", learn), rounds, dev))
        out[tag + "_shared_us"], out[tag + "_per_stream_us"] = statistics.median(ta), statistics.median(tb)
        out[tag + "_shared_spread_us"] = max(ta) - min(ta)
        out[tag + "_per_stream_spread_us"] = max(tb) - min(tb)
    for e in envs.values():
        e.close()
    return out


def run_envs(S, capacity, rounds, dev):
    """--compare-envs: the device round on Catch (A) against the same round on Breakout (B), and each game's step launch alone."""
    from rainbow_amd import _lib as L
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    cfg = dict(bench.CONFIGS["pong-canonical-b32"])
    args = bench.make_args(cfg, dev)
    lib = L.load()
    envs = {"A": make_env(S, dev, 11, "catch"), "B": make_env(S, dev, 11, "breakout")}
    agent = Agent(args, envs["A"])
    mems = {k: ReplayMemory(args, capacity, seed=7, streams=S) for k in "AB"}
    for m in mems.values():
        vec_loop_bench.fill(m, lib, L, capacity, envs["A"].action_space(), seed=0)
    st = {k: {"stacks": envs[k].reset().reshape(S, 4, 84, 84), "owed": 0.0} for k in "AB"}
    moves = [torch.from_numpy(np.random.RandomState(i).randint(0, 3, S).astype(np.int32)).to(dev) for i in range(8)]
    count = {"A": 0, "B": 0}

    def step_only(k):
        count[k] += 1
        envs[k].step_device(moves[count[k] & 7])

    def one_round(k, learn):
        s = st[k]
        a = agent.act_batch(s["stacks"], device_out=True)
        nxt, rw, nt = envs[k].step_device(a)
        mems[k].append_streams(s["stacks"], a, rw, nonterminals=nt)
        s["stacks"] = nxt
        if learn:
            s["owed"] += S / REPLAY_FREQUENCY
            while s["owed"] >= 1.0:
                agent.reset_noise()
                agent.learn(mems[k])
                s["owed"] -= 1.0

    out = {}
    for tag, fn in (("env_step", step_only), ("act_round", lambda k: one_round(k, False)), ("loop_round", lambda k: one_round(k, True))):
        for _ in range(20):
            fn("A"); fn("B")
        ta, tb = [], []
        for _ in range(BLOCKS):
            ta.append(block(lambda: fn("A"), rounds, dev))
            tb.append(block(lambda: fn("B"), rounds, dev))
        out[tag + "_catch_us"], out[tag + "_breakout_us"] = statistics.median(ta), statistics.median(tb)
        out[tag + "_catch_spread_us"] = max(ta) - min(ta)
        out[tag + "_breakout_spread_us"] = max(tb) - min(tb)
    out["breakout_stats"] = envs["B"].stats()
    for e in envs.values():
        e.close()
    return out


def main_envs(dev, capacity):
    result = {"capacity": capacity, "blocks": BLOCKS, "mode": "compare-envs"}
    print("%3s | %-38s | %-38s | %-38s" % ("S", "env step alone us: catch / breakout", "acting round us: catch / breakout",
                                          "loop round us (+learns): catch / breakout"))
    for S in (1, 16, 64):
        rounds = max(40, 2000 // S)
        r = run_envs(S, capacity, rounds, dev)
        r = {k: round(v, 2) if isinstance(v, float) else v for k, v in r.items()}
        result["S%d" % S] = r
        print("%3d | %8.1f / %-8.1f (spread %4.1f / %4.1f) | %8.1f / %-8.1f (spread %4.1f / %4.1f) | %8.1f / %-8.1f (spread %4.1f / %4.1f)"
              % ((S,) + tuple(r["%s_%s_us" % (t, g)] for t in ("env_step", "act_round", "loop_round")
                              for g in ("catch", "breakout", "catch_spread", "breakout_spread"))), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(result))


def main_noise(dev, capacity):
    result = {"capacity": capacity, "blocks": BLOCKS, "mode": "per-stream-noise"}
    print("%3s | %-44s | %-44s" % ("S", "acting round us: shared / per-stream noise", "loop round us (+learns): shared / per-stream noise"))
    for S in (1, 4, 16, 64):
        rounds = max(40, 2000 // S)
        r = {k: round(v, 2) for k, v in run_noise(S, capacity, rounds, dev).items()}
        result["S%d" % S] = r
        print("%3d | %10.1f / %-10.1f (spread %4.1f / %4.1f) | %10.1f / %-10.1f (spread %4.1f / %4.1f)"
              % (S, r["act_round_shared_us"], r["act_round_per_stream_us"], r["act_round_shared_spread_us"], r["act_round_per_stream_spread_us"],
                 r["loop_round_shared_us"], r["loop_round_per_stream_us"], r["loop_round_shared_spread_us"], r["loop_round_per_stream_spread_us"]),
              flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(result))


def main():
    import __graft_entry__
    __graft_entry__.build()
    dev = torch.device("cuda", 0)
    capacity = int(os.environ.get("LOOP_CAPACITY", str(1 << 17)))      # a multiple of every S measured
    global ENV
    argv = sys.argv[1:]
    if "--env" in argv:
        ENV = argv[argv.index("--env") + 1]
        if ENV not in ("catch", "breakout"):
            raise SystemExit("--env must be catch or breakout, got %r" % ENV)
    if "--compare-envs" in argv:
        return main_envs(dev, capacity)
    if "--per-stream-noise" in argv:
        return main_noise(dev, capacity)
    result = {"capacity": capacity, "blocks": BLOCKS, "env": ENV}
    print("%3s | %-34s | %-34s | env-steps/s host -> device" % ("S", "acting round us: host / device", "loop round us (+learns): host / device"))
    for S in (1, 4, 16, 64):
        rounds = max(40, 2000 // S)
        r = {k: round(v, 2) for k, v in run(S, capacity, rounds, dev).items()}
        result["S%d" % S] = r
        print("%3d | %10.1f / %-10.1f (spread %4.1f / %4.1f) | %10.1f / %-10.1f | %9.0f -> %9.0f"
              % (S, r["act_round_host_us"], r["act_round_device_us"], r["act_round_host_spread_us"], r["act_round_device_spread_us"],
                 r["loop_round_host_us"], r["loop_round_device_us"], r["env_steps_per_s_host"], r["env_steps_per_s_device"]), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
