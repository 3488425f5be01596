"""What the device-side diagnostics cost (a measurement, not a test): us per learn step at the headline and the data-efficient
config of bench.py in three settings, interleaved round by round in ONE process on one agent (timed as tools/loop_bench.py times
its pieces: device drained, perf_counter around N calls, device drained; the pass the last call left pending runs inside the region)

  off    no record ring                                           today's step: one launch fewer than `on`
  on     Agent.track_stats(4096): one k_step_stats launch per step, nothing read until the region ends
  sync   no ring; agent._loss and agent._norm read on the host after every step — what a caller who wanted a loss curve had to do

then rb_learner_eval_loss (Agent.evaluate_loss, one batch, its synchronising read-back included) at both configs and
rb_replay_priority_stats on a replay of 2^20 slots (stream time of the launch alone, and ReplayMemory.priority_stats with its
read-back).  Appends its lines to profiles/diag_bench.txt (--out), next to the library's source hash.

  python tools/diag_bench.py [--steps 1000 --warmup 200 --rounds 5] [--out profiles/diag_bench.txt]
"""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("pong-canonical-b32", "data-efficient-b32")
SETTINGS = ("off", "on", "sync")


def learn_settings(config, steps, warmup, rounds, emit):
    import numpy as np
    import torch
    import bench
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[config])
    args = bench.make_args(cfg, dev)
    env = types.SimpleNamespace(action_space=lambda: cfg["actions"])
    np.random.seed(123)
    torch.manual_seed(123)
    agent = Agent(args, env)
    mem = ReplayMemory(args, cfg["capacity"], seed=1000)
    bench.fill_replay(mem, cfg["capacity"], cfg["actions"], seed=0)
    sink = []

    def step(setting):
        agent.reset_noise()
        agent.learn(mem)
        if setting == "sync":
            sink.append((agent._loss.mean().item(), agent._norm.item()))
            del sink[:-1]

    def timed(setting, n):
        agent.track_stats(4096 if setting == "on" else 0)
        for _ in range(20):
            step(setting)
        agent.flush()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            step(setting)
        agent.flush()
        torch.cuda.synchronize(dev)
        us = (time.perf_counter() - t0) / n * 1e6
        if setting == "on":
            r = agent.read_stats()
            assert r["step"].size == min(n + 20, 4096) and np.isfinite(r["loss_mean"]).all()
        return us

    for _ in range(warmup):
        step("off")
    res = {s: [] for s in SETTINGS}
    for _ in range(rounds):
        for s in SETTINGS:
            res[s].append(timed(s, steps))
    for s in SETTINGS:
        v = sorted(res[s])
        emit("%-20s learn step, %-4s  us per step: min %.2f median %.2f max %.2f  (%d rounds of %d steps)"
             % (config, s, v[0], v[len(v) // 2], v[-1], rounds, steps))
    med = {s: sorted(res[s])[len(res[s]) // 2] for s in SETTINGS}
    emit("%-20s ring on - off: %+.2f us per step (medians); sync - off: %+.2f us" % (config, med["on"] - med["off"], med["sync"] - med["off"]))
    # ---- where the ring-on cost goes: the k_step_stats launch alone, bracketed by events (rb_profile_select; the brackets serialise
    # the stream around it, so this is the kernel's own duration, not its cost inside the step)
    import ctypes as C
    from rainbow_amd import _lib as L
    lib = L.load()
    agent.track_stats(4096)
    for _ in range(20):
        step("on")
    agent.flush()
    torch.cuda.synchronize(dev)
    L.check(lib, lib.rb_profile_select(b"k_step_stats"))
    for _ in range(200):
        step("on")
    agent.flush()
    torch.cuda.synchronize(dev)
    ms, nl = C.c_double(0), C.c_int64(0)
    L.check(lib, lib.rb_profile_read(C.byref(ms), C.byref(nl)))
    L.check(lib, lib.rb_profile_select(None))
    emit("%-20s k_step_stats alone (event brackets, %d launches): %.2f us per launch, grid %d x 256 threads"
         % (config, nl.value, ms.value / max(nl.value, 1) * 1e3, -(-args.batch_size // 16)))
    # ---- the held-out loss, one batch per call, read back
    agent.track_stats(0)
    uu = torch.from_numpy(np.random.RandomState(1).random_sample((64, args.batch_size))).to(dev)
    for _ in range(10):
        agent.evaluate_loss(mem, unit_uniforms=uu)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    n = 200
    for _ in range(n):
        agent.evaluate_loss(mem, unit_uniforms=uu)
    torch.cuda.synchronize(dev)
    emit("%-20s Agent.evaluate_loss (draw + gather + 3 forwards + head + record, read back): %.1f us per batch"
         % (config, (time.perf_counter() - t0) / n * 1e6))


def priority_stats(emit):
    import ctypes as C
    import numpy as np
    import torch
    from rainbow_amd import _lib as L
    from rainbow_amd.memory import ReplayMemory
    dev = torch.device("cuda", 0)
    args = types.SimpleNamespace(device=dev, history_length=4, discount=0.99, multi_step=3, priority_weight=0.4, priority_exponent=0.5)
    mem = ReplayMemory(args, 1 << 20, seed=3)
    lib = L.load()
    b = L.ReplayBuffers()
    L.check(lib, lib.rb_replay_buffers(mem._h, C.byref(b)))
    rs = np.random.RandomState(0)
    for _ in range(64):           # priorities all over the tree
        idx = torch.from_numpy(b.tree_start + rs.choice(1 << 20, size=1024, replace=False)).to(dev)
        val = torch.from_numpy(rs.uniform(0.01, 3.0, size=1024).astype(np.float32)).to(dev)
        L.check(lib, lib.rb_replay_update_leaves(mem._h, idx.data_ptr(), val.data_ptr(), 1024, mem._stream()))
    s = mem.priority_stats()
    out = torch.empty(C.sizeof(L.PriorityStats), dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 200
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(n):
        L.check(lib, lib.rb_replay_priority_stats(mem._h, out.data_ptr(), mem._stream()))
    e1.record()
    torch.cuda.synchronize(dev)
    emit("rb_replay_priority_stats, 2^20 slots (%d non-zero leaves, ess %.0f): %.2f us per launch back to back (4 MB of leaves: "
         "%.0f GB/s)" % (s["nonzero"], s["ess"], e0.elapsed_time(e1) / n * 1e3, 4.194304e6 / (e0.elapsed_time(e1) / n * 1e-3) / 1e9))
    t0 = time.perf_counter()
    for _ in range(50):
        mem.priority_stats()
    emit("ReplayMemory.priority_stats with its read-back: %.1f us per call" % ((time.perf_counter() - t0) / 50 * 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_bench.txt"))
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from rainbow_amd import _lib as L
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("tools/diag_bench.py --steps %d --warmup %d --rounds %d; library source hash %s" % (a.steps, a.warmup, a.rounds, L.source_hash(L.load())))
    for config in CONFIGS:
        learn_settings(config, a.steps, a.warmup, a.rounds, emit)
    priority_stats(emit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
