"""usage: python tools/step_time_at_batch.py BATCH [--config NAME] [--steps N] [--warmup W] [--rounds R] — bench.py's timed loop
(Agent.reset_noise + Agent.learn(mem) on the device-resident path, the last pending optimiser pass inside the region, a device
synchronise at the end) at a batch size bench.py's configs do not have: the network, action count and multi_step of --config with
batch_size replaced.  R timed rounds in one process after one warm-up; prints one line per round and the median.  For a same-box
A/B of two builds, alternate processes with RAINBOW_AMD_LIB pointing at each (tools/gpu_env_ab.sh does the same with bench.py)."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rainbow_amd import _lib as L  # noqa: E402
from rainbow_amd.agent import Agent  # noqa: E402
from rainbow_amd.memory import ReplayMemory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("batch", type=int)
ap.add_argument("--config", default="pong-canonical-b32", choices=sorted(bench.CONFIGS))
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--capacity", type=int, default=100000)
opt = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run gives no time"
dev = torch.device("cuda", 0)
cfg = dict(bench.CONFIGS[opt.config], batch_size=opt.batch, capacity=opt.capacity)
args = bench.make_args(cfg, dev)
env = types.SimpleNamespace(action_space=lambda: cfg["actions"])
np.random.seed(123)
torch.manual_seed(123)
agent = Agent(args, env)
mem = ReplayMemory(args, cfg["capacity"], seed=1000)
bench.fill_replay(mem, cfg["capacity"], cfg["actions"], seed=0)


def run(n):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        agent.reset_noise()
        agent.learn(mem)
    agent.flush()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e6


run(opt.warmup)
us = [run(opt.steps) for _ in range(opt.rounds)]
assert mem._header().last_status == 0 and mem.failed_samples() == 0 and bool(torch.isfinite(agent._loss).all())
lib = "%s %s" % (os.path.basename(L.LIB_PATH), L.source_hash(L.load()))      # which build: the hash of its sources
for r, t in enumerate(us):
    print("[%s] %s batch %d round %d: %.2f us/step" % (lib, opt.config, opt.batch, r + 1, t))
print("[%s] %s batch %d median of %d rounds x %d steps: %.2f us/step" % (lib, opt.config, opt.batch, opt.rounds, opt.steps, float(np.median(us))))
