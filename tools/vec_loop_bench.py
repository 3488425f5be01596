"""The ACTING side of a vectorised training loop (main.py:147-179 for S environments) with synthetic screens,
for S in {1, 4, 16, 64}.  Per round: FramePreprocessor.observe on the S raw [210, 160] screens, roll the S frame stacks,
Agent.act_batch (one forward for all S), ReplayMemory.append_streams (one launch); and reset_noise + learn at the
reference's replay ratio — one learn per `replay_frequency` (4) environment steps, i.e. S / 4 learns per round (one learn
every 4 / S rounds below S = 4).  Prints one JSON line: env-steps/s of the whole loop and microseconds per piece, per S.
Next to `observe_us` (observe + torch.cat: two launches) stand the figures of the one-launch front end,
rainbow_amd.frames.FrameStackVec: `observe_stack_us` (step_device: the screens are on the device, as for observe_us) and
`observe_stack_upload_us` (step: from the pinned slot, the upload of 2 * S raw screens included), measured in the same process.
`--observe` measures only these three.  Not the headline metric (bench.py is)."""
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

REPLAY_FREQUENCY = 4


def timed(fn, n, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e6


def fill(mem, lib, L, capacity, actions, seed):
    """capacity + capacity / 2 transitions as whole rounds (rb_replay_append_batch takes a multiple of S in ring order), then
    bench.py's priorities."""
    dev, S = mem.device, mem.streams
    g = torch.Generator(device=dev).manual_seed(seed)
    rs = np.random.RandomState(seed)
    total, chunk = capacity + capacity // 2, 65536 - 65536 % S
    done = 0
    while done < total:
        n = min(chunk, total - done)
        n -= n % S
        fr = torch.randint(0, 256, (n, 84, 84), dtype=torch.uint8, device=dev, generator=g)
        cols = [torch.from_numpy(x).to(dev) for x in (np.zeros(n, np.int32) + 1, rs.randint(0, actions, n).astype(np.int32),
                                                      rs.choice([-1.0, 0.0, 1.0], size=n).astype(np.float32),
                                                      np.ones(n, np.uint8))]
        L.check(lib, lib.rb_replay_append_batch(mem._h, fr.data_ptr(), *[c.data_ptr() for c in cols], n, mem._stream()))
        torch.cuda.synchronize(dev)
        done += n
    mem.stream_t[:] = 1
    tree_start = 2 ** int(capacity - 1).bit_length() - 1
    g1 = torch.Generator(device=dev).manual_seed(1)
    for lo in range(0, capacity, 1024):
        k = min(1024, capacity - lo)
        mem.update_priorities(torch.arange(lo, lo + k, device=dev, dtype=torch.int64) + tree_start,
                              torch.randn(k, device=dev, generator=g1).abs() + 1e-3)
    torch.cuda.synchronize(dev)


def observe_figures(S, dev, screens=None):
    """observe + torch.cat against FrameStackVec, interleaved blocks in one process, median of 7 blocks of 200 calls."""
    from rainbow_amd.frames import FramePreprocessor, FrameStackVec
    pre, front = FramePreprocessor(dev), FrameStackVec(S, dev)
    if screens is None:
        g = torch.Generator(device=dev).manual_seed(3)
        screens = [torch.randint(0, 256, (S, 210, 160), dtype=torch.uint8, device=dev, generator=g) for _ in range(8)]
    for slot in range(2):                     # both pinned slots hold screens
        front.step(front.STEP, np.stack([screens[slot].cpu().numpy(), screens[slot + 1].cpu().numpy()], 1))
    st = {"stacks": torch.zeros((S, 4, 84, 84), device=dev), "k": 0}

    def observe():
        st["k"] += 1
        obs = pre.observe(screens[st["k"] & 7], screens[(st["k"] + 1) & 7])
        st["stacks"] = torch.cat([st["stacks"][:, 1:], obs[:, None]], dim=1)      # env.py:70 deque, per stream

    def stack_device():
        st["k"] += 1
        front.step_device(front.STEP, screens[st["k"] & 7], screens[(st["k"] + 1) & 7])

    def stack_upload():
        front.step(front.STEP)

    legs = {"observe_us": observe, "observe_stack_us": stack_device, "observe_stack_upload_us": stack_upload}
    for fn in legs.values():
        timed(fn, 50, dev)
    samples = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            samples[k].append(timed(fn, 200, dev))
    return {k: float(np.median(v)) for k, v in samples.items()}


def run(S, capacity, rounds, dev):
    import __graft_entry__
    __graft_entry__.build()
    from rainbow_amd import _lib as L
    from rainbow_amd.agent import Agent
    from rainbow_amd.frames import FramePreprocessor
    from rainbow_amd.memory import ReplayMemory
    cfg = dict(bench.CONFIGS["pong-canonical-b32"])
    args = bench.make_args(cfg, dev)
    agent = Agent(args, types.SimpleNamespace(action_space=lambda: cfg["actions"]))
    mem = ReplayMemory(args, capacity, seed=7, streams=S)
    lib = L.load()
    fill(mem, lib, L, capacity, cfg["actions"], seed=0)
    pre = FramePreprocessor(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    screens = [torch.randint(0, 256, (S, 210, 160), dtype=torch.uint8, device=dev, generator=g) for _ in range(8)]
    rs = np.random.RandomState(4)
    rewards = [rs.choice([-1.0, 0.0, 1.0], size=S) for _ in range(8)]
    no_end = np.zeros(S, dtype=bool)
    st = {"stacks": torch.zeros((S, 4, 84, 84), device=dev), "k": 0, "owed": 0.0}

    def observe():
        st["k"] += 1
        obs = pre.observe(screens[st["k"] & 7], screens[(st["k"] + 1) & 7])
        st["stacks"] = torch.cat([st["stacks"][:, 1:], obs[:, None]], dim=1)      # env.py:70 deque, per stream

    def act():
        return agent.act_batch(st["stacks"])

    def append():
        mem.append_streams(st["stacks"], np.ones(S, dtype=np.int64), rewards[st["k"] & 7], no_end)

    def learn():
        agent.reset_noise()
        agent.learn(mem)

    def round_():                 # main.py:150-164 for S environments at once
        observe()
        a = agent.act_batch(st["stacks"])
        mem.append_streams(st["stacks"], a, rewards[st["k"] & 7], no_end)
        st["owed"] += S / REPLAY_FREQUENCY
        while st["owed"] >= 1.0:
            learn()
            st["owed"] -= 1.0

    for _ in range(20):
        round_()
    out = {"act_batch_us": timed(act, 200, dev), "append_streams_us": timed(append, 200, dev)}
    out.update(observe_figures(S, dev, screens))
    for _ in range(20):
        learn()
    out["learn_us"] = timed(learn, 200, dev)
    per = timed(round_, rounds, dev)
    out["round_us"] = per
    out["env_steps_per_s"] = S * 1e6 / per
    return out


def main():
    dev = torch.device("cuda", 0)
    if "--observe" in sys.argv[1:]:
        import __graft_entry__
        __graft_entry__.build()
        print(json.dumps({"S%d" % S: {k: round(v, 2) for k, v in observe_figures(S, dev).items()} for S in (1, 4, 16, 64)}))
        return
    capacity = int(os.environ.get("LOOP_CAPACITY", str(1 << 17)))      # a multiple of every S measured
    result = {"capacity": capacity}
    for S in (1, 4, 16, 64):
        rounds = max(50, 4000 // S)
        result["S%d" % S] = {k: round(v, 2) for k, v in run(S, capacity, rounds, dev).items()}
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
