"""What the random-shift frame-stack gather costs (a measurement, not a test), in ONE process on cuda:0:
  1. the replay alone, history 4, at batch 32 and 256: the draw without stacks, the plain path (rb_replay_sample handed stack
     pointers: k_sample + k_gather_stacks), and the new path (rb_replay_sample with NULL stacks + rb_replay_gather_shifted:
     k_sample + k_gather_stacks_shift) with pad 0 and pad 4 — stream time per call from device events around CALLS back-to-back
     calls, the variants interleaved over REPS repetitions, medians and the run-to-run spread (min .. max of the repetitions);
  2. the learn step at the data-efficient configuration through rainbow_amd.Agent with augment_pad 0 (the zero-copy path:
     conv1 reads the ring) and 4 (the gathered path: sampler launch, shifted gather, rb_learner_learn) — wall time per step
     over windows that end in a device synchronise, interleaved, medians and spread.  The difference between the two IS the
     price of the feature: the gathered path pays for building the stacks at all, not only for shifting them.
    python tools/shift_gather_bench.py [--reps 9] [--calls 300] [--steps 300]"""
import argparse
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CFG = dict(bench.CONFIGS["data-efficient-b32"])


def fmt(xs):
    return "median %8.2f us   spread %8.2f .. %8.2f" % (statistics.median(xs), min(xs), max(xs))


def gather_part(dev, reps, calls):
    from rainbow_amd.memory import ReplayMemory
    args = bench.make_args(CFG, dev)
    mem = ReplayMemory(args, CFG["capacity"], seed=7)
    bench.fill_replay(mem, CFG["capacity"], CFG["actions"], seed=0)
    lib, h, stream = mem._lib, mem._h, mem._stream()
    for B in (32, 256):
        o = mem._buffers(B)
        sh = torch.zeros(B, 2, 2, dtype=torch.int8, device=dev)
        scal = (o["actions"].data_ptr(), o["returns"].data_ptr(), o["nonterminals"].data_ptr(), o["weights"].data_ptr())
        st, ns = o["states"].data_ptr(), o["next_states"].data_ptr()

        def draw(with_stacks):
            rc = lib.rb_replay_sample(h, B, 0.4, None, mem.MAX_ATTEMPTS, o["tree_idxs"].data_ptr(), st if with_stacks else None,
                                      ns if with_stacks else None, *scal, stream)
            assert rc == 0, lib.rb_last_error()

        def shifted(pad, k):
            draw(False)
            rc = lib.rb_replay_gather_shifted(h, B, pad, k, None, st, ns, sh.data_ptr(), stream)
            assert rc == 0, lib.rb_last_error()

        variants = {"draw only (NULL stacks)": lambda k: draw(False), "plain path (draw + k_gather_stacks)": lambda k: draw(True),
                    "new path pad 0 (draw + k_gather_stacks_shift)": lambda k: shifted(0, k),
                    "new path pad 4 (draw + k_gather_stacks_shift)": lambda k: shifted(4, k)}
        times = {name: [] for name in variants}
        for name, fn in variants.items():                 # warm-up: every shape and kernel once
            for k in range(20):
                fn(k)
        torch.cuda.synchronize(dev)
        for r in range(reps):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(calls):
                    fn(r * calls + k)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
        print("replay alone, batch %d, history 4, multi_step %d, capacity %d: stream time per call (%d reps x %d calls)"
              % (B, CFG["multi_step"], CFG["capacity"], reps, calls))
        for name in variants:
            print("  %-48s %s" % (name, fmt(times[name])))
        med = {name: statistics.median(v) for name, v in times.items()}
        names = list(variants)
        print("  gather alone (path - draw only):  plain %.2f us   shifted pad 0 %.2f us   shifted pad 4 %.2f us   [%d frames of 7056 B]"
              % (med[names[1]] - med[names[0]], med[names[2]] - med[names[0]], med[names[3]] - med[names[0]], B * 8), flush=True)
    del mem


def learn_part(dev, reps, steps):
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    env = types.SimpleNamespace(action_space=lambda: CFG["actions"])
    runs = {}
    for pad in (0, 4):
        args = bench.make_args(CFG, dev)
        args.augment_pad = pad
        torch.manual_seed(1)
        agent = Agent(args, env)
        mem = ReplayMemory(args, CFG["capacity"], seed=7)
        bench.fill_replay(mem, CFG["capacity"], CFG["actions"], seed=0)
        runs[pad] = (agent, mem, [])
    for agent, mem, _ in runs.values():
        for _ in range(50):
            agent.learn(mem)
    torch.cuda.synchronize(dev)
    for r in range(reps):
        for pad, (agent, mem, ts) in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                agent.learn(mem)
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) / steps * 1e6)
    print("learn step through rainbow_amd.Agent, data-efficient config (batch %d, hidden %d, multi_step %d, capacity %d): wall time "
          "per step (%d reps x %d steps)" % (CFG["batch_size"], CFG["hidden_size"], CFG["multi_step"], CFG["capacity"], reps, steps))
    print("  %-48s %s" % ("augment_pad 0 (zero-copy path)", fmt(runs[0][2])))
    print("  %-48s %s" % ("augment_pad 4 (gathered path + shifted gather)", fmt(runs[4][2])))
    print("  the price of the feature: %+.2f us per step" % (statistics.median(runs[4][2]) - statistics.median(runs[0][2])), flush=True)
    for agent, mem, _ in runs.values():
        assert mem.failed_samples() == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    dev = torch.device("cuda", 0)
    print("command: python tools/shift_gather_bench.py --reps %d --calls %d --steps %d" % (a.reps, a.calls, a.steps))
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    gather_part(dev, a.reps, a.calls)
    learn_part(dev, a.reps, a.steps)


if __name__ == "__main__":
    main()
