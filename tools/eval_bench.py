"""Evaluation episodes per second on the device Catch (a measurement, not a test; no threshold): rainbow_amd.loop.evaluate_vec
for S in {1, 16, 64} against the reference-shaped single-environment loop it replaces (test.py:19-34: Agent.act_e_greedy +
CatchVec(1).step(int), one stream synchronise per environment step), in the same process, the two legs alternating.

Per S: both legs are warmed up, then timed `--repeats` times in turn; a leg is a host clock around whole evaluations that end
in a device synchronise (evaluate_vec's last poll / the single loop's last step).  Printed per S: the median episodes/s of both
legs with their min-max, and the ratio of the medians.  `--out FILE` also writes the lines to FILE (profiles/eval_vec_bench.txt
is the committed record).  The agent is untrained: the work per environment step does not depend on what the network
computes, and every Catch episode is 11 steps."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def options(dev):
    """The data-efficient recipe tools/catch_learning_curve.py trains with."""
    return types.SimpleNamespace(
        device=dev, architecture="data-efficient", hidden_size=256, multi_step=20, learning_rate=1e-4, replay_frequency=1,
        target_update=2000, batch_size=32, atoms=51, V_min=-10.0, V_max=10.0, history_length=4, noisy_std=0.1, discount=0.99,
        priority_exponent=0.5, priority_weight=0.4, adam_eps=1.5e-4, norm_clip=10.0, reward_clip=1, learn_start=1600, model=None)


def single_loop(agent, env, episodes, epsilon=0.001):
    """test.py:19-34 as the reference runs it: one act, one step, one synchronise per environment step."""
    agent.eval()
    rewards, done = [], True
    for _ in range(episodes):
        while True:
            if done:
                state, reward_sum, done = env.reset(), 0, False
            state, reward, done = env.step(agent.act_e_greedy(state, epsilon))
            reward_sum += reward
            if done:
                rewards.append(reward_sum)
                break
    return rewards


def measure(S, vec_episodes, single_episodes, repeats, dev):
    from rainbow_amd.agent import Agent
    from rainbow_amd.envs import CatchVec
    from rainbow_amd.loop import evaluate_vec
    torch.manual_seed(1)
    np.random.seed(1)
    env_vec, env_one = CatchVec(S, dev, seed=11), CatchVec(1, dev, seed=12)
    agent = Agent(options(dev), env_vec)

    def vec_leg(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = evaluate_vec(agent, env_vec, n, epsilon=0.001, seed=3)
        torch.cuda.synchronize(dev)
        assert len(out["rewards"]) == n
        return n / (time.perf_counter() - t0)

    def single_leg(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = single_loop(agent, env_one, n)
        torch.cuda.synchronize(dev)
        assert len(out) == n
        return n / (time.perf_counter() - t0)

    vec_leg(max(S, 8))
    single_leg(4)
    vec, single = [], []
    for _ in range(repeats):
        vec.append(vec_leg(vec_episodes))
        single.append(single_leg(single_episodes))
    env_vec.close()
    env_one.close()
    return vec, single


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--vec-episodes", type=int, default=8192, help="episodes per evaluate_vec call (at S = 1: a quarter of it)")
    ap.add_argument("--single-episodes", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_bench.py measures on the device: no GPU visible")
    import __graft_entry__
    __graft_entry__.build()
    from rainbow_amd import _lib as L
    dev = torch.device("cuda", 0)
    lines = ["evaluation episodes/s on the device Catch (11 steps per episode), epsilon 0.001, data-efficient net (hidden 256), untrained",
             "device %s, library %s; median of %d alternating repeats [min .. max]" % (torch.cuda.get_device_name(0), L.source_hash(L.load()),
                                                                                     a.repeats),
             "vec = rainbow_amd.loop.evaluate_vec (poll every 8 rounds); single = act_e_greedy + CatchVec(1).step(int), one synchronise per step"]
    for S in a.streams:
        n_vec = a.vec_episodes if S > 1 else max(8, a.vec_episodes // 4)
        vec, single = measure(S, n_vec, a.single_episodes, a.repeats, dev)
        mv, ms = float(np.median(vec)), float(np.median(single))
        lines.append("S %2d  vec %9.1f eps/s [%9.1f .. %9.1f] (%d episodes per call)   single %8.1f eps/s [%8.1f .. %8.1f] (%d episodes per call)   "
                     "ratio %6.2f" % (S, mv, min(vec), max(vec), n_vec, ms, min(single), max(single), a.single_episodes, mv / ms))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
