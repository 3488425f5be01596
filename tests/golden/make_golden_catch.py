"""Fixture generator for a learning check: how fast the REAL reference Agent + ReplayMemory learn Catch.

STATUS: no fixture is committed and no test consumes one.  The file is only written when every reference seed ends at an
evaluation return >= 0.8, and the reference did not get there: see profiles/catch_learning_curve.txt for the curves this
script produced (3-cell paddle up to T_max = 20 000; 5-cell paddle at T_max = 10 000, where one seed stalled at +0.36 and one
never returned from the reference sampler's rejection loop).  Kept so the experiment can be repeated.

Imports the reference's `agent.Agent` and `memory.ReplayMemory` from a checkout given with --reference (or $RAINBOW_REFERENCE)
at generation time, on the CPU, and drives them with tests/catch_oracle.py's single-stream Env through a loop of main.py:146-184's
shape (main.py itself needs atari_py).  Only recorded results are written: tests/golden/catch_learning.npz.

    python tests/golden/make_golden_catch.py --reference PATH --time-pieces          # what does a step cost here?
    python tests/golden/make_golden_catch.py --reference PATH --t-max 4000 --explore # curves only, nothing written
    python tests/golden/make_golden_catch.py --reference PATH --t-max 10000          # assert + write the fixture

Options: the reference's published data-efficient settings (README: --architecture data-efficient --hidden-size 256
--multi-step 20 --learning-rate 1e-4 --replay-frequency 1 --target-update 2000, batch 32, 51 atoms, V in [-10, 10]);
--learn-start 1600 is that recipe's value and is NOT scaled down with the budget: the reference's stratified sampler
(memory.py:124-132) redraws until no sample lies in the last multi_step slots before the write head, and with fresh
transitions at the running max priority its last stratum lies entirely inside that zone — the loop never ends — unless
total priority / batch_size exceeds the priority mass of the last 21 slots, i.e. well over 32 * 21 = 672 transitions are
stored (a learn start of 400 spins forever on the first learn call).  Memory capacity = T_max rounded up to even.
One process per seed, one torch thread each (the nets are tiny: more threads only add synchronisation)."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "catch_learning.npz")
EVAL_SEED = 777_001
EVAL_EPISODES = 200
RANDOM_EPISODES = 20_000
PASS_FLOOR = 0.8


def options(t_max):
    return dict(architecture="data-efficient", hidden_size=256, multi_step=20, learning_rate=1e-4, replay_frequency=1,
                target_update=2000, batch_size=32, atoms=51, V_min=-10.0, V_max=10.0, history_length=4, noisy_std=0.1,
                discount=0.99, priority_exponent=0.5, priority_weight=0.4, adam_eps=1.5e-4, norm_clip=10.0, reward_clip=1,
                learn_start=1600, memory_capacity=t_max + (t_max & 1), T_max=t_max)


def _imports(reference):
    for p in (os.path.join(ROOT, "tests"), reference):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    torch.set_num_threads(1)
    import agent as ref_agent
    import memory as ref_memory
    import catch_oracle
    return torch, ref_agent, ref_memory, catch_oracle


def evaluate(torch, dqn, catch_oracle, history, episodes=EVAL_EPISODES, seed=EVAL_SEED):
    """Mean return of `episodes` episodes in eval() mode on a fresh environment with the fixed evaluation seed."""
    env = catch_oracle.CatchEnv(seed, history)
    dqn.eval()
    total = 0.0
    for _ in range(episodes):
        state, done = env.reset(), False
        while not done:
            state, reward, done = env.step(dqn.act(state))
            total += reward
    dqn.train()
    return total / episodes


def run_seed(job):
    reference, seed, t_max, t_eval = job
    torch, ref_agent, ref_memory, catch_oracle = _imports(reference)
    opt = options(t_max)
    args = types.SimpleNamespace(device=torch.device("cpu"), model=None, **opt)
    np.random.seed(seed)                                      # main.py:70-71
    torch.manual_seed(np.random.randint(1, 10000))
    env = catch_oracle.CatchEnv(seed, args.history_length)
    dqn = ref_agent.Agent(args, env)
    losses = []

    class Memory(ref_memory.ReplayMemory):                    # (records the per-sample losses the agent hands back)
        def update_priorities(self, idxs, priorities):
            losses.append(float(np.mean(priorities)))
            super().update_priorities(idxs, priorities)

    mem = Memory(args, args.memory_capacity)
    increase = (1 - args.priority_weight) / (args.T_max - args.learn_start)
    curve, loss_curve = [], []
    dqn.train()
    done = True
    t0 = time.time()
    for T in range(1, args.T_max + 1):                        # main.py:146-184
        if done:
            state = env.reset()
        if T % args.replay_frequency == 0:
            dqn.reset_noise()
        action = dqn.act(state)
        next_state, reward, done = env.step(action)
        reward = max(min(reward, args.reward_clip), -args.reward_clip)
        mem.append(state, action, reward, done)
        if T >= args.learn_start:
            mem.priority_weight = min(mem.priority_weight + increase, 1)
            if T % args.replay_frequency == 0:
                dqn.learn(mem)
            if T % t_eval == 0:
                curve.append(evaluate(torch, dqn, catch_oracle, args.history_length))
                loss_curve.append(float(np.mean(losses)) if losses else float("nan"))
                losses.clear()
                print("seed %d  T %6d  eval %+.3f  loss %.4f  (%.0f s)" % (seed, T, curve[-1], loss_curve[-1], time.time() - t0),
                      flush=True)
            if T % args.target_update == 0:
                dqn.update_target_net()
        state = next_state
    return seed, curve, loss_curve


def random_policy(catch_oracle, episodes=RANDOM_EPISODES, seed=424_242):
    """Per-episode return of uniformly random actions: mean and standard deviation over `episodes` oracle episodes."""
    S = 50
    env = catch_oracle.CatchOracle(S, 1, seed)
    env.reset()
    rs = np.random.RandomState(seed)
    returns = []
    while len(returns) < episodes:
        _, rewards, terminals = env.step(rs.randint(0, catch_oracle.ACTIONS, S))
        returns += [float(r) for r in rewards[terminals]]
    returns = np.array(returns[:episodes])
    return float(returns.mean()), float(returns.std())


def pass_bar(random_mean, random_std, worst_final, episodes=256):
    """Midpoint between the random policy and the worst reference seed, never below random + 6 standard errors of an
    `episodes`-episode mean (tests/test_device_loop_gpu.py computes the same from the fixture)."""
    floor = random_mean + 6.0 * random_std / np.sqrt(episodes)
    return max(0.5 * (random_mean + worst_final), floor), floor


def time_pieces(reference):
    torch, ref_agent, ref_memory, catch_oracle = _imports(reference)
    opt = options(2000)
    args = types.SimpleNamespace(device=torch.device("cpu"), model=None, **opt)
    env = catch_oracle.CatchEnv(1, 4)
    dqn = ref_agent.Agent(args, env)
    mem = ref_memory.ReplayMemory(args, args.memory_capacity)
    state = env.reset()

    def timed(name, fn, n):
        t0 = time.time()
        for _ in range(n):
            fn()
        print("%-12s %8.3f ms" % (name, (time.time() - t0) / n * 1e3), flush=True)

    def step():
        nonlocal state
        nxt, r, d = env.step(np.random.randint(0, 3))
        mem.append(state, 0, r, d)
        state = env.reset() if d else nxt

    timed("act", lambda: dqn.act(state), 200)
    timed("reset_noise", dqn.reset_noise, 200)
    timed("env+append", step, 1700)       # (past the learn start: see the module docstring)
    timed("learn", lambda: dqn.learn(mem), 50)
    print("torch threads", torch.get_num_threads())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("RAINBOW_REFERENCE"), help="checkout of the reference implementation")
    ap.add_argument("--t-max", type=int, default=3000)
    ap.add_argument("--t-eval", type=int, default=1000)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--explore", action="store_true", help="print the curves, write nothing")
    ap.add_argument("--time-pieces", action="store_true")
    a = ap.parse_args()
    if not a.reference or not os.path.isdir(a.reference):
        sys.exit("give the reference checkout with --reference PATH (or RAINBOW_REFERENCE)")
    if a.time_pieces:
        return time_pieces(a.reference)
    assert a.seeds >= 3 and a.t_max % 1000 == 0
    seeds = [101 + 7 * k for k in range(a.seeds)]
    with mp.get_context("spawn").Pool(len(seeds)) as pool:
        results = pool.map(run_seed, [(a.reference, s, a.t_max, a.t_eval) for s in seeds])
    _, _, _, catch_oracle = _imports(a.reference)
    rmean, rstd = random_policy(catch_oracle)
    evals = np.array([r[1] for r in results], dtype=np.float64)
    losses = np.array([r[2] for r in results], dtype=np.float64)
    worst = float(evals[:, -1].min())
    bar, floor = pass_bar(rmean, rstd, worst)
    print("random policy %.4f +- %.4f per episode; final evals %s; worst %.3f; bar %.4f (floor %.4f)"
          % (rmean, rstd, np.round(evals[:, -1], 3), worst, bar, floor))
    if a.explore:
        return
    assert worst >= PASS_FLOOR, "a reference seed ends below %.1f: raise --t-max" % PASS_FLOOR
    assert np.all(evals[:, -1] >= bar)
    np.savez(OUT, seeds=np.array(seeds), checkpoints=np.arange(a.t_eval, a.t_max + 1, a.t_eval), eval_return=evals,
             mean_loss=losses, random_mean=rmean, random_std=rstd, random_episodes=RANDOM_EPISODES, eval_episodes=EVAL_EPISODES,
             eval_seed=EVAL_SEED, options=json.dumps(options(a.t_max)))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
