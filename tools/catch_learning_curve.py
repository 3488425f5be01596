"""Learning curves of the device agent on the device Catch environment (a measurement, not a test): rainbow_amd with production
randomness (device Philox sampler and noise, lazy reset_noise, deferred optimiser pass, beta annealing, target syncs — all
defaults) through rainbow_amd.loop.train_device, with the options tests/golden/make_golden_catch.py gives the reference.
Every --t-eval env steps the agent is evaluated in eval() mode over 256 episodes on a fresh environment with a fixed seed.
One line per checkpoint; `--no-learn` runs the same loop with learn() skipped (what an agent that does not learn scores).
`--protocol vec` evaluates with rainbow_amd.loop.evaluate_vec instead (test.py's protocol: epsilon 0.001, 256 episodes spread
evenly over the streams); the default, `device`, is evaluate_device as before.
`--env breakout` runs the same on the device Breakout environment (training: a lost life is a terminal; evaluation: whole
games, unclipped returns), same output format.  `--multi-step` / `--learn-start` override the recipe's 20 / 1600: with them the
stratified draw needs more than batch_size * (multi_step + 1) * S stored transitions, and its last stratum must not fall inside
the multi_step newest slots, which all carry the running max priority (Agent.learn raises; the line then ends in STOPPED).
`--augment-pad P` turns the replay's random-shift augmentation on (ReplayMemory augment_pad: sampled stacks shifted by up to P
pixels, the learn step on the gathered path).  `--target-tau TAU` gives the agent an EMA target (Agent target_tau: the target follows
every optimiser step inside the clip + Adam pass, and the loop makes no hard target syncs).  `--replay-ratio R` makes R learn steps
per environment step (args.replay_ratio; the recipe's replay_frequency = 1 is ratio 1) and `--reset-interval N` shrinks and perturbs
the networks every N GRADIENT steps (args.reset_interval: Agent.reset_parameters with its defaults, encoder 0.5 / head 0); the line
then carries both and the number of resets done.
`--stats` keeps the device's per-step records (args.step_stats, rainbow_amd/agent_stats.py) and reads them every --log-interval learn
steps (train_device's on_log): each checkpoint then also shows the means since the checkpoint before it of the loss, the online value
q, the |target - online| value gap td and the gradient norm g — why a curve moves or does not, not only whether it does.
`--redo N` recycles the dormant units every N GRADIENT steps (args.redo_interval: Agent.recycle_dormant, rainbow_amd/agent_redo.py, tau
0.1, one batch); the line then carries the number of recycles done, and each checkpoint the dormant share `dorm` the last recycle
found — beside the `--stats` columns when those are on.
`--rank N` measures the rank of the hidden features every N GRADIENT steps (args.rank_interval: Agent.feature_rank,
rainbow_amd/agent_rank.py, 8 batches; it synchronises); each checkpoint then shows the last measurement as `srank` / its feature
rank / its effective rank, beside the `--stats` and `--redo` columns."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EVAL_SEED = 777_001


def options(t_max, dev, multi_step=20, learn_start=1600, augment_pad=0, target_tau=0.0, replay_ratio=0.0, reset_interval=0):
    return types.SimpleNamespace(
        augment_pad=augment_pad, target_tau=target_tau, replay_ratio=replay_ratio, reset_interval=reset_interval,
        device=dev, architecture="data-efficient", hidden_size=256, multi_step=multi_step, learning_rate=1e-4, replay_frequency=1,
        target_update=2000, batch_size=32, atoms=51, V_min=-10.0, V_max=10.0, history_length=4, noisy_std=0.1, discount=0.99,
        priority_exponent=0.5, priority_weight=0.4, adam_eps=1.5e-4, norm_clip=10.0, reward_clip=1, learn_start=learn_start,
        model=None, T_max=t_max)


def run(S, seed, t_max, t_eval, learn, dev, protocol="device", game="catch", multi_step=20, learn_start=1600, augment_pad=0,
        target_tau=0.0, replay_ratio=0.0, reset_interval=0, stats=False, log_interval=200, redo=0, rank=0):
    from rainbow_amd.agent import Agent
    from rainbow_amd.envs import BreakoutVec, CatchVec
    from rainbow_amd.loop import evaluate_device, evaluate_vec, train_device
    from rainbow_amd.memory import ReplayMemory
    make = {"catch": CatchVec, "breakout": BreakoutVec}[game]
    args = options(t_max, dev, multi_step, learn_start, augment_pad, target_tau, replay_ratio, reset_interval)
    args.evaluation_interval = t_eval
    args.seed = seed
    if stats and learn:
        args.step_stats, args.log_interval = 4 * log_interval, log_interval
    if redo and learn:
        args.redo_interval = redo
    if rank and learn:
        args.rank_interval = rank
    np.random.seed(seed)
    torch.manual_seed(np.random.randint(1, 10000))
    env = make(S, dev, seed=seed)
    agent = Agent(args, env)
    cap = -(-t_max // (2 * S)) * 2 * S
    mem = ReplayMemory(args, cap, seed=seed, streams=S)
    if not learn:
        agent.learn = lambda mem: None
    curve = []
    seen = {k: [] for k in ("loss_mean", "q_mean", "td_abs_mean", "grad_norm")}      # the records since the last checkpoint
    dropped = [0]

    def on_log(T, records):
        for k in seen:                                                           # (with --redo the records also carry dormant_fraction)
            seen[k].append(records[k])
        dropped[0] += records["dropped"]

    def stats_columns():
        dorm = agent.dormant_fraction() if redo and learn else None              # (reads the last recycle's counts: on_eval may synchronise)
        fr = agent.last_feature_rank if rank and learn else None                 # (the last measurement's dict: host values)
        return (stats_only() + ("[dorm %.3f]" % dorm if dorm is not None else "")
                + ("[srank %d rank %d erank %.1f]" % (fr["srank"], fr["feature_rank"], fr["effective_rank"])
                   if fr is not None and fr["finite"] else ""))

    def stats_only():
        if not (stats and learn) or not seen["loss_mean"]:
            return ""
        m = {k: float(np.nanmean(np.concatenate(v))) for k, v in seen.items()}
        for v in seen.values():
            del v[:]
        return "[loss %.3f q %+.3f td %.3f g %.2f]" % (m["loss_mean"], m["q_mean"], m["td_abs_mean"], m["grad_norm"])

    def on_eval(T):
        ev = make(16, dev, seed=EVAL_SEED)
        ev.eval()
        if protocol == "vec":
            curve.append((T, evaluate_vec(agent, ev, 256, seed=T)["avg_reward"], stats_columns()))
        else:
            curve.append((T, evaluate_device(agent, ev, 256), stats_columns()))
        ev.close()

    t0 = time.perf_counter()
    try:
        train_device(agent, mem, env, args, t_max, on_eval=on_eval, on_log=on_log if stats and learn else None)
        note = ""
    except RuntimeError as e:
        note = "  STOPPED: " + str(e)[:150]
    torch.cuda.synchronize()
    tag = "learn" if learn else "NO-LEARN"
    if replay_ratio or reset_interval:
        tag += " replay-ratio %g reset-interval %d (%d resets)" % (replay_ratio or 1.0, reset_interval, agent.resets)
    if redo and learn:
        tag += " redo-interval %d (%d recycles)" % (redo, agent.recycles)
    print("S %2d seed %3d %s (%.1f s): " % (S, seed, tag, time.perf_counter() - t0)
          + " ".join("%d:%+.3f%s" % c for c in curve) + ("  (%d records dropped)" % dropped[0] if dropped[0] else "") + "  training-episode mean %+.3f" % env.stats()["mean_return"] + note,
          flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t-max", type=int, default=20000)
    ap.add_argument("--t-eval", type=int, default=2000)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--no-learn", action="store_true")
    ap.add_argument("--protocol", choices=["device", "vec"], default="device")
    ap.add_argument("--env", choices=["catch", "breakout"], default="catch")
    ap.add_argument("--multi-step", type=int, default=20)
    ap.add_argument("--learn-start", type=int, default=1600)
    ap.add_argument("--augment-pad", type=int, default=0)
    ap.add_argument("--target-tau", type=float, default=0.0)
    ap.add_argument("--replay-ratio", type=float, default=0.0)
    ap.add_argument("--reset-interval", type=int, default=0)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--log-interval", type=int, default=200)
    ap.add_argument("--redo", type=int, default=0, metavar="N")
    ap.add_argument("--rank", type=int, default=0, metavar="N")
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    dev = torch.device("cuda", 0)
    for S in a.streams:
        for k in range(a.seeds if S == 1 else min(3, a.seeds)):
            run(S, 101 + 7 * k, a.t_max, a.t_eval, not a.no_learn, dev, a.protocol, a.env, a.multi_step, a.learn_start, a.augment_pad,
                a.target_tau, a.replay_ratio, a.reset_interval, a.stats, a.log_interval, a.redo, a.rank)


if __name__ == "__main__":
    main()
