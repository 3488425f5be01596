"""The reference's training loop (main.py:146-184) for S environment streams that live on the device.

A round is launches on one stream and nothing else: Agent.act_batch(device_out=True) -> env.step_device ->
ReplayMemory.append_streams with device operands -> Agent.learn.  Actions, rewards, nonterminals and the per-stream episode
timesteps never reach the host, and no call in a round synchronises (Agent.learn reports a sampler that found no batch one
call late, from pinned memory).  `env` is a rainbow_amd.envs environment (CatchVec, BreakoutVec) with as many streams as `mem`.
An environment with lives (BreakoutVec in training mode) reports a lost life as nonterminals == 0 while its next stack is the
old one moved on, not a reset stack (env.py:70-75); the loop needs to know nothing about it.

`train_host_vec` is the same loop for S raw HOST emulators (ALE) behind a rainbow_amd.frames.FrameStackVec: the emulators write
their u8 screens into the front end's pinned staging, one upload and one launch per round build all S frame stacks.

`evaluate_vec` / `evaluate_host_vec` are the reference's evaluation (test.py:13-41) for the same two kinds of environment:
epsilon-greedy actions drawn in the batched act path, the per-episode list of returns, `episodes` spread evenly over the streams."""
import math
from contextlib import contextmanager

import numpy as np
import torch

from .evaluate import EpisodeTally, stream_quotas


def horizon_at(t, n0, n1, g0, g1, T):
    """BBF's annealed update horizon and discount, a pure function: t gradient steps after the last reset (or the start) the
    horizon has moved geometrically from n0 towards n1 and 1 - gamma geometrically from 1 - g0 towards 1 - g1, both reaching their
    end at t = T and staying there.  With f = min(t, T) / T:  n = floor(n0 * (n1 / n0) ** f + 0.5),
    gamma = 1 - (1 - g0) * ((1 - g1) / (1 - g0)) ** f.  (BBF: 10 -> 3 and 0.97 -> 0.997 over T = 10 000.)  Returns (n, gamma)."""
    f = (min(t, T) / T) if T > 0 else 1.0
    n = int(math.floor(n0 * (n1 / n0) ** f + 0.5))
    if g1 == g0:
        return n, float(g0)                                                       # (no rounding of 1 - (1 - g0))
    if not (g0 < 1 and g1 < 1):
        raise ValueError("horizon_at: 1 - gamma is interpolated geometrically, so both discounts must be below 1")
    return n, 1 - (1 - g0) * ((1 - g1) / (1 - g0)) ** f


def _train_rounds(agent, mem, S, args, T_max, on_eval, per_stream_noise, states, round_fn, on_log=None):
    """The cadence of main.py:146-184 at S environment steps per round, shared by train_device and train_host_vec:
    round_fn(states) acts, steps the environment and appends the round to `mem`, and returns the next states.
    args.multi_step_final (absent: no schedule, set_horizon is never called) anneals the horizon from args.multi_step and, with
    args.discount_final, the discount from args.discount (horizon_at) over args.horizon_anneal_steps (10 000) gradient steps counted
    from the start or the last reset: agent and memory are set before the first learn step, before every learn step whose count t is
    a multiple of args.horizon_update_interval (100) up to the end of the anneal, at t = horizon_anneal_steps, and right after each
    agent.reset_parameters(), which restarts t at 0.
    on_log (None: nothing is read, nothing changes): called as on_log(T, agent.read_stats()) right after every learn step whose
    count is a multiple of args.log_interval (in learn steps; absent or 0: never) — the records of the steps since the last call
    (Agent.track_stats / args.step_stats; None when the agent keeps none).  read_stats synchronises; the steps in between do not.
    args.redo_interval (absent or 0: never, no call is made) counts gradient steps like reset_interval: right after the learn step
    that makes the count a multiple of it, agent.recycle_dormant(mem, tau=args.redo_tau, batches=args.redo_batches (1),
    target=args.redo_target (False)) recycles the dormant units; where a full reset falls on the same step the reset runs and the
    recycle is skipped.  With redo_interval in use the records handed to on_log gain `dormant_fraction`, the share the last
    recycle found (None before the first), read at log time, where the loop synchronises anyway.
    args.rank_interval (absent or 0: never, no call is made) counts gradient steps too: right after the learn step that makes the
    count a multiple of it — before on_log, and before a reset or a recycle that falls on the same step, whose need it is there to
    show — agent.feature_rank(mem, batches=args.rank_batches (8), layer=args.rank_layer ("hidden")) measures the rank of the
    features.  It SYNCHRONISES (it copies the Gram matrix to the host and takes its eigenvalues there): keep the interval in the
    thousands.  With rank_interval in use on_log's records gain `srank`, `feature_rank` and `effective_rank` of the last
    measurement (None before the first)."""
    seed = int(getattr(args, "seed", 0))
    increase = (1 - args.priority_weight) / (T_max - args.learn_start)           # main.py:123
    eval_every = int(getattr(args, "evaluation_interval", 0) or 0)
    replay_ratio = float(getattr(args, "replay_ratio", 0) or 0)                   # learn steps per environment step; may exceed 1
    reset_interval = int(getattr(args, "reset_interval", 0) or 0)                 # in GRADIENT steps; 0 = never
    redo_interval = int(getattr(args, "redo_interval", 0) or 0)                   # in GRADIENT steps; 0 = never
    redo_kw = dict(tau=getattr(args, "redo_tau", None), batches=int(getattr(args, "redo_batches", 1) or 1),
                   target=bool(getattr(args, "redo_target", False)))
    rank_interval = int(getattr(args, "rank_interval", 0) or 0)                   # in GRADIENT steps; 0 = never
    rank_kw = dict(batches=int(getattr(args, "rank_batches", 8) or 8), layer=getattr(args, "rank_layer", None) or "hidden")
    rank_last = None
    learn_owed, learns = 0.0, 0
    log_interval = int(getattr(args, "log_interval", 0) or 0) if on_log is not None else 0
    n1 = getattr(args, "multi_step_final", None)
    set_horizon = None
    if n1 is not None:
        n0, n1, g0 = int(args.multi_step), int(n1), float(args.discount)
        if n1 > n0:
            raise ValueError("multi_step_final (%d) must not exceed multi_step (%d): the horizon anneals downwards" % (n1, n0))
        g1 = getattr(args, "discount_final", None)
        g1 = g0 if g1 is None else float(g1)
        anneal = int(getattr(args, "horizon_anneal_steps", 10000))
        interval = max(1, int(getattr(args, "horizon_update_interval", 100)))

        def set_horizon(t):
            n, g = horizon_at(t, n0, n1, g0, g1, anneal)
            agent.set_horizon(n, g)
            mem.set_horizon(n, g)
    since_reset, horizon_set_at = 0, None         # gradient steps since the last reset; the count the horizon was last set for
    if per_stream_noise:
        agent.reset_noise_rows(S, rng=(seed, 0))                                  # S < replay_frequency: the first rounds come before the first redraw
    for T in range(1, T_max + 1, S):
        if T % args.replay_frequency < S:
            agent.reset_noise()                                                   # main.py:150-151
            if per_stream_noise:
                agent.reset_noise_rows(S, rng=(seed, T))
        states = round_fn(states)                                                 # main.py:153-157
        if T >= args.learn_start:
            mem.priority_weight = min(mem.priority_weight + increase * S, 1)      # main.py:161
            learn_owed += S * replay_ratio if replay_ratio > 0 else S / args.replay_frequency
            while learn_owed >= 1:
                if (set_horizon is not None and since_reset != horizon_set_at and since_reset <= anneal
                        and (since_reset % interval == 0 or since_reset == anneal)):
                    set_horizon(since_reset)
                    horizon_set_at = since_reset
                agent.learn(mem)                                                  # main.py:164
                learn_owed -= 1
                learns += 1
                since_reset += 1
                if rank_interval and learns % rank_interval == 0:
                    rank_last = agent.feature_rank(mem, **rank_kw)                # srank & co (Agent.feature_rank); synchronises
                if log_interval and learns % log_interval == 0:
                    records = agent.read_stats()
                    if redo_interval:
                        records = dict(records or {}, dormant_fraction=agent.dormant_fraction())
                    if rank_interval:
                        records = dict(records or {}, **{k: None if rank_last is None else rank_last[k]
                                                         for k in ("srank", "feature_rank", "effective_rank")})
                    on_log(T, records)
                if reset_interval and learns % reset_interval == 0:
                    agent.reset_parameters()                                      # shrink-and-perturb (Agent.reset_parameters)
                    since_reset = 0
                    if set_horizon is not None:
                        set_horizon(0)                                            # the anneal starts again with the reset
                        horizon_set_at = 0
                elif redo_interval and learns % redo_interval == 0:
                    agent.recycle_dormant(mem, **redo_kw)                         # ReDo (Agent.recycle_dormant)
            if on_eval is not None and eval_every and T % eval_every < S:         # main.py:166-170
                on_eval(T)
                agent.train()
            if T % args.target_update < S and not float(getattr(agent, "target_tau", 0.0)) > 0:
                agent.update_target_net()                                         # main.py:177-178 (an EMA target follows every step instead)
    return learns


def train_device(agent, mem, env, args, T_max, on_eval=None, per_stream_noise=False, on_log=None):
    """main.py:146-184 for S = env.streams device streams: T counts environment steps, S per round;
    reset_noise once per replay_frequency env steps; from learn_start on, beta is annealed by priority_weight_increase * S per
    round, one learn() per replay_frequency env steps (learn_owed), target update and evaluation at `T % k < S`.
    With agent.target_tau > 0 (args.target_tau: the target follows every optimiser step by EMA) the periodic hard target update
    is skipped.
    args.replay_ratio (absent or 0: replay_frequency decides, as above): learn steps per environment step, a float that may exceed
    1 — S * replay_ratio learn steps are owed per round.  args.reset_interval (absent or 0: never) counts GRADIENT steps: right
    after the learn() that makes the count a multiple of it, agent.reset_parameters() shrinks and perturbs the networks
    (args.reset_shrink_encoder / reset_shrink_head) — what keeps a replay ratio above 1 from hurting.
    args.multi_step_final (absent: no schedule, no set_horizon call ever) anneals the update horizon from args.multi_step and,
    with args.discount_final, the discount from args.discount after the start and after every reset (horizon_at, _train_rounds;
    args.horizon_anneal_steps, args.horizon_update_interval): agent.set_horizon and mem.set_horizon, INTEGRATION.md §2.
    on_eval(T), if given, is called at the evaluation rounds (args.evaluation_interval); it may synchronise.
    per_stream_noise=True: every stream acts under its OWN noisy-net sample — agent.reset_noise_rows(S, rng=(args.seed, T)) at
    the cadence of reset_noise() (which stays: learn() needs the learner's own sample) and act_batch(per_row_noise=True);
    the default leaves today's launches exactly as they are (all S streams share the one online sample).
    on_log(T, records), if given, is called every args.log_interval LEARN steps with agent.read_stats(): the per-step records the
    device has written since the last call (args.step_stats / Agent.track_stats); it synchronises, nothing else in the loop does.
    Returns the number of learn() calls made."""
    S = env.streams
    if S != mem.streams:
        raise ValueError("train_device: the environment has %d streams, the memory %d" % (S, mem.streams))
    clip = float(getattr(args, "reward_clip", 0) or 0)
    lo, hi = getattr(env, "reward_range", (-float("inf"), float("inf")))
    clip_needed = clip > 0 and (lo < -clip or hi > clip)
    act_kw = dict(per_row_noise=True) if per_stream_noise else {}                 # (the default passes no per_row_noise at all)

    def round_fn(states):
        actions = agent.act_batch(states, device_out=True, **act_kw)              # main.py:153, all streams, stays on the device
        next_states, rewards, nonterminals = env.step_device(actions)             # main.py:154 (ended streams: their reset stack)
        if clip_needed:
            rewards = rewards.clamp(-clip, clip)                                  # main.py:155-156
        mem.append_streams(states, actions, rewards, nonterminals=nonterminals)   # main.py:157
        return next_states

    agent.train()
    states = env.reset()
    if S == 1:
        states = states.unsqueeze(0)
    return _train_rounds(agent, mem, S, args, T_max, on_eval, per_stream_noise, states, round_fn, on_log)


def train_host_vec(agent, mem, emus, front, args, T_max, on_eval=None, per_stream_noise=False, on_log=None):
    """main.py:146-184 for S = len(emus) raw host emulators behind `front`, a rainbow_amd.frames.FrameStackVec (INTEGRATION.md
    §2).  emus[s] is duck-typed:
        reset(out_a)                 starts the next game — or, after a step that reported life_lost, does env.py:36-38's
                                     single no-op instead — and writes the u8 [H, W] screen into out_a
        step(action, out_a, out_b)   env.py:54-75: repeats the action, writes the screens after frames 3 and 4 of the repeat
                                     into out_a / out_b as far as the repeat got, and returns (flags, reward, done, life_lost):
                                     flags = the FrameStackVec bits of the frames it wrote, done = the game is over,
                                     life_lost = a life was lost and the game goes on (env.py:70-75, training mode)
    A stream whose step ended its game is reset in the same round and its next stack is the RESET stack (env.py:40-52), as
    rainbow_amd.envs.CatchVec does; a stream that lost a life gets LIFE_RESET from the emulator's no-op screen.  Either way the
    transition is stored as terminal and the observation of the ending step itself is never stored by the replay (it is not
    in the reference either: memory.py:105-108 stores state[-1] of the state acted on).  One difference to env.py remains for
    the ACTOR: after a lost life env.py's deque also holds the ending step's observation below the no-op screen, here the
    stream's stack moves by one frame per round, so that frame is skipped.
    Cadences are train_device's: reset_noise once per replay_frequency env steps; from learn_start on, beta annealed by
    priority_weight_increase * S per round, one learn() per replay_frequency env steps (learn_owed) — or S * args.replay_ratio
    per round, with agent.reset_parameters() every args.reset_interval gradient steps, as in train_device — target update and
    on_eval at `T % k < S`; args.multi_step_final and its companions anneal the horizon as in train_device.  per_stream_noise: as in train_device (one noise sample per emulator); on_log and args.log_interval: as in train_device.
    Returns the number of learn() calls made."""
    S = len(emus)
    if S != mem.streams or S != front.streams:
        raise ValueError("train_host_vec: %d emulators, a front end of %d streams, a memory of %d" % (S, front.streams, mem.streams))
    clip = float(getattr(args, "reward_clip", 0) or 0)
    flags, rewards, terminals = np.zeros(S, dtype=np.uint8), np.zeros(S, dtype=np.float32), np.zeros(S, dtype=bool)

    def round_fn(states):
        actions = agent.act_batch(states, per_row_noise=per_stream_noise)         # main.py:153, one forward for all streams
        scr = front.screens
        for s in range(S):
            f, r, done, life_lost = emus[s].step(int(actions[s]), scr[s, 0], scr[s, 1])    # main.py:154
            if done or life_lost:                                                 # main.py:147-148, in the same round
                emus[s].reset(scr[s, 0])
                f = front.RESET if done else front.LIFE_RESET
            flags[s], rewards[s], terminals[s] = f, r, done or life_lost
        if clip > 0:
            np.clip(rewards, -clip, clip, out=rewards)                            # main.py:155-156
        next_states = front.step(flags)
        mem.append_streams(states, actions, rewards, terminals)                   # main.py:157
        return next_states

    agent.train()
    scr = front.screens
    for s in range(S):
        emus[s].reset(scr[s, 0])
    return _train_rounds(agent, mem, S, args, T_max, on_eval, per_stream_noise, front.reset_all(), round_fn, on_log)


def evaluate_device(agent, env, episodes):
    """Mean episode return of the agent in eval() mode (test.py's loop without epsilon) on `env` — a fresh environment with
    its own seed — over at least `episodes` finished episodes, read from the totals the environment keeps on the device.
    The episode count is polled (one synchronisation) every 11 rounds; the agent is left in the mode it came in.
    This is a quick mean for a game whose episodes all have one length; `evaluate_vec` is the test.py-faithful evaluation
    (epsilon-greedy, the per-episode list, an even share of the episodes per stream, any rainbow_amd.envs environment)."""
    was_training = agent.training
    agent.eval()
    S = env.streams
    states = env.reset()
    if S == 1:
        states = states.unsqueeze(0)
    env.reset_stats()
    while True:
        for _ in range(11):
            states, _, _ = env.step_device(agent.act_batch(states, device_out=True))
        st = env.stats()
        if st["episodes"] >= episodes:
            break
    if was_training:
        agent.train()
    return st["mean_return"]


def _evaluation_result(agent, returns, lengths, val_mem, with_loss=False):
    rewards = [float(x) for x in returns]                                         # test.py:33 T_rewards
    Qs = agent.evaluate_q_memory(val_mem) if val_mem is not None else None        # test.py:38-39
    out = dict(avg_reward=sum(rewards) / len(rewards), rewards=rewards, lengths=[int(x) for x in lengths],      # test.py:41
               avg_Q=float(sum(float(q) for q in Qs) / len(Qs)) if Qs is not None else None, Qs=Qs)
    if with_loss and val_mem is not None:         # the held-out loss and TD error (Agent.evaluate_loss): the overfitting signal
        ev = agent.evaluate_loss(val_mem)
        out["val_loss"], out["val_td_abs"] = ev["loss_mean"], ev["td_abs_mean"]
    return out


@contextmanager
def _eval_mode(agent):
    """agent.eval() for the block; the mode the agent came in is restored on the way out, also by an exception."""
    was_training = agent.training
    agent.eval()                                                                  # test.py:15 / main.py:168
    try:
        yield
    finally:
        if was_training:
            agent.train()


def _unfinished(who, missing, episodes, max_rounds):
    return RuntimeError("%s: %d of %d episodes still unfinished after max_rounds = %d rounds" % (who, missing, episodes, max_rounds))


def evaluate_vec(agent, env, episodes, epsilon=0.001, seed=0, val_mem=None, poll_every=8, max_rounds=None, with_loss=False):
    """test.py:13-41 on `env`, a rainbow_amd.envs environment of S streams with a seed of its own: the agent in eval() mode,
    act_e_greedy with `epsilon` for every stream (Agent.act_batch(epsilon=..., rng=(seed, round)): the draw happens in the head
    kernel), raw rewards, and the list of episode returns the reference calls T_rewards.  A round is act -> env.step_device ->
    EpisodeTally.step, launches only; the number of episodes still missing is polled (one synchronisation) every `poll_every`
    rounds.  Stream s contributes its first episodes // S + (s < episodes % S) episodes, so short episodes are not
    over-represented; the list is stream-major.  More than `max_rounds` rounds (None = no bound) raise RuntimeError.
    The caller hands over an environment in EVALUATION mode (test.py:17 builds its env and calls env.eval()): an episode is a
    whole game, so an environment with lives must not report a lost life as a terminal — BreakoutVec(training=False) or
    env.eval() before the call; a training-mode environment would have every life recorded as an episode.
    Returns dict(avg_reward, rewards, lengths, avg_Q, Qs): `rewards` has exactly `episodes` entries; Qs is
    agent.evaluate_q_memory(val_mem) (test.py:38-39) and avg_Q its mean when a validation memory is given, else None.
    with_loss=True (and a validation memory that is a rainbow_amd ReplayMemory): also val_loss / val_td_abs, the loss and the mean
    |target value - online value| of one batch drawn from it (Agent.evaluate_loss; it advances val_mem's draw state).
    The agent is left in the mode it came in."""
    S = env.streams
    poll_every = max(1, int(poll_every))
    with _eval_mode(agent):
        tally = EpisodeTally(S, episodes, env.device)
        states = env.reset()
        if S == 1:
            states = states.unsqueeze(0)
        rounds = 0
        while True:
            actions = agent.act_batch(states, device_out=True, epsilon=epsilon, rng=(seed, rounds))     # test.py:26
            states, rewards, nonterminals = env.step_device(actions)              # test.py:27
            tally.step(rewards, nonterminals)                                     # test.py:28,32-33
            rounds += 1
            last = max_rounds is not None and rounds >= max_rounds
            if rounds % poll_every == 0 or last:
                missing = tally.remaining()
                if missing == 0:
                    break
                if last:
                    raise _unfinished("evaluate_vec", missing, episodes, max_rounds)
        returns, lengths, _ = tally.result()
        tally.close()
        return _evaluation_result(agent, returns, lengths, val_mem, with_loss)


def evaluate_host_vec(agent, emus, front, episodes, epsilon=0.001, seed=0, val_mem=None, max_rounds=None, with_loss=False):
    """The same protocol for S = len(emus) raw host emulators behind `front`, a rainbow_amd.frames.FrameStackVec, duck-typed as
    in train_host_vec.  The emulators are the caller's EVALUATION ones: env.py's eval mode reports no life-loss terminals
    (env.py:70-75 is training only), so a step that reports life_lost raises ValueError.  A stream whose step ended its game
    is reset in the same round with front.RESET.  Rewards are host values here, so the tally rule of rb_tally_* (even quotas,
    f32 running return, the ending step's reward belongs to the ending episode, stream-major list) is kept in numpy.
    Returns what evaluate_vec returns (with_loss as there); more than `max_rounds` rounds raise RuntimeError."""
    S = len(emus)
    if S != front.streams:
        raise ValueError("evaluate_host_vec: %d emulators, a front end of %d streams" % (S, front.streams))
    quotas = stream_quotas(S, episodes)
    if not 1 <= int(episodes) <= 65536:
        raise ValueError("evaluate_host_vec: episodes must be in [1, 65536], got %d" % episodes)
    recorded = [[] for _ in range(S)]
    ret, length = np.zeros(S, dtype=np.float32), np.zeros(S, dtype=np.int64)
    flags = np.zeros(S, dtype=np.uint8)
    with _eval_mode(agent):
        scr = front.screens
        for s in range(S):
            emus[s].reset(scr[s, 0])
        states = front.reset_all()
        missing, rounds = int(episodes), 0
        while missing > 0:
            if max_rounds is not None and rounds >= max_rounds:
                raise _unfinished("evaluate_host_vec", missing, episodes, max_rounds)
            actions = agent.act_batch(states, epsilon=epsilon, rng=(seed, rounds))              # test.py:26
            scr = front.screens
            for s in range(S):
                f, r, done, life_lost = emus[s].step(int(actions[s]), scr[s, 0], scr[s, 1])     # test.py:27
                if life_lost:
                    raise ValueError("evaluate_host_vec: emulator %d reported a lost life as an episode end; evaluation "
                                     "needs emulators in evaluation mode (env.py:70-75 applies to training only)" % s)
                ret[s] = ret[s] + np.float32(r)                                                  # test.py:28, unclipped
                length[s] += 1
                if done:
                    if len(recorded[s]) < quotas[s]:
                        recorded[s].append((ret[s], length[s]))                                 # test.py:33
                        missing -= 1
                    ret[s], length[s] = 0.0, 0
                    emus[s].reset(scr[s, 0])                                                    # test.py:23-24, in the same round
                    f = front.RESET
                flags[s] = f
            states = front.step(flags)
            rounds += 1
        flat = [x for per_stream in recorded for x in per_stream]
        return _evaluation_result(agent, [x[0] for x in flat], [x[1] for x in flat], val_mem, with_loss)
