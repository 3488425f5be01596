"""The reference's training loop (main.py:146-184) for S environment streams that live on the device.

A round is launches on one stream and nothing else: Agent.act_batch(device_out=True) -> env.step_device ->
ReplayMemory.append_streams with device operands -> Agent.learn.  Actions, rewards, nonterminals and the per-stream episode
timesteps never reach the host, and no call in a round synchronises (Agent.learn reports a sampler that found no batch one
call late, from pinned memory).  `env` is a rainbow_amd.envs environment (CatchVec) with as many streams as `mem`."""
import torch


def train_device(agent, mem, env, args, T_max, on_eval=None):
    """main.py:146-184 for S = env.streams device streams: T counts environment steps, S per round;
    reset_noise once per replay_frequency env steps; from learn_start on, beta is annealed by priority_weight_increase * S per
    round, one learn() per replay_frequency env steps (learn_owed), target update and evaluation at `T % k < S`.
    on_eval(T), if given, is called at the evaluation rounds (args.evaluation_interval); it may synchronise.
    Returns the number of learn() calls made."""
    S = env.streams
    if S != mem.streams:
        raise ValueError("train_device: the environment has %d streams, the memory %d" % (S, mem.streams))
    increase = (1 - args.priority_weight) / (T_max - args.learn_start)           # main.py:123
    clip = float(getattr(args, "reward_clip", 0) or 0)
    lo, hi = getattr(env, "reward_range", (-float("inf"), float("inf")))
    clip_needed = clip > 0 and (lo < -clip or hi > clip)
    eval_every = int(getattr(args, "evaluation_interval", 0) or 0)
    agent.train()
    states = env.reset()
    if S == 1:
        states = states.unsqueeze(0)
    learn_owed, learns = 0.0, 0
    for T in range(1, T_max + 1, S):
        if T % args.replay_frequency < S:
            agent.reset_noise()                                                   # main.py:150-151
        actions = agent.act_batch(states, device_out=True)                        # main.py:153, all streams, stays on the device
        next_states, rewards, nonterminals = env.step_device(actions)             # main.py:154 (ended streams: their reset stack)
        if clip_needed:
            rewards = rewards.clamp(-clip, clip)                                  # main.py:155-156
        mem.append_streams(states, actions, rewards, nonterminals=nonterminals)   # main.py:157
        if T >= args.learn_start:
            mem.priority_weight = min(mem.priority_weight + increase * S, 1)      # main.py:161
            learn_owed += S / args.replay_frequency
            while learn_owed >= 1:
                agent.learn(mem)                                                  # main.py:164
                learn_owed -= 1
                learns += 1
            if on_eval is not None and eval_every and T % eval_every < S:         # main.py:166-170
                on_eval(T)
                agent.train()
            if T % args.target_update < S:
                agent.update_target_net()                                         # main.py:177-178
        states = next_states
    return learns


def evaluate_device(agent, env, episodes):
    """Mean episode return of the agent in eval() mode (test.py's loop without epsilon) on `env` — a fresh environment with
    its own seed — over at least `episodes` finished episodes, read from the totals the environment keeps on the device.
    The episode count is polled (one synchronisation) every 11 rounds; the agent is left in the mode it came in."""
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
