"""The per-row-noise act path on the MI355X: the host-interpreter checks of test_noise_rows_emu.py on the device, the BASELINE
cfg-2 network at 64 and 100 rows (the second past the learner's 3 * batch rows: the forward buffers regrow), the generator's
statistics over 10^6 values, and the Python surface: Agent.reset_noise_rows, Agent.act_batch(per_row_noise=True),
train_device(per_stream_noise=True).  There is no learning check here: whether independent noise helps learning on Catch is
a question for profiles/, not for the suite."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import noise_rows_scenarios as NR
from cabi_adapter import TorchMem
from oracle import learner_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


def _ctx(hip, name, n_max):
    c = NR.RowsContext(hip, TorchMem(), name, n_max)
    yield c
    c.close()


@pytest.fixture(scope="module")
def k10(hip):
    yield from _ctx(hip, "k10", 33)


@pytest.fixture(scope="module")
def canon(hip):
    yield from _ctx(hip, "canon", 17)


@pytest.fixture(scope="module")
def atoms21(hip):
    yield from _ctx(hip, "atoms21", 3)


@pytest.fixture(scope="module")
def cfg2(hip):
    yield from _ctx(hip, NR.CFG2, 100)


# ------------------------------------------------------------------ the emulator's checks on the device
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33])
def test_rows_parity_k10_on_device(k10, n):
    NR.check_parity(k10, n)


@pytest.mark.parametrize("n", [5, 17])
def test_rows_parity_canon_on_device(canon, n):
    NR.check_parity(canon, n)


def test_rows_parity_atoms21_fallback_on_device(atoms21):
    NR.check_parity(atoms21, 3)


@pytest.mark.parametrize("n", [64, 100])
def test_rows_parity_at_the_baseline_cfg2_shape(cfg2, n):
    """H = 512, A = 6, batch 32: 64 rows fit the learner's 96-row forward buffers, 100 rows make them regrow."""
    NR.check_parity(cfg2, n)


@pytest.mark.parametrize("n", [1, 17])
def test_rows_consistent_with_the_shared_noise_path_on_device(k10, n):
    NR.check_consistency(k10, n)


def test_rows_consistent_with_the_shared_noise_path_at_cfg2(cfg2):
    NR.check_consistency(cfg2, 64)


def test_rows_consistent_with_the_shared_noise_path_fallback_on_device(atoms21):
    NR.check_consistency(atoms21, 3)


def test_rows_locality_on_device(k10):
    NR.check_locality(k10, 33, 16)


def test_rows_locality_at_cfg2(cfg2):
    NR.check_locality(cfg2, 33, 16)


def test_rows_locality_fallback_on_device(atoms21):
    NR.check_locality(atoms21, 3, 1)


def test_noise_rows_generator_on_device(k10):
    NR.check_generator(k10)


def test_noise_rows_generator_statistics(cfg2):
    NR.check_generator_statistics(cfg2, 128)


@pytest.mark.parametrize("shape", ["k10", "canon", "atoms21"])
def test_noise_rows_injected_normals_are_make_noise_on_device(shape, request):
    NR.check_injected_normals(request.getfixturevalue(shape))


def test_rows_refusals_on_device(k10):
    NR.check_refusals(k10)


def test_rows_kernels_stay_inside_their_buffers_on_device():
    """The out-of-bounds write hunt (tests/noise_rows_guard_run.py: k10, atoms21, cfg-2 up to 256 rows) in a child process:
    RB_GUARD is read when the library first allocates."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "noise_rows_guard_run.py"), "hip"], env=dict(os.environ, RB_GUARD="1"),
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "guard run ok" in p.stdout, p.stdout[-3000:] + "\n" + p.stderr[-3000:]


# ------------------------------------------------------------------ the Python surface
def _args(**kw):
    base = dict(device=torch.device(DEV), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=8, norm_clip=10.0, model=None,
                learning_rate=1e-4, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=32, noisy_std=0.1,
                replay_frequency=4, target_update=500, learn_start=3200, reward_clip=1)
    base.update(kw)
    return types.SimpleNamespace(**base)


N_AGENT = 40                     # batch_size 8: act_batch's chunks are 16 + 16 + 8


@pytest.fixture(scope="module")
def agent_case(hip):
    """An Agent with the k10 network (3 actions) and eval_learner-style parameters, 40 states, 40 blocks of normals and the
    per-row oracle."""
    from rainbow_amd.agent import Agent
    torch.manual_seed(3)
    np.random.seed(3)
    agent = Agent(_args(), types.SimpleNamespace(action_space=lambda: 3))
    seed = NR.pick_noise_seed("k10", N_AGENT)
    ora = NR.oracle_rows("k10", N_AGENT, seed)
    cfg = O.Config(**NR.shape_of("k10"))
    params = NR.scaled_params(cfg)
    with torch.no_grad():
        for name, off, shape in agent._layout:
            agent._params[off:off + int(np.prod(shape))].copy_(torch.from_numpy(np.ascontiguousarray(params[name]).ravel()))
    states = torch.from_numpy(NR.varied_states(N_AGENT, cfg.history)).to(DEV)
    raw = torch.from_numpy(NR.raw_normals(seed, N_AGENT, O.noise_draw_count(cfg))).to(DEV)
    torch.cuda.synchronize()
    return agent, states, raw, ora


@pytest.mark.parametrize("device_out", [False, True])
def test_agent_act_batch_per_row_noise_matches_the_oracle(agent_case, device_out):
    agent, states, raw, ora = agent_case
    agent.train()
    assert ora["margin"].min() >= NR.MIN_MARGIN and (ora["a"] != ora["a_shared"]).any()
    agent.reset_noise_rows(N_AGENT, raw_normals=raw)
    got = agent.act_batch(states, device_out=device_out, per_row_noise=True)
    if device_out:
        assert got.dtype == torch.int32 and got.device.type == "cuda"
        got = got.cpu().numpy()
    else:
        assert got.dtype == np.int64
    assert np.array_equal(got, ora["a"])
    # the chunking does not carry the result: the tail alone, with its row offset
    tail = agent.act_batch(states[16:], per_row_noise=True, row0=16)
    assert np.array_equal(tail, ora["a"][16:])


def test_agent_eval_mode_ignores_the_flag(agent_case):
    agent, states, raw, _ = agent_case
    agent.reset_noise_rows(N_AGENT, raw_normals=raw)
    agent.eval()
    try:
        plain = agent.act_batch(states, device_out=True)
        flagged = agent.act_batch(states, device_out=True, per_row_noise=True)
        assert torch.equal(plain, flagged)
        assert np.array_equal(agent.act_batch(states), agent.act_batch(states, per_row_noise=True))
    finally:
        agent.train()


def test_agent_per_row_noise_value_errors(agent_case):
    agent, states, raw, _ = agent_case
    agent.train()
    agent.reset_noise_rows(8, rng=(1, 2))
    with pytest.raises(ValueError, match="epsilon"):
        agent.act_batch(states[:8], epsilon=0.1, per_row_noise=True)
    with pytest.raises(ValueError, match="noise rows"):
        agent.act_batch(states[:9], per_row_noise=True)
    with pytest.raises(ValueError, match="noise rows"):
        agent.act_batch(states[:8], per_row_noise=True, row0=1)
    with pytest.raises(ValueError, match="rows"):
        agent.reset_noise_rows(0)
    with pytest.raises(ValueError, match="raw_normals"):
        agent.reset_noise_rows(8, raw_normals=raw[:7])
    assert agent.act_batch(states[:8], per_row_noise=True).shape == (8,)
    # the same (seed, round) redraws the same rows; the rows are the agent's own tensor, regrown when rows grows
    first = agent._noise_rows[:8].clone()
    agent.reset_noise_rows(8, rng=(1, 2))
    assert torch.equal(first, agent._noise_rows[:8])
    agent.reset_noise_rows(8, rng=(1, 3))
    assert not torch.equal(first, agent._noise_rows[:8])


def _run_train(seed, T_max, sync_debug=False, **loop_kw):
    from rainbow_amd.agent import Agent
    from rainbow_amd.envs import CatchVec
    from rainbow_amd.loop import train_device
    from rainbow_amd.memory import ReplayMemory
    S = 4
    # batch 4, multi_step 3: more than 4 * (3 + 1) * S = 64 transitions must be stored before the first draw can succeed
    args = _args(batch_size=4, learn_start=120, seed=77)
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = CatchVec(S, args.device, seed=seed, history_length=args.history_length)
    agent = Agent(args, env)
    mem = ReplayMemory(args, S * 100, seed=seed, streams=S)
    if sync_debug:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        learns = train_device(agent, mem, env, args, T_max, **loop_kw)
    finally:
        if sync_debug:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = dict(params=agent.params.detach().cpu().numpy().copy(), learns=learns, failed=mem.failed_samples(),
               cols={k: mem._grab(k) for k in ("tree", "timestep", "action", "reward", "nonterminal")})
    env.close()
    return out


def _same_run(a, b):
    return (a["learns"] == b["learns"] and np.array_equal(a["params"], b["params"])
            and all(np.array_equal(a["cols"][k], b["cols"][k]) for k in a["cols"]))


def test_train_device_per_stream_noise_is_deterministic_and_never_synchronises():
    """S = 4, 50 rounds, the k10-sized network: two runs with per_stream_noise=True from one seed end with bit-identical
    parameters and replay columns, a third under torch's sync debug mode ("error") raises nothing and ends the same; the flag
    off is the run without the argument, and the flag changes the run (other actions are stored)."""
    T_max = 4 * 50
    a, b = _run_train(9, T_max, per_stream_noise=True), _run_train(9, T_max, per_stream_noise=True)
    assert a["learns"] == sum(1 for T in range(1, T_max + 1, 4) if T >= 120) and a["failed"] == 0
    assert _same_run(a, b)
    c = _run_train(9, T_max, sync_debug=True, per_stream_noise=True)
    assert _same_run(a, c)
    off, plain = _run_train(9, T_max, per_stream_noise=False), _run_train(9, T_max)
    assert _same_run(off, plain)
    assert not np.array_equal(a["params"], plain["params"])
