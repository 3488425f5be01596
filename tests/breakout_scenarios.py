"""Checks of the device Breakout environment (rb_breakout_*) shared by the host-interpreter tests (test_breakout_emu.py) and the
device tests (test_breakout_gpu.py): the same code drives either build through the C ABI; tests/breakout_oracle.py is the
oracle.  Equality means bit-identical stacks every round and equal rewards / nonterminals / totals.  The coverage asserts
(games ended, lives lost, bricks, reflections ...) are conditions on the ORACLE's run: the seeds were picked on the CPU so
that they hold."""
import ctypes as C

import numpy as np

import breakout_oracle as BO
import device_loop_scenarios as DS
from rainbow_amd import _lib as L

SCRIPTED_SEED = 4                 # seeds of the runs whose coverage asserts depend on them, picked on the oracle
ROUND_SEED_EMU, ROUND_SEED_GPU = 4, 4
STATE_FIELDS = [f for f, _ in L.BreakoutState._fields_]
SCALARS = [f for f in STATE_FIELDS if f not in ("rows", "reserved")]


# =============================================================================== the handle
class BreakoutHandle:
    """rb_breakout_* through the C ABI with two stack buffers swapped by the caller."""

    def __init__(self, lib, mem, S, history, max_steps, seed, life_terminals=1):
        self.lib, self.mem, self.S, self.history, self.life_terminals = lib, mem, S, history, life_terminals
        self.h = C.c_void_p()
        L.check(lib, lib.rb_breakout_create(C.byref(self.h), S, history, max_steps, seed))
        self.bufs = [mem.empty((S, history, 84, 84), np.float32) for _ in range(2)]
        self.cur = 0
        self.rewards = mem.empty((S,), np.float32)
        self.nonterminals = mem.empty((S,), np.uint8)

    def close(self):
        if self.h:
            self.lib.rb_breakout_destroy(self.h)
            self.h = None

    def stacks(self):
        return self.bufs[self.cur]

    def reset(self):
        L.check(self.lib, self.lib.rb_breakout_reset(self.h, self.mem.ptr(self.bufs[self.cur]), self.mem.stream))
        self.mem.sync()
        return self.mem.download(self.bufs[self.cur])

    def step_dev(self, actions_buf):
        """actions already on the device; no download"""
        m = self.mem
        L.check(self.lib, self.lib.rb_breakout_step(self.h, m.ptr(actions_buf), m.ptr(self.bufs[self.cur]), m.ptr(self.bufs[self.cur ^ 1]),
                                                    m.ptr(self.rewards), m.ptr(self.nonterminals), self.life_terminals, m.stream))
        self.cur ^= 1

    def step(self, actions):
        m = self.mem
        self._ac = m.upload(np.asarray(actions, dtype=np.int32))
        self.step_dev(self._ac)
        m.sync()
        return m.download(self.bufs[self.cur]), m.download(self.rewards).copy(), m.download(self.nonterminals).copy()

    def stats(self):
        st = L.BreakoutStats()
        L.check(self.lib, self.lib.rb_breakout_stats(self.h, C.byref(st), self.mem.stream))
        return dict(games=int(st.games), return_sum=int(st.return_sum), bricks=int(st.bricks), lives_lost=int(st.lives_lost),
                    steps=int(st.steps))

    def reset_stats(self):
        L.check(self.lib, self.lib.rb_breakout_reset_stats(self.h, self.mem.stream))

    def get_state(self):
        arr = (L.BreakoutState * self.S)()
        L.check(self.lib, self.lib.rb_breakout_get_state(self.h, arr, self.mem.stream))
        return arr

    def set_state(self, arr):
        return self.lib.rb_breakout_set_state(self.h, arr, self.mem.stream)

    def set_stacks(self, stacks):
        self.bufs[self.cur] = self.mem.upload(np.asarray(stacks, dtype=np.float32))


def state_dicts(arr):
    """rb_breakout_state_t [S] -> the oracle's per-stream dicts (k = 0xFFFFFFFF reads as -1)"""
    out = []
    for st in arr:
        g = {f: int(getattr(st, f)) for f in SCALARS}
        g["rows"] = [int(x) for x in st.rows]
        g["k"] = -1 if g["k"] == 0xFFFFFFFF else g["k"]
        assert st.reserved == 0
        out.append(g)
    return out


def state_array(dicts):
    arr = (L.BreakoutState * len(dicts))()
    for st, g in zip(arr, dicts):
        for f in SCALARS:
            setattr(st, f, g[f] & 0xFFFFFFFF if f == "k" else g[f])
        for r in range(3):
            st.rows[r] = g["rows"][r]
    return arr


def game(**kw):
    """A legal mid-game state: all bricks, 3 lives, the ball falling from the serve row; kw overrides."""
    g = BO.blank_game()
    g.update(bx=6, by=BO.SERVE_ROW, dx=1, dy=1, paddle=5, t=0, k=0, rows=[BO.FULL] * 3, lives=3)
    g.update(kw)
    return g


def last_outputs(h):
    """what the handle's last step wrote: (stacks, rewards, nonterminals)"""
    m = h.mem
    return m.download(h.bufs[h.cur]), m.download(h.rewards), m.download(h.nonterminals)


def assert_same_state(env, ora, label):
    got, want = state_dicts(env.get_state()), ora.g
    assert got == want, (label, [(s, k, a[k], b[k]) for s, (a, b) in enumerate(zip(got, want)) for k in a if a[k] != b[k]][:6])


def step_both(env, ora, actions, label):
    got_st, got_rw, got_nt = env.step(actions)
    want_st, want_rw, want_term = ora.step(actions, life_terminals=env.life_terminals)
    assert np.array_equal(got_st, want_st), label
    assert np.array_equal(got_rw, want_rw) and np.array_equal(got_nt.astype(bool), ~want_term), label
    return want_rw, want_term


class Coverage:
    """What the oracle's run went through, summed over rounds and streams."""

    def __init__(self, S):
        self.games = np.zeros(S, dtype=int)
        self.life_only = 0              # steps that lost a life and did not end the game
        self.capped = self.capped_and_lost = self.ceiling = self.refills = self.reward_steps = 0
        self.brick_rows, self.paddle_cells = set(), set()

    def add(self, ora, rewards):
        for s, ev in enumerate(ora.events):
            self.games[s] += bool(ev["over"])
            self.life_only += bool(ev["lost"] and not ev["over"])
            self.capped += bool(ev["capped"])
            self.capped_and_lost += bool(ev["capped"] and ev["lost"])
            self.ceiling += bool(ev["ceiling"])
            self.refills += bool(ev["refill"])
            if ev["brick_row"]:
                self.brick_rows.add(ev["brick_row"])
            if ev["paddle_cell"] is not None:
                self.paddle_cells.add(ev["paddle_cell"])
        self.reward_steps += int((np.asarray(rewards) > 0).sum())


# =============================================================================== 1. random play
def check_breakout_against_oracle(lib, mem, S, history, seed, life_terminals, rounds=200, max_steps=500):
    """Random actions, out-of-range ones included; a manual reset at round 90 and reset_stats at 140.  At 200 rounds and more:
    every stream ends >= 3 games, >= S steps lose a life without ending the game, a brick is hit."""
    rs = np.random.RandomState(seed)
    env, ora = BreakoutHandle(lib, mem, S, history, max_steps, seed, life_terminals), BO.BreakoutOracle(S, history, max_steps, seed)
    assert np.array_equal(env.reset(), ora.reset())
    cov = Coverage(S)
    for r in range(rounds):
        rewards, _ = step_both(env, ora, DS.random_actions(rs, S), (S, history, r))
        cov.add(ora, rewards)
        if r == 90:
            assert env.stats() == ora.stats()
            assert np.array_equal(env.reset(), ora.reset())          # the game in play is abandoned and counts nothing
            assert env.stats() == ora.stats()
        if r == 140:
            env.reset_stats(); ora.reset_stats()
            assert env.stats() == ora.stats() == dict.fromkeys(BO.TOTALS, 0)
    if rounds >= 200:
        assert cov.games.min() >= 3 and cov.life_only >= S and cov.brick_rows
    assert env.stats() == ora.stats()
    assert_same_state(env, ora, "final")
    env.close()
    return cov


# =============================================================================== 2. a policy that keeps the ball in play
def scripted_actions(rs, ora):
    """Move the paddle under the column where the ball will come down (bricks ignored), alternating the paddle cell offered
    to it; 15 % random actions."""
    out = np.zeros(ora.S, dtype=np.int64)
    for s in range(ora.S):
        g = ora.g[s]
        want = min(max(ora.landing_column(s) - (g["bricks"] + s) % 2, 0), BO.GRID - BO.PADDLE)
        out[s] = 1 if g["paddle"] > want else 2 if g["paddle"] < want else 0
    return np.where(rs.random_sample(ora.S) < 0.15, rs.randint(0, 3, ora.S), out)


def check_breakout_scripted_policy(lib, mem, seed, S=7, history=4, rounds=600, max_steps=500):
    rs = np.random.RandomState(seed)
    env, ora = BreakoutHandle(lib, mem, S, history, max_steps, seed), BO.BreakoutOracle(S, history, max_steps, seed)
    assert np.array_equal(env.reset(), ora.reset())
    cov = Coverage(S)
    for r in range(rounds):
        rewards, _ = step_both(env, ora, scripted_actions(rs, ora), (seed, r))
        cov.add(ora, rewards)
    assert cov.ceiling >= 1 and cov.brick_rows == {1, 2, 3} and cov.paddle_cells == {0, 1}
    assert cov.capped >= 1                                             # a game of 500 steps inside the 600 rounds
    assert env.stats() == ora.stats()
    assert_same_state(env, ora, "final")
    env.close()
    return cov


# =============================================================================== 3. the step cap
def check_breakout_step_cap(lib, mem, seed, max_steps, S=7, history=4, rounds=200):
    """200 random rounds with a cap so low that games end by it.  Also wanted: a capped step that loses a life.  From a new
    game the ball reaches the paddle row 7 steps after a serve, 14 after a bounce (a brick of row 3 on the way) and 16 or 18
    after a bounce through a gap in the wall, and 7 a + 14 b + 16 c + 18 d = 25 has no solution a game of 25 steps can reach
    (7 + 18 needs a gap two rows deep on the first way up), so at max_steps = 25 no capped step can lose a life, whatever
    the seed; at max_steps = 28 (7 + 7 + 14 in any order) it happens in every run.  Both caps are run; the constructed
    states of check_breakout_cap_cases put the two on one step directly."""
    rs = np.random.RandomState(seed)
    env, ora = BreakoutHandle(lib, mem, S, history, max_steps, seed), BO.BreakoutOracle(S, history, max_steps, seed)
    assert np.array_equal(env.reset(), ora.reset())
    cov = Coverage(S)
    for r in range(rounds):
        rewards, _ = step_both(env, ora, DS.random_actions(rs, S), (seed, r))
        cov.add(ora, rewards)
    assert cov.capped >= S
    assert cov.capped_and_lost >= 1 or max_steps == 25
    assert env.stats() == ora.stats()
    assert max(g["t"] for g in ora.g) < max_steps
    env.close()
    return cov


# =============================================================================== 4. constructed states
def _constructed(lib, mem, dicts, history=2, max_steps=500, life_terminals=1, seed=77):
    """A handle and an oracle put into the given states (no reset), with the same random stacks under them."""
    S = len(dicts)
    env, ora = BreakoutHandle(lib, mem, S, history, max_steps, seed, life_terminals), BO.BreakoutOracle(S, history, max_steps, seed)
    assert env.set_state(state_array(dicts)) == 0, lib.rb_last_error()
    ora.g = [dict(g, rows=list(g["rows"])) for g in dicts]
    stacks = np.random.RandomState(5).random_sample((S, history, 84, 84)).astype(np.float32)
    env.set_stacks(stacks)
    ora.stacks = stacks.copy()
    assert_same_state(env, ora, "set_state")
    return env, ora


def check_breakout_last_brick_and_refill(lib, mem):
    """One brick left and the ball about to take it; the paddle waits where the ball comes down: the bounce refills all 36."""
    one = game(bx=4, by=4, dx=1, dy=-1, paddle=10, rows=[0, 0, 1 << 5], t=40, game_return=70, bricks=35)
    env, ora = _constructed(lib, mem, [one, game(bx=3, by=4, dx=1, dy=-1, paddle=0, rows=[0, 0, 1 << 4])])
    rewards, _ = step_both(env, ora, [0, 0], "the last brick")
    assert rewards.tolist() == [2.0, 2.0] and ora.g[0]["rows"] == [0, 0, 0] and (ora.g[0]["bx"], ora.g[0]["by"]) == (4, 4)
    refilled = None
    for i in range(12):
        step_both(env, ora, [0, 0], ("after the last brick", i))
        assert_same_state(env, ora, ("after the last brick", i))
        if ora.events[0]["refill"]:
            refilled = i
            break
        assert ora.g[0]["rows"] == [0, 0, 0]
    assert refilled == 6 and ora.events[0]["paddle_cell"] == 1
    got = state_dicts(env.get_state())
    assert got[0]["rows"] == [BO.FULL] * 3 and got[0]["lives"] == 3 and got[0]["t"] == 48
    assert got[1]["rows"] == [0, 0, 0] and got[1]["lives"] == 2          # stream 1 had no paddle there: no refill, a life lost
    for i in range(8):                                                    # and the refilled wall is played on
        step_both(env, ora, [0, 0], ("refilled", i))
    assert ora.stats()["bricks"] == 35 + 2 + 1
    assert env.stats() == ora.stats()
    env.close()


def check_breakout_corner(lib, mem):
    """bx = 0, by = 0, dx = dy = -1: both reflections in one step, with and without a brick at (1, 1)."""
    corner = dict(bx=0, by=0, dx=-1, dy=-1)
    env, ora = _constructed(lib, mem, [game(**corner), game(rows=[BO.FULL & ~2, BO.FULL, BO.FULL], **corner)])
    rewards, _ = step_both(env, ora, [1, 2], "corner")
    assert rewards.tolist() == [4.0, 0.0]
    assert all(ora.events[s]["wall"] and ora.events[s]["ceiling"] for s in range(2))
    assert [(g["bx"], g["by"], g["dx"], g["dy"]) for g in ora.g] == [(0, 0, 1, -1), (1, 1, 1, 1)]
    for i in range(6):
        step_both(env, ora, [0, 0], ("corner", i))
        assert_same_state(env, ora, ("corner", i))
    env.close()


def check_breakout_cap_cases(lib, mem, life_terminals):
    """t = max_steps - 1: the last life missed on the capped step (stream 0), a brick hit on the capped step (stream 1, its
    reward belongs to the game that ends), a life lost on the capped step with lives to spare (stream 2)."""
    M = 30
    miss = dict(bx=5, by=10, dx=1, dy=1, paddle=0, t=M - 1)
    env, ora = _constructed(lib, mem, [game(lives=1, game_return=9, **miss),
                                       game(bx=4, by=4, dx=1, dy=-1, t=M - 1, game_return=5),
                                       game(lives=3, **miss)], max_steps=M, life_terminals=life_terminals)
    rewards, terms = step_both(env, ora, [0, 0, 0], "capped")
    assert rewards.tolist() == [0.0, 2.0, 0.0] and terms.all()
    assert all(ev["capped"] and ev["over"] for ev in ora.events) and [bool(ev["lost"]) for ev in ora.events] == [True, False, True]
    assert env.stats() == ora.stats() == dict(games=3, return_sum=9 + 7 + 0, bricks=1, lives_lost=2, steps=3)
    for g in ora.g:
        assert (g["t"], g["lives"], g["rows"], g["k"], g["game_return"]) == (0, 3, [BO.FULL] * 3, 1, 0)
    assert_same_state(env, ora, "capped")
    for i in range(M + 3):                                                # through the next cap as well
        step_both(env, ora, [2, 1, 0], ("after the cap", i))
    assert_same_state(env, ora, "after the next cap")
    env.close()


def check_breakout_resume(lib, mem, seed=31, S=5, history=4, max_steps=60):
    """get_state after 50 rounds, set_state into a fresh handle together with the copied stacks: the next 50 rounds are those
    of the handle that went on (and of the oracle)."""
    rs = np.random.RandomState(seed)
    env, ora = BreakoutHandle(lib, mem, S, history, max_steps, seed), BO.BreakoutOracle(S, history, max_steps, seed)
    env.reset(); ora.reset()
    for r in range(50):
        step_both(env, ora, DS.random_actions(rs, S), r)
    saved, stacks = env.get_state(), mem.download(env.stacks()).copy()
    twin = BreakoutHandle(lib, mem, S, history, max_steps, seed)
    assert twin.set_state(saved) == 0                                     # (marks the handle as reset: no rb_breakout_reset)
    twin.set_stacks(stacks)
    assert twin.stats() == env.stats() == ora.stats()
    for r in range(50):
        actions = DS.random_actions(rs, S)
        want = env.step(actions)
        step_both(twin, ora, actions, ("resumed", r))
        for u, v in zip(last_outputs(twin), want):
            assert np.array_equal(u, v), r
    assert bytes(twin.get_state()) == bytes(env.get_state())
    assert twin.stats() == ora.stats() and ora.stats()["games"] >= S
    env.close(); twin.close()


INVALID = [("bx", -1), ("bx", 12), ("by", -1), ("by", 11), ("dx", 0), ("dx", 2), ("dy", 0), ("dy", -2), ("paddle", -1),
           ("paddle", 11), ("t", -1), ("t", 40), ("lives", 0), ("lives", 4), ("rows", [0x1000, 0, 0]), ("rows", [0, 0, 0xFFFF]),
           ("game_return", -1), ("games", -1), ("return_sum", -1), ("bricks", -1), ("lives_lost", -1), ("steps", -1)]


def check_breakout_set_state_refusals(lib, mem):
    """Every field out of its range, the ball on a brick and a non-zero reserved word: RB_ERR_INVALID naming the entry point,
    the device state as it was, and a handle that was never reset stays one."""
    M = 40
    env = BreakoutHandle(lib, mem, 2, 2, M, 3)
    fresh = BreakoutHandle(lib, mem, 2, 2, M, 3)
    env.reset()
    before = bytes(env.get_state())
    good = state_dicts(env.get_state())
    cases = [dict(good[1], **{f: v}) for f, v in INVALID]
    cases += [dict(good[1], bx=7, by=2), dict(good[1], bx=0, by=1), dict(good[1], bx=11, by=3)]       # on a brick
    arrays = [state_array([good[0], bad]) for bad in cases]
    arrays.append(state_array(good))
    arrays[-1][0].reserved = 1
    ac = mem.upload(np.zeros(2, dtype=np.int32))
    for arr in arrays:
        for h in (env, fresh):
            assert h.set_state(arr) == -1
            err = lib.rb_last_error()
            assert b"rb_breakout_set_state" in err and (b"stream 1" in err or arr[0].reserved), err
        assert bytes(env.get_state()) == before
        args = [mem.ptr(ac), mem.ptr(fresh.bufs[0]), mem.ptr(fresh.bufs[1]), mem.ptr(fresh.rewards), mem.ptr(fresh.nonterminals)]
        assert lib.rb_breakout_step(fresh.h, *args, 1, mem.stream) == -4
    assert env.set_state(None) == -1 and b"NULL" in lib.rb_last_error()
    # the edges of the ranges are accepted (t = max_steps - 1, a ball in a gap of the wall)
    edge = dict(good[1], bx=11, by=3, rows=[BO.FULL, BO.FULL, BO.FULL & ~(1 << 11)], t=M - 1, lives=1, paddle=10)
    assert env.set_state(state_array([good[0], edge])) == 0
    assert state_dicts(env.get_state())[1] == edge
    env.close(); fresh.close()


# =============================================================================== 5. seeds and refusals
def check_breakout_seeds_and_refusals(lib, mem):
    mk = lambda seed: BreakoutHandle(lib, mem, 7, 4, 500, seed)
    a, b, c = mk(11), mk(11), mk(12)
    sa, sb, sc = a.reset(), b.reset(), c.reset()
    assert np.array_equal(sa, sb) and not np.array_equal(sa, sc)
    rs = np.random.RandomState(0)
    differ = False
    for r in range(30):
        actions = rs.randint(0, 3, 7)
        xa, xb, xc = a.step(actions), b.step(actions), c.step(actions)
        for u, v in zip(xa, xb):
            assert np.array_equal(u, v)
        differ |= not np.array_equal(xa[0], xc[0])
    assert differ and a.stats() == b.stats()
    for bad in (0, 65, -1):
        h = C.c_void_p()
        assert lib.rb_breakout_create(C.byref(h), bad, 4, 500, 1) == -1 and not h.value
        assert b"rb_breakout_create" in lib.rb_last_error() and b"streams" in lib.rb_last_error()
    for bad in (0, 17):
        h = C.c_void_p()
        assert lib.rb_breakout_create(C.byref(h), 4, bad, 500, 1) == -1 and b"history" in lib.rb_last_error()
    for bad in (0, 65536, -5):
        h = C.c_void_p()
        assert lib.rb_breakout_create(C.byref(h), 4, 4, bad, 1) == -1 and b"max_steps" in lib.rb_last_error() and not h.value
    # a step before the first reset, an in-place step, NULL and misaligned operands are refused
    d = BreakoutHandle(lib, mem, 2, 4, 500, 1)
    ac = mem.upload(np.zeros(2, dtype=np.int32))
    args = [mem.ptr(ac), mem.ptr(d.bufs[0]), mem.ptr(d.bufs[1]), mem.ptr(d.rewards), mem.ptr(d.nonterminals)]
    assert lib.rb_breakout_step(d.h, *args, 1, mem.stream) == -4 and b"rb_breakout_reset" in lib.rb_last_error()
    d.reset()
    for missing in range(5):
        broken = list(args)
        broken[missing] = None
        assert lib.rb_breakout_step(d.h, *broken, 1, mem.stream) == -1 and b"NULL" in lib.rb_last_error()
    broken = list(args)
    broken[2] = broken[1]
    assert lib.rb_breakout_step(d.h, *broken, 1, mem.stream) == -1 and b"overlaps" in lib.rb_last_error()
    broken[2] = args[1] + 4 * 84 * 84 * 4                               # the second stream's stack of the input
    assert lib.rb_breakout_step(d.h, *broken, 1, mem.stream) == -1 and b"overlaps" in lib.rb_last_error()
    broken = list(args)
    broken[1] = args[1] + 4
    assert lib.rb_breakout_step(d.h, *broken, 1, mem.stream) == -1 and b"aligned" in lib.rb_last_error()
    assert lib.rb_breakout_reset(d.h, args[1] + 4, mem.stream) == -1 and b"aligned" in lib.rb_last_error()
    assert lib.rb_breakout_stats(d.h, None, mem.stream) == -1 and lib.rb_breakout_get_state(d.h, None, mem.stream) == -1
    assert lib.rb_breakout_destroy(None) == 0
    for x in (a, b, c, d):
        x.close()


# =============================================================================== 6. guard bands
def check_breakout_guard_bands(lib, guarded_mem, seed=8):
    """Scenario 1 at (7, 4) for 60 rounds on canaried buffers: no band around stacks, rewards or nonterminals is written."""
    check_breakout_against_oracle(lib, guarded_mem, 7, 4, seed, 1, rounds=60)
    n, bad = guarded_mem.check()
    assert n >= 4 and not bad, bad


# =============================================================================== 7. a whole round
def check_breakout_device_round(lib, mem, make_learner, S, rounds, seed):
    """act_batch -> rb_breakout_step(life_terminals = 1) -> rb_replay_append_streams_dev with nothing read back in between,
    against the host-operand append fed by the oracle with the same actions: replays bit-identical, the device timestep vector
    equal to the host's counters — through >= S terminals whose next stack is NOT a reset stack (a lost life)."""
    ad = make_learner()
    history, n = ad.c["history"], ad.c["multi_step"]
    cap = S * (2 * (history + n) + 2)
    env, ora = BreakoutHandle(lib, mem, S, history, 500, seed, 1), BO.BreakoutOracle(S, history, 500, seed)
    dev = DS.DevRoundAdapter(lib, mem, cap, history, n, S)
    host = DS.DevRoundAdapter(lib, mem, cap, history, n, S)
    env.reset()
    stacks = ora.reset()
    actions_dev = mem.empty((S,), np.int32)
    life_terminals = 0
    for r in range(rounds):
        L.check(lib, lib.rb_learner_act_batch(ad.h, mem.ptr(env.stacks()), S, 1, mem.ptr(actions_dev), None, mem.stream))
        acted_on = env.stacks()
        env.step_dev(actions_dev)
        L.check(lib, lib.rb_replay_append_streams_dev(dev.h, mem.ptr(acted_on), mem.ptr(dev.ts_dev), mem.ptr(actions_dev),
                                                      mem.ptr(env.rewards), mem.ptr(env.nonterminals), mem.stream))
        mem.sync()
        actions = mem.download(actions_dev).copy()          # (read back for the host-driven twin only)
        assert actions.min() >= 0 and actions.max() < BO.ACTIONS
        nxt, rewards, terms = ora.step(actions, life_terminals=True)
        host.append_round(stacks, actions, rewards, terms)
        for s, ev in enumerate(ora.events):
            if ev["lost"] and not ev["over"]:            # a terminal whose next stack is the old one moved on, not a reset stack
                assert terms[s] and np.array_equal(nxt[s, :-1], stacks[s, 1:]) and nxt[s, -2].any()
                life_terminals += 1
        stacks = nxt
        assert np.array_equal(mem.download(env.stacks()), stacks), r
        DS.assert_identical(host, dev, "round %d" % r)
        assert np.array_equal(dev.timesteps_dev(), host.stream_t)
    assert life_terminals >= S
    assert env.stats() == ora.stats()
    for x in (env, dev, host, ad):
        x.close()
