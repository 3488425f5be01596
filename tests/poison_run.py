"""Read-before-write hunt (run as a script, with RB_GUARD=1 or 2 in the environment; tests/test_poison_emu.py and
tests/test_poison_gpu.py run it once under each and compare).  Under 1 every allocation the library owns, and every buffer this
script hands to the C ABI, is zeroed between its guard bands; under 2 both are left at the bands' fill byte 0xC5
(include/rainbow_hip.h rb_debug_check_guards, tests/guarded_mem.py Poisoned*Mem).  A kernel that reads memory nobody has written
sees 0.0 under 1 and -6.3e3 (or a nonsense integer) under 2, so the two runs of one group must write the same digests.
    python tests/poison_run.py <emu|hip> <group> <out.json>
out.json: {"level", "digests": {"<case>/<tensor>": sha256}, "guards": [per case: library and caller block counts and overwritten
bands], "control": ...}.  Only OUTPUTS are digested — per-sample loss, gradient norm, every named gradient, parameter and Adam
moment (never the alignment padding of the flat buffers), a*, m, log_ps_a, act (action, q), replay traces; in the groups that run
a scenario body unchanged (its oracle is exact or has its own tolerance, so the body is a comparator too), everything the body
downloads from the device, in order.

Groups (no shape of its own: every table and input builder is the parity tests'):
  control          a fresh learner's m (RB_ALLOC without a clear), read before any learn call: 0xC5 bytes under 2, zeros under 1
  learn-small      the four small scenarios.LEARN_CONFIGS (learn-k10: the last of them alone)
  learn-ladder-a/b/c, learn-ladder-opts   test_learner_batches_gpu.RUNS (device only)
  learn-range      shape_range_scenarios.LEARN_RUNS (host interpreter: EMU_CASES); -narrow / -wide-b4 / -wide-batch: its parts
  learn-head       head_shapes_scenarios.CASES
  exchange-finish  exchange_scenarios.check_finish over FINISH_CASES
  exchange-learn   exchange_scenarios.check_learn over LEARN_RUNS (host interpreter: EMU_LEARN_RUNS)
  replay-golden    scenarios.replay_scenario over REPLAY_CONFIGS, update_sample_twin_check
  replay-streams   streams_scenarios.check_append_rounds / check_sampling, device_loop_scenarios.check_append_dev_equals_host
  replay-shift     shift_scenarios.check_injected_enumeration / check_philox_path, horizon_scenarios.check_table_row / check_write_head
  envs-obs         obs_stack_scenarios.check_scripted, test_frames._check_backend, check_catch_against_oracle
  envs-breakout    check_breakout_against_oracle
  envs-eval        eval_scenarios.check_tally_against_oracle / check_eps_quarter
A learn row, in this order: two learn steps; rb_learner_act_batch at 3 B + 1 rows (ensure_rows frees and re-allocates the forward
buffers); rb_learner_act_batch_rows at 17 rows (ensure_rows_scaled); a third learn step on the regrown buffers; rb_learner_act,
noisy and eval.  No oracle runs."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LEVEL = os.environ.get("RB_GUARD")
assert LEVEL in ("1", "2"), "run with RB_GUARD=1 or RB_GUARD=2"

import scenarios  # noqa: E402
from rainbow_amd import _lib as L  # noqa: E402

ACT_ROWS_SCALED = 17


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s%s|" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


class Recorder:
    def __init__(self, lib):
        self.lib, self.digests, self.guards, self.control = lib, {}, [], None
        self.case, self.n_auto, self.mems, self.flat, self.t0 = None, 0, [], {}, time.time()

    def begin(self, case):
        self.case, self.n_auto, self.mems, self.flat, self.t0 = case, 0, [], {}, time.time()

    def put(self, name, arr):
        key = "%s/%s" % (self.case, name)
        assert key not in self.digests, key
        self.digests[key] = sha(arr)

    def auto(self, arr):
        """A download of a scenario body: digested whole, except a flat parameter-sized buffer, of which only the named tensors
        count (register_flat) — the alignment padding between them belongs to nobody."""
        arr = np.asarray(arr)
        lay = self.flat.get(arr.size) if arr.ndim == 1 else None
        if lay is not None:
            arr = np.concatenate([arr[off:off + int(np.prod(shape))] for off, shape in lay])
        self.put("download%04d" % self.n_auto, arr)
        self.n_auto += 1

    def register_flat(self, ad):
        self.flat[ad.n_params] = sorted(ad.layout.values())

    def end(self, live=False):
        """The library's and the caller's guard counts after the case (live: the case's handle still exists, so the library owns
        guarded blocks; a scenario body has destroyed its own by the time it returns, and the count is what else is alive)."""
        nb, bad = C.c_int64(0), C.c_int64(0)
        L.check(self.lib, self.lib.rb_debug_check_guards(C.byref(nb), C.byref(bad)))
        checks = [m.check() for m in self.mems]
        g = dict(case=self.case, lib_blocks=nb.value, lib_bad=bad.value, caller_blocks=sum(n for n, _b in checks),
                 caller_bad=[name for _n, b in checks for name in b], seconds=round(time.time() - self.t0, 2))
        self.guards.append(g)
        print("  %-44s library blocks %4d bad %d, caller blocks %4d bad %d, %.1f s"
              % (g["case"], g["lib_blocks"], g["lib_bad"], g["caller_blocks"], len(g["caller_bad"]), g["seconds"]), flush=True)
        assert nb.value > 0 or not live, "library allocations are not guarded (RB_GUARD read too late?)"


def recording(Base, rec, auto):
    """Base (guarded_mem.Guarded* / Poisoned*Mem) whose instances report to `rec`; auto: digest every download and view."""
    class Mem(Base):
        def __init__(self):
            super().__init__()
            rec.mems.append(self)

        def download(self, buf):
            out = super().download(buf)
            if auto:
                rec.auto(out)
            return out

        def view(self, ptr, shape, dtype):
            out = super().view(ptr, shape, dtype)
            if auto:
                rec.auto(out)
            return out
    return Mem


# =============================================================================== control
def run_control(rec, Mem, where):
    from head_shapes_scenarios import make_learner
    rec.begin("control")
    c = scenarios.LEARN_CONFIGS["k10"]
    m = Mem()
    ad = make_learner(rec.lib, m, "control", c)
    try:
        out = m.upload(np.full((c["batch"], c["atoms"]), 0x11111111, dtype=np.uint32).view(np.float32))   # neither zero nor the fill
        L.check(rec.lib, rec.lib.rb_learner_debug_read(ad.h, 1, m.ptr(out), m.stream))
        m.sync()
        got = np.unique(m.download(out).view(np.uint8)).tolist()
        rec.end(live=True)
    finally:
        ad.close()
    want = [0x00] if LEVEL == "1" else [0xC5]
    assert got == want, "control: the bytes of a fresh learner's m are %s, expected %s under RB_GUARD=%s" % (got, want, LEVEL)
    rec.control = dict(m_bytes=got)


# =============================================================================== learn
def learn_row(rec, Mem, case, cfgd, inp, flagset="default", steps=2, full=True):
    """inp: dict(online, target, steps=[dict(raw_on, raw_tg, batch), ...]).  steps: learn steps before the regrow."""
    from head_shapes_scenarios import make_learner
    lib = rec.lib
    rec.begin(case if flagset == "default" else "%s[%s]" % (case, flagset))
    B, Z, h = cfgd["batch"], cfgd["atoms"], cfgd["history"]
    if "=" in flagset:
        os.environ["RB_OPTS"] = flagset          # read when the handle is created
    m = Mem()
    try:
        ad = make_learner(lib, m, case, cfgd)
    finally:
        os.environ.pop("RB_OPTS", None)
    try:
        if flagset == "implicit-sigma":
            ad.learner_flags = L.LEARNER_IMPLICIT_SIGMA
        ad.load(inp["online"], inp["target"])

        def learn(tag, st):
            ad.reset_noise_online(st["raw_on"])
            got = ad.learn_step(st["batch"], st["raw_tg"])
            rec.put(tag + "_loss", got["loss"])
            rec.put(tag + "_grad_norm", np.float32(got["grad_norm"]))
            for name, g in got["grads"].items():
                rec.put("%s_grad/%s" % (tag, name), g)
            for name, p in ad.params().items():
                rec.put("%s_param/%s" % (tag, name), p)
            for mom, buf in (("exp_avg", ad.adam_m), ("exp_avg_sq", ad.adam_v)):
                for name, v in ad._unflat(m.download(buf)).items():
                    rec.put("%s_%s/%s" % (tag, mom, name), v)
            rec.put(tag + "_a_star", ad.debug(2, (B,), np.int32))
            rec.put(tag + "_m", ad.debug(1, (B, Z), np.float32))
            rec.put(tag + "_log_ps_a", ad.debug(0, (B, Z), np.float32))

        for k in range(steps):
            learn("s%d" % k, inp["steps"][k % len(inp["steps"])])
        if full:
            rs = np.random.RandomState(77)
            n = 3 * B + 1                                                           # beyond rows_cap = 3 B: ensure_rows
            st = rs.randint(0, 256, size=(max(n, ACT_ROWS_SCALED), h, 84, 84)).astype(np.uint8).astype(np.float32) * np.float32(1.0 / 255.0)
            a, q = ad.act_batch(st[:n], True)
            rec.put("act_batch_a", a)
            rec.put("act_batch_q", q)
            n = ACT_ROWS_SCALED                                                     # ensure_rows_scaled
            draws = len(inp["steps"][0]["raw_on"])
            raw = m.upload(rs.randn(n, draws).astype(np.float32))
            rows = m.empty((n, ad.n_noise), np.float32)
            L.check(lib, lib.rb_learner_noise_rows(ad.h, n, 0, 0, 0, m.ptr(raw), m.ptr(rows), m.stream))
            assert len(st) >= n
            sd, a, q = m.upload(st[:n]), m.empty((n,), np.int32), m.empty((n,), np.float32)
            L.check(lib, lib.rb_learner_act_batch_rows(ad.h, m.ptr(sd), n, m.ptr(rows), m.ptr(a), m.ptr(q), m.stream))
            m.sync()
            rec.put("act_rows_a", m.download(a))
            rec.put("act_rows_q", m.download(q))
            del st, sd
            learn("s%d" % steps, inp["steps"][0])                                   # on the regrown buffers
        st1 = scenarios.synth_state(np.random.RandomState(78), h, 0)
        for noisy in (True, False):
            a, q = ad.act(st1, noisy)
            rec.put("act_%s" % ("noisy" if noisy else "eval"), np.array([a, np.float32(q).view(np.int32)], dtype=np.int64))
        rec.end(live=True)
    finally:
        ad.close()


def run_learn_small(rec, Mem, where, names=("canon", "dataeff", "atoms21", "k10")):
    from learn_steps import two_step_inputs
    for name in names:
        c = scenarios.LEARN_CONFIGS[name]
        # the interpreter tests run the canonical stack for one step (test_learner_emu.py); so does this, and its third step is left out
        emu_canon = where == "emu" and name == "canon"
        learn_row(rec, Mem, name, c, two_step_inputs(c, 0), steps=1 if emu_canon else 2)


def _ladder(rec, Mem, runs):
    import test_learner_batches_gpu as TB
    for case, flagset in runs:
        learn_row(rec, Mem, case, TB.LADDER[case][0], TB.case_inputs(case), flagset)


def ladder_parts():
    """test_learner_batches_gpu.RUNS, every row, in parts of a few seconds of input generation each."""
    import test_learner_batches_gpu as TB
    default = [r for r in TB.RUNS if r[1] == "default"]
    big = [r for r in default if TB.LADDER[r[0]][0]["batch"] >= 257]
    rest = [r for r in default if r not in big]
    parts = {"learn-ladder-a": rest[:len(rest) // 2], "learn-ladder-b": rest[len(rest) // 2:], "learn-ladder-c": big,
             "learn-ladder-opts": [r for r in TB.RUNS if r[1] != "default"]}
    assert sorted(sum(parts.values(), [])) == sorted(TB.RUNS)
    return parts


def run_learn_range(rec, Mem, where, part=None):
    import shape_range_scenarios as SR
    from learn_steps import two_step_inputs
    runs = [(c, "default") for c in SR.EMU_CASES] if where == "emu" else SR.LEARN_RUNS
    if part is not None:      # the rows with 2 M hidden-layer weights and more apart, batch 4 and above: their inputs and digests take seconds
        wide = [r for r in runs if r[0] in SR.WIDE_NORM_ROWS]
        parts = {"narrow": [r for r in runs if r not in wide], "wide-b4": [r for r in wide if SR.case_config(r[0])["batch"] == 4],
                 "wide-batch": [r for r in wide if SR.case_config(r[0])["batch"] != 4]}
        assert sorted(sum(parts.values(), [])) == sorted(runs)
        runs = parts[part]
    for case, flagset in runs:
        cfgd = SR.case_config(case)
        learn_row(rec, Mem, case, cfgd, two_step_inputs(cfgd, SR.CASES[case].seed), flagset)


def run_learn_head(rec, Mem, where):
    import head_shapes_scenarios as HS
    for case in sorted(HS.CASES):
        c, seed = HS.case_config(case)
        _cfg, online, target, raw_on, raw_tg, batch = HS.learn_inputs(c, seed)
        learn_row(rec, Mem, case, c, dict(online=online, target=target, steps=[dict(raw_on=raw_on, raw_tg=raw_tg, batch=batch)]))


# =============================================================================== bodies that run unchanged
def run_exchange(rec, Mem, where, which):
    import exchange_scenarios as XS
    inner = XS.make_learner

    def make_learner(lib, mem, case, c):
        """The body's own adapters.  Their flat buffers are digested by tensor: the parameter-sized ones, the noise buffer (the
        resample writes the eps vectors, not the padding between them) and a rank's exchange block (its noise and conv segments
        are copies of those two; the gaps between its segments are never read, include/rainbow_hip.h)."""
        ad = inner(lib, mem, case, c)
        rec.register_flat(ad)
        noise = sorted(XS._noise_layout(lib, ad).values())
        rec.flat[ad.n_noise] = noise
        B, NZ, H = c["batch"], c["atoms"] * (c["actions"] + 1), c["hidden"]
        F = int(np.prod(XS.conv_shapes(XS.O.Config(**c), B)[-1][1:]))
        stride, _off, small = XS.exchange_layout(lib, ad)
        lay, total = XS.block_layout(B, NZ, H, F, ad.n_noise, small)
        assert total == stride, (total, stride)
        rec.flat[stride] = ([(lay[s][0], (lay[s][1],)) for s in ("dlogits", "h", "dh", "feat")]
                            + [(lay["noise"][0] + off, shape) for off, shape in noise]
                            + [(lay["conv"][0] + off, shape) for name, (off, shape) in sorted(ad.layout.items()) if name.startswith("convs.")])
        return ad
    XS.make_learner = make_learner
    if which == "finish":
        for case in XS.FINISH_CASES:
            rec.begin(case)
            XS.check_finish(rec.lib, Mem, case, where=where)
            rec.end()
    else:
        for case, flagset in (XS.EMU_LEARN_RUNS if where == "emu" else XS.LEARN_RUNS):
            rec.begin(case if flagset == "default" else "%s[%s]" % (case, flagset))
            XS.check_learn(rec.lib, Mem, case, flagset, where=where)
            rec.end()


def body(rec, name, fn):
    rec.begin(name)
    fn()
    rec.end()


def run_replay_golden(rec, Mem, where):
    from cabi_adapter import CAbiReplayAdapter
    lib = rec.lib
    for name in sorted(scenarios.REPLAY_CONFIGS):
        rec.begin("golden-" + name)
        capacity, history, n, discount, omega, _ = scenarios.REPLAY_CONFIGS[name]
        ad = CAbiReplayAdapter(lib, Mem(), capacity, history, n, discount, omega)
        for key, val in scenarios.replay_scenario(ad, name).items():
            rec.put("trace/" + key, val)
        ad.close()
        rec.end()
    for capacity, n in ((6000, 3), (2000, 20) if where == "emu" else (100000, 20)):     # test_replay_emu.py / test_replay_gpu.py
        body(rec, "twin-c%d-n%d" % (capacity, n), lambda: scenarios.update_sample_twin_check(
            lambda c, h, nn: CAbiReplayAdapter(lib, Mem(), c, h, nn, 0.99, 0.5), capacity=capacity, n=n))


def run_replay_streams(rec, Mem, where):
    import device_loop_scenarios as DS
    import streams_scenarios as SS
    lib, emu = rec.lib, where == "emu"
    for S in (2, 7, 16, 64):                                    # test_replay_streams_emu.py / _gpu.py
        body(rec, "append-rounds-S%d" % S, lambda: SS.check_append_rounds(lib, Mem(), S, seed=(100 if emu else 200) + S))
    for S in (2, 16, 64):
        for n in (3, 20):
            body(rec, "sampling-S%d-n%d" % (S, n), lambda: SS.check_sampling(lib, Mem(), S, n, seed=(10 if emu else 20) * S + n))
    for S in (1, 2, 7, 16, 64):                                 # test_device_loop_emu.py / _gpu.py
        body(rec, "append-dev-S%d" % S, lambda: DS.check_append_dev_equals_host(lib, Mem(), S, seed=(300 if emu else 400) + S))


def run_replay_shift(rec, Mem, where):
    import horizon_scenarios as HZ
    import shift_scenarios as SH
    lib = rec.lib
    for history, n, streams in ((4, 3, 1), (1, 1, 1), (3, 20, 1), (4, 3, 3)):       # test_shift_emu.py / _gpu.py
        for pad in (1, 4, 8):
            body(rec, "shift-h%d-n%d-S%d-pad%d" % (history, n, streams, pad),
                 lambda: SH.check_injected_enumeration(lib, Mem(), history, n, pad, streams=streams))
    for seed in (7, 0x9E3779B97F4A7C15):
        body(rec, "philox-%x" % seed, lambda: SH.check_philox_path(lib, Mem(), seed))
    for row in (HZ.A1_EMU_ROWS if where == "emu" else HZ.A1_ROWS):                  # test_horizon_emu.py / _gpu.py
        body(rec, "horizon-" + HZ.a1_id(row), lambda: HZ.check_table_row(lib, Mem(), row))
    for streams, cap in ((1, 96), (3, 192)):
        body(rec, "write-head-S%d" % streams, lambda: HZ.check_write_head(lib, Mem(), S=streams, cap=cap))


def run_envs_obs(rec, Mem, where):
    import device_loop_scenarios as DS
    import obs_stack_scenarios as OS
    import test_frames as TF
    lib, emu = rec.lib, where == "emu"
    for history in (1, 4):                                      # test_obs_stack_emu.py / _gpu.py
        for S in (1, 3, 64):
            body(rec, "obs-S%d-h%d" % (S, history), lambda: OS.check_scripted(lib, Mem(), S, history, seed=3))
    body(rec, "obs-S2-h16", lambda: OS.check_scripted(lib, Mem(), 2, 16, seed=4))
    body(rec, "obs-97x131", lambda: OS.check_scripted(lib, Mem(), 3, 4, H=97, W=131, seed=5))
    body(rec, "frames", lambda: TF._check_backend(lib, Mem()))
    for history in (1, 4):                                      # test_device_loop_emu.py / _gpu.py
        for S in (1, 7, 64):
            body(rec, "catch-S%d-h%d" % (S, history),
                 lambda: DS.check_catch_against_oracle(lib, Mem(), S, history, seed=(1000 if emu else 2000) * history + S))


def run_envs_breakout(rec, Mem, where):
    import breakout_scenarios as BS
    k = 1000 if where == "emu" else 2000                        # test_breakout_emu.py / _gpu.py
    for life_terminals in (0, 1):
        for S, history, rounds in ((1, 1, 200), (1, 4, 200), (7, 1, 200), (7, 4, 200), (64, 4, 100)):
            body(rec, "breakout-S%d-h%d-lt%d" % (S, history, life_terminals),
                 lambda: BS.check_breakout_against_oracle(rec.lib, Mem(), S, history, seed=k * history + 10 * S + life_terminals,
                                                          life_terminals=life_terminals, rounds=rounds))


def run_envs_eval(rec, Mem, where):
    import eval_scenarios as ES
    lib, emu = rec.lib, where == "emu"
    for S, episodes in ((1, 1), (1, 5), (3, 7), (64, 10), (64, 130)):               # test_eval_emu.py / _gpu.py
        body(rec, "tally-S%d-E%d" % (S, episodes),
             lambda: ES.check_tally_against_oracle(lib, Mem(), S, episodes, seed=(100 if emu else 200) * S + episodes))
    n_stat = 7 if emu else 64
    seed = ES.pick_seed(n_stat)
    rec.begin("eps-context")
    ctx = ES.EpsContext(lib, Mem(), n_stat)
    rec.end()
    try:
        for row0 in ES.ROW0S:
            parts = [(2 * p, 2 * p + 1) for p in range(ES.EPS_ROUNDS // 2)] if emu else [tuple(range(ES.EPS_ROUNDS))]
            for rounds in parts:
                rec.begin("eps-quarter-row%d-round%d" % (row0, rounds[0]))
                rec.mems.append(ctx.mem)
                ES.check_eps_quarter(ctx, n_stat, row0, seed, rounds)
                rec.end()
    finally:
        ctx.close()


GROUPS = {
    "control": (run_control, False),
    "learn-small": (run_learn_small, False),
    "learn-k10": (lambda rec, Mem, where: run_learn_small(rec, Mem, where, ("k10",)), False),
    "learn-range": (run_learn_range, False),
    "learn-range-narrow": (lambda rec, Mem, where: run_learn_range(rec, Mem, where, "narrow"), False),
    "learn-range-wide-b4": (lambda rec, Mem, where: run_learn_range(rec, Mem, where, "wide-b4"), False),
    "learn-range-wide-batch": (lambda rec, Mem, where: run_learn_range(rec, Mem, where, "wide-batch"), False),
    "learn-head": (run_learn_head, False),
    "exchange-finish": (lambda rec, Mem, where: run_exchange(rec, Mem, where, "finish"), True),
    "exchange-learn": (lambda rec, Mem, where: run_exchange(rec, Mem, where, "learn"), True),
    "replay-golden": (run_replay_golden, True),
    "replay-streams": (run_replay_streams, True),
    "replay-shift": (run_replay_shift, True),
    "envs-obs": (run_envs_obs, True),
    "envs-breakout": (run_envs_breakout, True),
    "envs-eval": (run_envs_eval, True),
}
for _part in ("learn-ladder-a", "learn-ladder-b", "learn-ladder-c", "learn-ladder-opts"):
    GROUPS[_part] = ((lambda p: lambda rec, Mem, where: _ladder(rec, Mem, ladder_parts()[p]))(_part), False)


def main():
    where, group, out_path = sys.argv[1:4]
    import guarded_mem as GM
    if where == "emu":
        from hipemu import loader
        lib = loader.load()
        Base = GM.GuardedNumpyMem if LEVEL == "1" else GM.PoisonedNumpyMem
    else:
        assert where == "hip", where
        import torch  # noqa: F401
        lib = L.load()
        Base = GM.GuardedTorchMem if LEVEL == "1" else GM.PoisonedTorchMem
    fn, auto = GROUPS[group]
    rec = Recorder(lib)
    t0 = time.time()
    fn(rec, recording(Base, rec, auto), where)
    with open(out_path, "w") as f:
        json.dump(dict(level=int(LEVEL), group=group, digests=rec.digests, guards=rec.guards, control=rec.control,
                       seconds=round(time.time() - t0, 2)), f, indent=0, sort_keys=True)
    print("poison run ok: RB_GUARD=%s %s %s, %d digests, %d cases, %.1f s" % (LEVEL, where, group, len(rec.digests), len(rec.guards),
                                                                           time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
