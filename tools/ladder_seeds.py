"""usage: python tools/ladder_seeds.py [case ...] [--seeds N] [--best] — the data seeds of tests/test_learner_batches_gpu.py's table.  CPU only.
For each case: the first seed in [0, N) for which the ORACLE ALONE reports a hidden_relu_margin of at least RELU_MARGIN in both of the
test's steps (step 1 runs on the oracle's own post-Adam parameters of step 0), or 'none': the case then hands the device's ReLU
decisions to the oracle (masked).  --best: all N seeds, and the one whose smaller margin is largest (a seed well clear of the bound
where the first one only just passes).  Prints the margins it saw and the oracle's time for the two steps.
usage: python tools/ladder_seeds.py --shape-range [case ...] [--seeds N] — the same for tests/shape_range_scenarios.py's table: the first
seed in [0, N) (default 14) that gives both steps a margin of at least 2.5 x RELU_MARGIN and the act calls their top-two gap; prints the
row's seed and margins as the table holds them, and 'none' where the row has to be masked.
usage: python tools/ladder_seeds.py --exchange [case ...] [--seeds N] — the same for table B of tests/exchange_scenarios.py (the learn step
with the replica exchange armed): the first seed in [0, N) (default 14) for which every rank, in both steps, has a margin of at least
2.5 x RELU_MARGIN; the margins printed are the smallest over the ranks."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import test_learner_batches_gpu as T  # noqa: E402
from oracle import learner_oracle as O  # noqa: E402


def margin(run, k):
    st, probe = run.inp["steps"][k], {}
    x = torch.from_numpy(st["batch"]["states"]).to(torch.float32).div(255)
    with torch.no_grad():
        O.forward(run.inp["cfg"], {n: torch.from_numpy(v) for n, v in run.online.items()}, O.make_noise(run.inp["cfg"], st["raw_on"]), x,
                  log=True, probe=probe)
    return probe["hidden_relu_margin"]


args = sys.argv[1:]
if "--exchange" in args:
    import exchange_scenarios as ES  # noqa: E402
    args.remove("--exchange")
    n = 14
    if "--seeds" in args:
        i = args.index("--seeds")
        n = int(args[i + 1])
        del args[i:i + 2]
    for case in args or list(ES.LEARN_CASES):
        t0 = time.time()
        found, seen = ES.find_seed(case, n)
        tried = "; ".join("%d: %.1e %.1e" % (s, m[0], m[1]) for s, m in seen)
        if found:
            print("%-14s seed %d   margins (%.1e, %.1e)   (%.1f s)   seen: %s" % (case, found[0], found[1][0], found[1][1], time.time() - t0, tried),
                  flush=True)
        else:
            print("%-14s seed none: masked   (%.1f s)   seen: %s" % (case, time.time() - t0, tried), flush=True)
    sys.exit(0)
if "--shape-range" in args:
    import shape_range_scenarios as SR  # noqa: E402
    args.remove("--shape-range")
    n = 14
    if "--seeds" in args:
        i = args.index("--seeds")
        n = int(args[i + 1])
        del args[i:i + 2]
    for case in args or list(SR.CASES):
        t0 = time.time()
        found, masked, seen = SR.find_seed(case, n)
        tried = "; ".join("%d: %.1e %.1e gap %.1e" % (s, m[0], m[1], g) for s, m, g in seen)
        if found:
            print("%-14s seed %d   margins (%.1e, %.1e)   act gap %.3e   (%.1f s)   seen: %s" % (case, found[0], found[1][0], found[1][1], found[2],
                                                                                             time.time() - t0, tried), flush=True)
        else:
            print("%-14s seed none: masked, on seed %s (the first whose act calls have their gap)   (%.1f s)   seen: %s"
                  % (case, masked[0] if masked else "none", time.time() - t0, tried), flush=True)
    sys.exit(0)
n = 12
best = "--best" in args
if best:
    args.remove("--best")
if "--seeds" in args:
    i = args.index("--seeds")
    n = int(args[i + 1])
    del args[i:i + 2]
for case in args or list(T.LADDER):
    found, seen, top = None, [], 0.0
    for seed in range(n):
        run = T.OracleRun(T.case_inputs(case, seed))
        m0 = margin(run, 0)
        if m0 < T.RELU_MARGIN:
            seen.append("%d: %.1e" % (seed, m0))
            continue
        t0 = time.time()
        run.step(0)
        dt = time.time() - t0
        m1 = margin(run, 1)
        seen.append("%d: %.1e %.1e" % (seed, m0, m1))
        if m1 >= T.RELU_MARGIN and min(m0, m1) > top:
            found, top = seed, min(m0, m1)
            if not best:
                break
    print("%-10s seed %s   (oracle step %.1f s)   margins by seed: %s" % (case, found if found is not None else "none", dt if seen else 0.0,
                                                                          "; ".join(seen)), flush=True)
