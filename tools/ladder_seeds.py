"""usage: python tools/ladder_seeds.py [case ...] [--seeds N] [--best] — the data seeds of tests/test_learner_batches_gpu.py's table.  CPU only.
For each case: the first seed in [0, N) for which the ORACLE ALONE reports a hidden_relu_margin of at least RELU_MARGIN in both of the
test's steps (step 1 runs on the oracle's own post-Adam parameters of step 0), or 'none': the case then hands the device's ReLU
decisions to the oracle (masked).  --best: all N seeds, and the one whose smaller margin is largest (a seed well clear of the bound
where the first one only just passes).  Prints the margins it saw and the oracle's time for the two steps."""
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
