"""Same calls, same bits across a change of the Python host layer: runs one small fixed-seed scenario under two checkouts (a
reference tree, --parent, and this one) in fresh processes and compares every result bit for bit.

Scenario (data-efficient architecture, batch 4, hidden 32, history 2, replay capacity 64): 48 appends, 6 learn steps with a
reset_noise() before every second one, one act, one act_batch of 5 states; digests of params, target_params, the Adam moments
and step, the sum-tree, every step's loss and the actions.  Repeated with RAINBOW_AMD_ONE_CALL=0 and RAINBOW_AMD_DEFER_UPDATE=0.
The replay (before the learn steps) is also written with save_to and pickled: the two trees' files must be byte-equal, and each
tree must load the other's into the same replay.

    python tools/host_split_identity.py --parent /path/to/parent/checkout [--out profiles/host_split_identity.txt]"""
import argparse
import hashlib
import io
import json
import os
import pickle
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ({}, {"RAINBOW_AMD_ONE_CALL": "0"}, {"RAINBOW_AMD_DEFER_UPDATE": "0"})


def _sha(x):
    import numpy as np
    import torch
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return hashlib.sha256(x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def _replay_digest(mem):
    d = mem._dump()
    return {k: _sha(d[k]) for k in sorted(d)}


def record(root, work, foreign):
    """Runs under `root`'s rainbow_amd; prints one JSON line of digests.  Writes the replay to work/, or with `foreign` (a
    directory another tree wrote) loads that tree's stream and pickle instead and digests what came back."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    dev = torch.device("cuda", 0)
    if foreign:
        out = {}
        with open(os.path.join(foreign, "replay.stream"), "rb") as f:
            out["from_stream"] = _replay_digest(ReplayMemory.load_from(f, dev))
        with open(os.path.join(foreign, "replay.pkl"), "rb") as f:
            out["from_pickle"] = _replay_digest(pickle.load(f))
        print(json.dumps(out))
        return
    torch.manual_seed(3)
    np.random.seed(3)
    args = types.SimpleNamespace(
        device=dev, history_length=2, discount=0.99, multi_step=3, priority_weight=0.4, priority_exponent=0.5, atoms=51,
        V_min=-10.0, V_max=10.0, batch_size=4, norm_clip=10.0, model=None, learning_rate=6.25e-5, adam_eps=1.5e-4,
        architecture="data-efficient", hidden_size=32, noisy_std=0.1)
    agent = Agent(args, types.SimpleNamespace(action_space=lambda: 4))
    mem = ReplayMemory(args, 64, seed=7)
    g = torch.Generator().manual_seed(5)
    for i in range(48):
        mem.append(torch.rand(2, 84, 84, generator=g).to(dev), i % 4, float(i % 3 - 1), i % 17 == 16)
    stream = io.BytesIO()
    mem.save_to(stream)
    blob = pickle.dumps(mem)
    with open(os.path.join(work, "replay.stream"), "wb") as f:
        f.write(stream.getvalue())
    with open(os.path.join(work, "replay.pkl"), "wb") as f:
        f.write(blob)
    out = {"save_to": _sha(stream.getvalue()), "pickle": _sha(blob), "replay": _replay_digest(mem)}
    losses = []
    for step in range(6):
        if step % 2 == 0:
            agent.reset_noise()
        agent.learn(mem)
        losses.append(_sha(agent._loss))
    states = torch.rand(5, 2, 84, 84, generator=g).to(dev)
    out["act"] = int(agent.act(states[0]))
    out["act_batch"] = [int(a) for a in agent.act_batch(states)]
    st = agent.optimiser.state_dict()["state"][0]
    out.update(loss=losses, params=_sha(agent.params), target_params=_sha(agent.target_params), exp_avg=_sha(st["exp_avg"]),
               exp_avg_sq=_sha(st["exp_avg_sq"]), adam_step=float(st["step"]), tree=_sha(mem._dump()["tree"]))
    print(json.dumps(out))


def _child(root, work, env, foreign=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--record", root, "--work", work] + (["--foreign", foreign] if foreign else [])
    res = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(cmd), res.returncode, res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "host_split_identity.txt"))
    ap.add_argument("--work", default=None, help="where the two trees write their replay files (default: a temporary directory)")
    ap.add_argument("--record")
    ap.add_argument("--foreign")
    opt = ap.parse_args()
    if opt.record:
        return record(opt.record, opt.work, opt.foreign)
    if not opt.parent:
        ap.error("--parent: a checkout of the commit to compare against (with its library built)")
    opt.work = opt.work or tempfile.mkdtemp(prefix="host_split_identity_")
    lines, ok = [], True
    for env in SWITCHES:
        tag = " ".join("%s=%s" % kv for kv in env.items()) or "defaults"
        got = {}
        for name, root in (("parent", os.path.abspath(opt.parent)), ("new", HERE)):
            work = os.path.join(opt.work, name)
            os.makedirs(work, exist_ok=True)
            got[name] = _child(root, work, env)
        for key in got["parent"]:
            same = got["parent"][key] == got["new"][key]
            ok &= same
            lines.append("%-28s %-14s %s  %s" % (tag, key, "equal" if same else "DIFFERENT",
                                                 json.dumps(got["new"][key]) if same else json.dumps([got["parent"][key], got["new"][key]])))
        if not env:       # each tree loads what the other wrote: the replay that comes back is the one that was saved
            for name, root, other in (("parent", os.path.abspath(opt.parent), "new"), ("new", HERE, "parent")):
                back = _child(root, os.path.join(opt.work, name), env, foreign=os.path.join(opt.work, other))
                for how, dig in back.items():
                    same = dig == got[other]["replay"]
                    ok &= same
                    lines.append("%-28s %-14s %s  (%s loads %s's)" % (tag, how, "equal" if same else "DIFFERENT", name, other))
    lines.append("RESULT: " + ("every figure bit-equal between parent and new" if ok else "MISMATCH"))
    text = "\n".join(lines) + "\n"
    with open(opt.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
