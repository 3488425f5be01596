"""One group of tests/poison_run.py under RB_GUARD=1 and then RB_GUARD=2, each in a child process (RB_GUARD is read when the
library first allocates), and the comparison of what the two wrote: shared by test_poison_emu.py and test_poison_gpu.py."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(where, group, level, out_dir, timeout):
    """-> the child's JSON.  Asserts exit 0 and that no guard band, the library's or the caller's, was overwritten."""
    out = os.path.join(str(out_dir), "%s_%s_%d.json" % (where, group, level))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "poison_run.py"), where, group, out],
                       env=dict(os.environ, RB_GUARD=str(level)), cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0 and "poison run ok" in p.stdout, \
        "RB_GUARD=%d %s %s: exit %d\n%s\n%s" % (level, where, group, p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    with open(out) as f:
        res = json.load(f)
    assert res["level"] == level and res["guards"], (level, res["level"], len(res["guards"]))
    bad = [g for g in res["guards"] if g["lib_bad"] or g["caller_bad"]]
    assert not bad, "RB_GUARD=%d %s %s: overwritten guard bands: %s" % (level, where, group, bad[:4])
    return res


def same_digests(a, b, what):
    """Key by key; a mismatch names the tensors."""
    da, db = a["digests"], b["digests"]
    assert da, "%s: nothing was digested" % what
    assert sorted(da) == sorted(db), "%s: the two runs digested different tensors: %s" % (what, sorted(set(da) ^ set(db))[:12])
    diff = [k for k in sorted(da) if da[k] != db[k]]
    assert not diff, "%s: %d of %d tensors differ between the two runs; the first: %s" % (what, len(diff), len(da), diff[:24])


def run_pair(where, group, out_dir, timeout):
    """The group on zero-filled and then on poison-filled allocations (the second child is not started if the first failed):
    bit-identical outputs.  -> (zeroed run, poisoned run)."""
    zeroed = run_child(where, group, 1, out_dir, timeout)
    poisoned = run_child(where, group, 2, out_dir, timeout)
    same_digests(zeroed, poisoned, "%s %s, RB_GUARD=1 against RB_GUARD=2" % (where, group))
    assert [g["case"] for g in zeroed["guards"]] == [g["case"] for g in poisoned["guards"]]
    print("%s %s: %d tensors of %d cases identical; RB_GUARD=1 %.1f s, RB_GUARD=2 %.1f s"
          % (where, group, len(zeroed["digests"]), len(zeroed["guards"]), zeroed["seconds"], poisoned["seconds"]))
    return zeroed, poisoned
