"""CPU check of the hosted optimiser pass's gfx950 code (adam_body.h): its arguments reach it in scalar registers, so no buffer
access of the pass sits in a waterfall loop.

A waterfall loop is what the compiler wraps around a buffer access whose descriptor it could not prove wave-uniform: a block
that branches back to itself and contains v_readfirstlane_b32 (one lane's descriptor into SGPRs), s_and_saveexec_b64 (the lanes
that share it) and the buffer_ access.  With ClipAdamArgs fetched by vector loads every load and store of the pass was one
(profiles/hosted_pass_isa.txt: 19 such blocks in k_adam_pending, 113 in the hosting sampler kernel).  k_adam_pending is the
hosted body and nothing else, so it is the kernel looked at; the learner's unit is compiled the way tests/test_abi.py does."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_body(asm_path, name):
    """The instruction lines (comments stripped) between `name:` and its .Lfunc_end."""
    body, inside = [], False
    for line in open(asm_path):
        if not inside:
            inside = line.startswith(name + ":")
            continue
        if line.startswith(".Lfunc_end"):
            return body
        body.append(line.split(";")[0].rstrip())
    return body if inside else None


def basic_blocks(body):
    """[(label, lines)] of the blocks that carry a label."""
    out, label, cur = [], None, []
    for line in body:
        m = re.match(r"^(\.LBB[0-9_]+):", line)
        if m:
            if label is not None:
                out.append((label, cur))
            label, cur = m.group(1), []
        else:
            cur.append(line)
    if label is not None:
        out.append((label, cur))
    return out


def waterfall_blocks(body):
    found = []
    for label, lines in basic_blocks(body):
        loops = any(re.search(r"\bs_cbranch_\w+\s+" + re.escape(label) + r"\s*$", ln) for ln in lines)
        if (loops and any("v_readfirstlane_b32" in ln for ln in lines) and any("s_and_saveexec_b64" in ln for ln in lines)
                and any(re.search(r"\bbuffer_(load|store|atomic)", ln) for ln in lines)):
            found.append(label)
    return found


def test_the_detector_finds_a_waterfall_block():
    """(so that an assembler syntax the pattern no longer matches cannot pass for 'no waterfall block')"""
    body = """
.LBB7_3:
	v_readfirstlane_b32 s4, v10
	v_readfirstlane_b32 s5, v11
	v_readfirstlane_b32 s6, v12
	v_readfirstlane_b32 s7, v13
	v_cmp_eq_u64_e32 vcc, s[4:5], v[10:11]
	v_cmp_eq_u64_e64 s[0:1], s[6:7], v[12:13]
	s_and_b64 s[0:1], vcc, s[0:1]
	s_and_saveexec_b64 s[0:1], s[0:1]
	buffer_load_dwordx4 v[2:5], v1, s[4:7], 0 offen
	s_xor_b64 exec, exec, s[0:1]
	s_cbranch_execnz .LBB7_3
.LBB7_4:
	buffer_load_dwordx4 v[2:5], v1, s[4:7], 0 offen
	s_cbranch_execnz .LBB7_3
""".splitlines()
    assert waterfall_blocks(body) == [".LBB7_3"]


def test_no_waterfall_block_in_the_pending_pass():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rainbow_amd", "csrc", "learner.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "learner.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                               src, "-o", out], stderr=subprocess.DEVNULL)
        body = kernel_body(out, "k_adam_pending")
    assert body, "k_adam_pending is not in the learner's unit"
    loads = sum(bool(re.search(r"\bbuffer_load_dwordx4\b", ln)) for ln in body)
    stores = sum(bool(re.search(r"\bbuffer_store_dwordx4\b", ln)) for ln in body)
    assert loads >= 16 + 14 and stores >= 12 + 14, ("the pass's quad accesses must be there to be judged", loads, stores)
    assert waterfall_blocks(body) == []
