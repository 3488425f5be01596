"""Which kernel a shape reaches, pinned: rb_debug_launch_plan prints the plans of csrc/learner_plan.h — the very functions the
launchers call — and this file holds them against the project's own record: the kernel tables of DESIGN.md sections 3 and 8, the
kernel names of profiles/round6_final_cfg{2,3,4}_kernel_stats.csv, and the workgroup counts DESIGN.md and the code comments state
(480 / 224 / 249 workgroups, 7 / 7 / 8 images, 48 tiles x split-K 5, 13 waves, ...).  No device: the entry touches none, and it
is called here through the host-interpreter build with 256 compute units, the MI355X's count.  The GPU parity tests cannot see a
step that silently falls back to a slower kernel; this can."""
import csv
import ctypes as C
import os
import re

import pytest

from hipemu import loader
from rainbow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_FLAGS = _lib.LEARNER_DEFER_UPDATE | _lib.LEARNER_IMPLICIT_SIGMA      # what Agent sets on one device (agent.py)


@pytest.fixture(scope="module")
def emu():
    return loader.load()


def plan(lib, batch=32, atoms=51, actions=6, history=4, hidden=512, architecture=0, opts=None, flags=DEFAULT_FLAGS, world=1,
         sink=1, cap=1 << 14):
    """-> {tag: {"kernel": str, "grid": (x, y, z), "block": int, key: int, ...}} in launch order."""
    cfg = _lib.LearnerConfig(batch=batch, atoms=atoms, actions=actions, history=history, hidden=hidden, architecture=architecture,
                             multi_step=3, v_min=-10.0, v_max=10.0, discount=0.99)
    buf = C.create_string_buffer(cap)
    rc = lib.rb_debug_launch_plan(C.byref(cfg), opts.encode() if opts else None, 256, flags, world, sink, buf, cap)
    assert rc == 0, lib.rb_last_error()
    out = {}
    for line in buf.value.decode().splitlines():
        tag, *fields = line.split(" ")
        row = {}
        for f in fields:
            k, v = f.split("=", 1)
            if k == "kernel":
                row[k] = v
            elif k == "grid":
                row[k] = tuple(int(x) for x in v.split("x"))
            elif "/" in v:
                row[k] = tuple(int(x) for x in v.split("/"))
            elif "x" in v:
                row[k] = tuple(int(x) for x in v.split("x"))
            else:
                row[k] = int(v)
        assert tag not in out, tag
        out[tag] = row
    return out


def wgs(row):
    g = row["grid"]
    return g[0] * g[1] * g[2]


def base(kernel):
    return kernel.split("<")[0]


CANONICAL = dict()                                                   # config 2: B 32, A 6
B256 = dict(batch=256, actions=4)                                    # config 3
DATA_EFF = dict(architecture=1, hidden=256)                          # config 4


def recorded_kernels(cfg):
    """Base names of the library's kernels in the recorded rocprofv3 statistics of a config."""
    names = set()
    with open(os.path.join(ROOT, "profiles", "round6_final_cfg%d_kernel_stats.csv" % cfg)) as f:
        for row in csv.DictReader(f):
            m = re.match(r"(?:void )?(k_[a-z0-9_]+)", row["Name"])
            if m:
                names.add(m.group(1))
    return names


# ---------------------------------------------------------------------------------------- the three benchmark configs
def test_canonical_batch_32_reaches_the_kernels_of_design_3_1(emu):
    p = plan(emu, **CANONICAL)
    for i in (1, 2, 3):
        assert base(p["conv%d_fwd" % i]["kernel"]) == "k_conv_fwd_t16"
        assert p["conv%d_fwd" % i]["img_fast"] == 1
    assert wgs(p["conv1_fwd"]) == 480 and p["conv1_fwd"]["grid"][0] == 96          # 5 x 96, the image index fastest
    assert p["fc_h_fwd"]["kernel"] == "k_nl_fwd3<2>" and p["fc_z_fwd"]["kernel"] == "k_nl_fwd3<2>"
    assert p["head"]["kernel"] == "k_head<1>" and p["head"]["grid"] == (32 + 96, 1, 1) and p["head"]["waves"] == 13
    assert p["head"]["samples"] == 32 and p["head"]["tenants"] == 96 and p["head"]["block"] == 64 * 13
    assert p["fc_z_bwd"]["kernel"] == "k_nl_bwd<true>"
    assert p["fc_h_bwd"]["kernel"] == "k_nl_bwd<false>" and p["fc_h_bwd"]["writeback"] == 1
    assert p["conv3_dx"]["kernel"] == "k_conv_dx_lds<GeomC3,MULTI=false>"
    assert p["conv2_dx"]["kernel"] == "k_conv_dx_lds<GeomC2,MULTI=false>"
    assert p["conv_dw_all"]["kernel"] == "k_conv_dw_all<3>" and p["conv_dw_all"]["nblocks"] == (96, 64, 64)
    assert wgs(p["conv_dw_all"]) == 224
    assert p["fc_h_bwd"]["implicit_sigma"] == 1 and p["fc_h_bwd"]["fuse_norm"] == 1 and p["fc_h_bwd"]["defer_dw"] == 0
    assert "dfeat_finish" not in p and "pack_factors" not in p
    # without a sink there is no write-back block
    q = plan(emu, sink=0, **CANONICAL)
    assert q["fc_h_bwd"]["writeback"] == 0 and wgs(q["fc_h_bwd"]) == wgs(p["fc_h_bwd"]) - 1
    # without the flag the sigma gradient is stored
    assert plan(emu, flags=0, **CANONICAL)["fc_h_bwd"]["implicit_sigma"] == 0


def test_batch_256_reaches_the_kernels_of_design_3_2(emu):
    p = plan(emu, **B256)
    assert p["conv1_fwd"]["kernel"] == "k_conv_fwd_full<GeomC1>" and p["conv1_fwd"]["ipb"] == 3 and wgs(p["conv1_fwd"]) == 256
    for i in (2, 3):
        r = p["conv%d_fwd" % i]
        assert base(r["kernel"]) == "k_conv_fwd_multi_t16" and r["ipb"] == 6 and r["img_fast"] == 1
        assert r["grid"][0] == 768 // 6                                              # the image GROUP index fastest
    assert p["fc_h_fwd"]["kernel"] == "k_fc_gemm_fwd" and p["fc_h_fwd"]["tiles"] == 48 and p["fc_h_fwd"]["S"] == 5
    assert wgs(p["fc_h_fwd"]) == 240
    assert p["fc_z_fwd"]["kernel"] == "k_nl_fwd3<4>"
    assert p["fc_z_bwd"]["kernel"] == "k_nl_bwd<false>"
    assert p["fc_h_bwd"]["kernel"] == "k_fc_gemm_bwd" and wgs(p["fc_h_bwd"]) == 416
    assert p["conv3_dx"]["kernel"] == "k_conv_dx_t16_multi<GeomC3>" and p["conv2_dx"]["kernel"] == "k_conv_dx_t16_multi<GeomC2>"
    assert p["conv3_dx"]["wt_t16"] == 1 and p["head"]["wt_t16"] == (1, 1)           # the tenants write the layout the kernel reads
    assert p["conv_dw_all"]["ipb"] == (7, 7, 8) and wgs(p["conv_dw_all"]) == 249
    assert p["fc_h_bwd"]["implicit_sigma"] == 1                                      # (the tiled GEMM carries it too)


def test_data_efficient_reaches_the_kernels_of_design_3_3(emu):
    p = plan(emu, **DATA_EFF)
    assert p["conv1_fwd"]["kernel"] == "k_conv_fwd_lds<GeomD1>" and p["conv2_fwd"]["kernel"] == "k_conv_fwd_lds<GeomD2>"
    assert "conv3_fwd" not in p
    assert p["conv2_dx"]["kernel"] == "k_conv_dx_lds<GeomD2,MULTI=false>"
    assert p["conv_dw_all"]["kernel"] == "k_conv_dw_all<2>" and p["conv_dw_all"]["nblocks"][2] == 0
    # 2 * 256 * 576 = 0.3 M elements: under the 1 M threshold of the pairing
    assert p["fc_h_bwd"]["implicit_sigma"] == 0
    assert plan(emu, opts="implicit_small=1", **DATA_EFF)["fc_h_bwd"]["implicit_sigma"] == 1


@pytest.mark.parametrize("cfg,kw", [(2, CANONICAL), (3, B256), (4, DATA_EFF)])
def test_every_planned_kernel_is_in_the_recorded_profile_of_its_config(emu, cfg, kw):
    recorded = recorded_kernels(cfg)
    p = plan(emu, **kw)
    for tag, row in p.items():
        if tag == "caps" or tag.startswith("act_"):
            continue
        assert base(row["kernel"]) in recorded, (tag, row["kernel"])
    # and the other way round: every step kernel of the learner that the profile shows is one the plan names
    step = {"k_conv_fwd_t16", "k_conv_fwd_full", "k_conv_fwd_multi_t16", "k_conv_fwd_lds", "k_nl_fwd3", "k_fc_gemm_fwd", "k_head",
            "k_nl_bwd", "k_fc_gemm_bwd", "k_conv_dx_lds", "k_conv_dx_t16_multi", "k_conv_dw_all", "k_reduce_conv_dw_all"}
    planned = {base(r["kernel"]) for t, r in p.items() if t != "caps" and not t.startswith("act_")}
    assert recorded & step == planned


# ------------------------------------------------------------------------------------------------------ the thresholds
def test_conv_forward_image_loop_starts_at_256_images(emu):
    lo, hi = plan(emu, batch=85), plan(emu, batch=86)                                # 255 / 258 images
    assert [base(lo["conv%d_fwd" % i]["kernel"]) for i in (1, 2, 3)] == ["k_conv_fwd_t16"] * 3
    assert all(lo["conv%d_fwd" % i]["ipb"] == 1 for i in (1, 2, 3))
    assert [base(hi["conv%d_fwd" % i]["kernel"]) for i in (1, 2, 3)] == ["k_conv_fwd_full", "k_conv_fwd_multi_t16", "k_conv_fwd_multi_t16"]
    assert all(hi["conv%d_fwd" % i]["ipb"] > 1 for i in (1, 2, 3))


def test_batch_64_conv_input_gradient_image_loop_and_the_forward_only_gemm(emu):
    lo, hi = plan(emu, batch=63), plan(emu, batch=64)
    for i in (2, 3):
        assert base(lo["conv%d_dx" % i]["kernel"]) == "k_conv_dx_lds" and lo["conv%d_dx" % i]["ipb"] == 1
        assert base(hi["conv%d_dx" % i]["kernel"]) == "k_conv_dx_t16_multi"
    assert lo["head"]["wt_t16"] == (0, 0) and hi["head"]["wt_t16"] == (1, 1)
    # the forward's online net carries 2B rows, the backward B: from 64 to 127 only the forward is on the tiled GEMM
    assert lo["fc_h_fwd"]["kernel"] == "k_nl_fwd3<2>" and lo["fc_h_bwd"]["kernel"] == "k_nl_bwd<false>"
    assert hi["fc_h_fwd"]["kernel"] == "k_fc_gemm_fwd" and hi["fc_h_bwd"]["kernel"] == "k_nl_bwd<false>"
    assert hi["fc_h_bwd"]["gemm_bwd"] == 0


@pytest.mark.parametrize("batch", [86, 100, 129, 257])
def test_batches_without_a_multiple_of_8_groups_get_one_image_group(emu, batch):
    """No images-per-workgroup count at or above the one-round estimate divides these batches into a multiple of 8 groups, and
    round_ipb_to_groups_of_8 counts on to the batch itself: ONE image group, 2 to 25 workgroups that walk the whole batch with their
    weight slab resident.  Keeping the one-round estimate instead (86 / 43 groups at batch 86, ...) was measured and is no faster —
    profiles/dx_group_rounding.txt: batch 100 +1 .. +3.5 us per step, batch 257 equal — so the plan stays; at default options the
    image loops of the data-gradient kernels therefore never see a SHORT last group, and tests/test_learner_batches_gpu.py
    reaches one through RB_OPTS dx_ipb, pinned here as well."""
    ceil = lambda a, b: -(-a // b)
    p = plan(emu, batch=batch)
    for tag, phases, cit in (("conv3_dx", 1, 2), ("conv2_dx", 4, 1)):
        r = p[tag]
        assert base(r["kernel"]) == "k_conv_dx_t16_multi" and r["ipb"] == batch and r["img_fast"] == 0 and r["grid"] == (phases, cit, 1), (tag, r)
    d = plan(emu, batch=batch, **DATA_EFF)["conv2_dx"]
    assert d["kernel"] == "k_conv_dx_lds<GeomD2,MULTI=true>" and d["ipb"] == batch and d["img_fast"] == 0 and d["grid"] == (25, 1, 1), d
    for ipb in (2, 5):      # the hook: the count as given, (phase, tile, group) order, a short last group
        q = plan(emu, batch=batch, opts="dx_ipb=%d" % ipb)
        for tag in ("conv3_dx", "conv2_dx"):
            assert q[tag]["ipb"] == ipb and q[tag]["grid"][2] == ceil(batch, ipb) and q[tag]["img_fast"] == (1 if batch % ipb == 0 and (batch // ipb) % 8 == 0 else 0)
        e = plan(emu, batch=batch, opts="dx_ipb=%d" % ipb, **DATA_EFF)["conv2_dx"]
        assert e["kernel"] == "k_conv_dx_lds<GeomD2,MULTI=true>" and e["ipb"] == ipb and e["grid"][2] == ceil(batch, ipb)
    if batch == 129:      # dx_ipb=2: 64 groups of two images and one of a single image
        assert plan(emu, batch=129, opts="dx_ipb=2")["conv3_dx"]["grid"] == (1, 2, 65)


@pytest.mark.parametrize("batch,c3,c2,d2", [(64, (1, 64), (1, 64), (8, 8)), (128, (1, 128), (2, 64), (16, 8)), (200, (5, 40), (5, 40), (25, 8)),
                                            (256, (2, 128), (4, 64), (32, 8)), (320, (4, 80), (5, 64), (40, 8)),
                                            (1024, (8, 128), (16, 64), (128, 8))])
def test_batches_with_a_multiple_of_8_groups_are_rounded_to_them(emu, batch, c3, c2, d2):
    """(images per workgroup, groups) of the data-gradient launches where the rounding exists: image-group-fastest order."""
    p, d = plan(emu, batch=batch), plan(emu, batch=batch, **DATA_EFF)
    for r, (ipb, ng) in ((p["conv3_dx"], c3), (p["conv2_dx"], c2), (d["conv2_dx"], d2)):
        assert r["ipb"] == ipb and r["img_fast"] == 1 and r["grid"][0] == ng and ipb * ng == batch, r


def test_backward_gemm_starts_at_batch_128(emu):
    lo, hi = plan(emu, batch=127), plan(emu, batch=128)
    assert lo["fc_h_fwd"]["kernel"] == "k_fc_gemm_fwd" and lo["fc_h_bwd"]["kernel"] == "k_nl_bwd<false>" and lo["fc_h_bwd"]["gemm_bwd"] == 0
    assert hi["fc_h_fwd"]["kernel"] == "k_fc_gemm_fwd" and hi["fc_h_bwd"]["kernel"] == "k_fc_gemm_bwd" and hi["fc_h_bwd"]["gemm_bwd"] == 1


def test_batch_32_is_the_last_on_the_pipelined_and_tall_bodies(emu):
    lo, hi = plan(emu, batch=32), plan(emu, batch=33)
    assert lo["fc_z_bwd"]["pipe"] == 1 and lo["fc_z_bwd"]["z_tall"] == 1 and lo["fc_z_bwd"]["kernel"] == "k_nl_bwd<true>"
    assert lo["fc_z_bwd"]["z_ct"] == 2 and lo["fc_h_bwd"]["h_ct"] == 4
    assert hi["fc_z_bwd"]["pipe"] == 0 and hi["fc_z_bwd"]["z_tall"] == 0 and hi["fc_z_bwd"]["kernel"] == "k_nl_bwd<false>"
    assert hi["fc_z_bwd"]["z_ct"] == 0 and hi["fc_h_bwd"]["h_ct"] == 0
    # neither the pipelined body nor the tiled GEMM: the sigma gradient is stored
    assert hi["fc_h_bwd"]["implicit_sigma"] == 0
    # weight gradients: one image per workgroup up to 32, from 33 on the per-layer search.  At 33 images one image per workgroup
    # is 3 * 33 + 2 * 33 + 2 * 33 = 231 workgroups, within one round of 256, and no choice has a shorter longest workgroup; the
    # uniform count would be ceil(33 / 32) = 2, so the launch loses the image-fastest decode
    assert lo["conv_dw_all"]["ipb"] == (1, 1, 1) and lo["conv_dw_all"]["img_fast"] == 1 and wgs(lo["conv_dw_all"]) == 224
    assert hi["conv_dw_all"]["ipb"] == (1, 1, 1) and hi["conv_dw_all"]["img_fast"] == 0 and wgs(hi["conv_dw_all"]) == 231


def test_short_and_long_histories(emu):
    p3 = plan(emu, history=3)
    assert p3["conv1_fwd"]["kernel"] == "k_conv_fwd_lds<GeomC1>"                     # K = 192: not the whole-K tile's 256
    assert base(p3["conv2_fwd"]["kernel"]) == "k_conv_fwd_t16"
    p5 = plan(emu, history=5)                                                        # no LDS conv kernel beyond history 4
    for i in (1, 2, 3):
        assert base(p5["conv%d_fwd" % i]["kernel"]) == "k_gemm"
    assert base(p5["conv3_dx"]["kernel"]) == "k_gemm" and base(p5["conv2_dx"]["kernel"]) == "k_gemm"
    assert base(p5["conv1_dw"]["kernel"]) == "k_gemm" and "conv_dw_all" not in p5
    assert p5["fc_h_fwd"]["kernel"] == "k_nl_fwd3<2>" and p5["fc_h_bwd"]["kernel"] == "k_nl_bwd<false>"    # FC still streamed
    assert "feat_block_copy" in p5 and "dfeat_finish" in p5 and p5["head"]["tenants"] == 0


def test_one_row_f32_forward(emu):
    p = plan(emu)
    assert p["act_conv1_fwd"]["kernel"] == "k_conv_fwd_lds<GeomC1,F32SRC>"
    assert base(p["act_conv2_fwd"]["kernel"]) == "k_conv_fwd_t16" and base(p["act_conv3_fwd"]["kernel"]) == "k_conv_fwd_t16"
    assert p["act_fc_h_fwd"]["kernel"] == "k_nl_fwd3<2>" and p["act_fc_z_fwd"]["kernel"] == "k_nl_fwd3<2>"
    assert p["act_conv1_fwd"]["img_fast"] == 0                                       # one image: no multiple of 8
    d = plan(emu, **DATA_EFF)
    assert d["act_conv1_fwd"]["kernel"] == "k_conv_fwd_lds<GeomD1,F32SRC>"


@pytest.mark.parametrize("atoms,zi", [(51, 1), (64, 1), (65, 2), (128, 2), (129, 4)])
def test_head_instantiation_follows_the_atom_count(emu, atoms, zi):
    assert plan(emu, atoms=atoms)["head"]["kernel"] == "k_head<%d>" % zi


# ------------------------------------------------------------------------------------------------ RB_OPTS
def test_rb_opts_keys_reach_the_kernels_design_8_names(emu):
    g1 = plan(emu, opts="generic=1")                                                 # every contraction on the fallback
    for tag in ("conv1_fwd", "conv2_fwd", "conv3_fwd", "fc_h_fwd", "fc_z_fwd", "fc_z_dw", "fc_z_dx", "fc_h_dw", "fc_h_dx", "conv3_dx",
                "conv2_dx", "conv1_dw", "conv2_dw", "conv3_dw"):
        assert base(g1[tag]["kernel"]) == "k_gemm", tag
    g2 = plan(emu, opts="generic=2")                                                 # the noisy-linear layers only
    assert base(g2["conv1_fwd"]["kernel"]) == "k_conv_fwd_t16" and "conv_dw_all" in g2
    for tag in ("fc_h_fwd", "fc_z_fwd", "fc_z_dw", "fc_z_dx", "fc_h_dw", "fc_h_dx"):
        assert base(g2[tag]["kernel"]) == "k_gemm", tag
    f0 = plan(emu, opts="fc_gemm=0", **B256)
    assert f0["fc_h_fwd"]["kernel"] == "k_nl_fwd3<4>" and f0["fc_h_bwd"]["kernel"] == "k_nl_bwd<false>"
    f1 = plan(emu, opts="fc_gemm=1")
    assert f1["fc_h_fwd"]["kernel"] == "k_fc_gemm_fwd" and f1["fc_h_bwd"]["kernel"] == "k_fc_gemm_bwd"
    c0 = plan(emu, opts="conv_full=0", **B256)                                       # the chunked kernel
    assert c0["conv1_fwd"]["kernel"] == "k_conv_fwd_t16<GeomC1>"
    assert base(c0["conv2_fwd"]["kernel"]) == "k_conv_fwd_multi_t16"
    t0 = plan(emu, opts="t16=0")                                                     # the split-K kernel that history < 4 gets
    assert t0["conv1_fwd"]["kernel"] == "k_conv_fwd_lds<GeomC1>" and base(t0["conv2_fwd"]["kernel"]) == "k_conv_fwd_t16"
    i0 = plan(emu, opts="img_fast=0")
    for tag in ("conv1_fwd", "conv2_fwd", "conv3_fwd", "conv3_dx", "conv2_dx", "conv_dw_all"):
        assert i0[tag]["img_fast"] == 0, tag
    assert i0["conv1_fwd"]["grid"] == (5, 1, 96)                                     # the image index slowest
    d2 = plan(emu, opts="dx_ipb=2")
    assert d2["conv3_dx"]["kernel"] == "k_conv_dx_t16_multi<GeomC3>" and d2["conv3_dx"]["ipb"] == 2
    assert d2["conv2_dx"]["kernel"] == "k_conv_dx_t16_multi<GeomC2>" and d2["head"]["wt_t16"] == (1, 1)
    e2 = plan(emu, opts="dx_ipb=2", **DATA_EFF)
    assert e2["conv2_dx"]["kernel"] == "k_conv_dx_lds<GeomD2,MULTI=true>" and e2["conv2_dx"]["ipb"] == 2
    m0 = plan(emu, opts="conv_multi=0", **B256)                                      # one image per workgroup
    assert [base(m0["conv%d_fwd" % i]["kernel"]) for i in (1, 2, 3)] == ["k_conv_fwd_t16"] * 3
    w = plan(emu, opts="dw_ipb0=2,dw_ipb1=4,dw_ipb2=8")
    assert w["conv_dw_all"]["ipb"] == (2, 4, 8)
    assert plan(emu, opts="xs=2")["fc_h_bwd"]["hsplits"] == 2


def test_replica_exchange_defers_the_fc_weight_gradients(emu):
    p = plan(emu, world=2)
    assert "pack_factors" in p and p["fc_z_bwd"]["dw"] == (0, 0) and p["fc_h_bwd"]["dw"] == (0, 0)
    assert p["fc_h_bwd"]["fuse_norm"] == 0 and p["fc_h_bwd"]["implicit_sigma"] == 0 and p["fc_z_bwd"]["pipe"] == 0


# table B of tests/exchange_scenarios.py, world 2: what each row reaches with the exchange armed (tag.field: value, as below)
EXCHANGE_PINS = {
    "e-d-w2": {"fc_z_bwd.kernel": "k_nl_bwd<true>", "fc_z_bwd.z_tall": 1, "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_fwd.kernel": "k_nl_fwd3<2>",
               "fc_h_bwd.hsplits": 1, "fc_h_bwd.lazy_dfeat": 1, "head.kernel": "k_head<1>"},
    "e-d-w3-b33": {"fc_z_bwd.kernel": "k_nl_bwd<false>", "fc_z_bwd.z_tall": 0, "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_fwd.kernel": "k_nl_fwd3<2>"},
    "e-d-w2-b129": {"fc_z_bwd.kernel": "k_nl_bwd<false>", "fc_z_bwd.z_tall": 0, "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_bwd.gemm_bwd": 0,
                    "fc_h_fwd.kernel": "k_fc_gemm_fwd", "fc_h_bwd.dx": (9, 1, 3)},
    "e-d-w2-h160": {"fc_z_bwd.kernel": "k_nl_bwd<true>", "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_fwd.kernel": "k_nl_fwd3<2>", "fc_h_bwd.hsplits": 2,
                    "fc_h_bwd.lazy_dfeat": 1},
    "e-c-w2": {"fc_z_bwd.kernel": "k_nl_bwd<true>", "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_fwd.kernel": "k_nl_fwd3<2>", "caps.fast_conv": 1,
               "conv_dw_all.kernel": "k_conv_dw_all<3>"},
    "e-c-w2-hist8": {"fc_z_bwd.kernel": "k_nl_bwd<true>", "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_fwd.kernel": "k_nl_fwd3<2>", "caps.fast_conv": 0,
                     "conv1_fwd.kernel": "k_gemm<ConvFwdProb<GeomC1>>", "feat_block_copy.kernel": "k_block_copy", "dfeat_finish.splits": 1,
                     "fc_h_bwd.lazy_dfeat": 0},
    "e-d-w2-z65-a8": {"fc_z_bwd.kernel": "k_nl_bwd<true>", "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_fwd.kernel": "k_nl_fwd3<2>", "head.kernel": "k_head<2>"},
}


def exchange_plan(lib, case, flags=0):
    import exchange_scenarios as ES
    c = ES.case_config(case)
    return plan(lib, batch=c["batch"], atoms=c["atoms"], actions=c["actions"], history=c["history"], hidden=c["hidden"],
                architecture=0 if c["architecture"] == "canonical" else 1, flags=flags, world=2, cap=1 << 15)


def test_every_row_of_the_exchange_learn_table_is_pinned():
    import exchange_scenarios as ES
    assert set(EXCHANGE_PINS) == set(ES.LEARN_CASES)


@pytest.mark.parametrize("case", sorted(EXCHANGE_PINS))
def test_exchange_learn_table_reaches_what_each_row_claims(emu, case):
    """Every row: k_pack_factors in the step, no weight-gradient tiles in either backward launch, no pipelined body, tiled backward
    GEMM, fused norm or implicit sigma — and the flags Agent sets on one device change nothing."""
    import exchange_scenarios as ES
    p = exchange_plan(emu, case)
    assert "pack_factors" in p and p["fc_z_bwd"]["dw"] == (0, 0) and p["fc_h_bwd"]["dw"] == (0, 0), (case, p["fc_z_bwd"], p["fc_h_bwd"])
    assert p["fc_z_bwd"]["pipe"] == 0 and p["fc_h_bwd"]["gemm_bwd"] == 0 and p["fc_h_bwd"]["fuse_norm"] == 0
    assert p["fc_h_bwd"]["implicit_sigma"] == 0 and p["fc_h_bwd"]["defer_dw"] == 0
    for key, want in EXCHANGE_PINS[case].items():
        tag, _, field = key.partition(".")
        assert tag in p and p[tag][field] == want, (case, key, p.get(tag), want)
    assert exchange_plan(emu, case, flags=ES.AGENT_FLAGS) == p


def test_bad_arguments_are_refused_with_a_message(emu):
    cfg = _lib.LearnerConfig(batch=32, atoms=51, actions=6, history=4, hidden=512, architecture=0, multi_step=3, v_min=-10.0,
                             v_max=10.0, discount=0.99)
    small = C.create_string_buffer(64)
    assert emu.rb_debug_launch_plan(C.byref(cfg), None, 256, 0, 1, 0, small, 64) == -1      # RB_ERR_INVALID
    assert b"too few" in emu.rb_last_error()
    buf = C.create_string_buffer(1 << 14)
    assert emu.rb_debug_launch_plan(C.byref(cfg), b"no_such_key=1", 256, 0, 1, 0, buf, 1 << 14) < 0
    assert b"no_such_key" in emu.rb_last_error()


# ------------------------------------------------------------- the history / hidden table (tests/shape_range_scenarios.py)
def shape_range_plan(lib, case, flags=0):
    import shape_range_scenarios as SR
    c = SR.case_config(case)
    return plan(lib, batch=c["batch"], atoms=c["atoms"], actions=c["actions"], history=c["history"], hidden=c["hidden"],
                architecture=0 if c["architecture"] == "canonical" else 1, flags=flags, cap=1 << 15)


# row: the plan fields the row's "crosses" column claims — tag.field: value; a tag alone with None: that line is absent
SHAPE_RANGE_PINS = {
    # history < 4: off the whole-K first-layer kernel (canonical), the same split-K kernel part filled (data-efficient)
    "c-hist1": {"caps.fast_conv": 1, "conv1_fwd.kernel": "k_conv_fwd_lds<GeomC1>", "conv_dw_all.kernel": "k_conv_dw_all<3>", "act_path.rg": (6, 9, 7)},
    "c-hist2": {"caps.fast_conv": 1, "conv1_fwd.kernel": "k_conv_fwd_lds<GeomC1>", "conv_dw_all.kernel": "k_conv_dw_all<3>", "act_path.rg": (6, 9, 7)},
    "d-hist1": {"caps.fast_conv": 1, "conv1_fwd.kernel": "k_conv_fwd_lds<GeomD1>", "conv_dw_all.kernel": "k_conv_dw_all<2>", "act_path.rg": (8, 3, 0)},
    "d-hist3": {"caps.fast_conv": 1, "conv1_fwd.kernel": "k_conv_fwd_lds<GeomD1>", "conv_dw_all.kernel": "k_conv_dw_all<2>", "act_path.rg": (8, 3, 0)},
    # history > 4: every conv on k_gemm behind the streamed FC, and the act path's patch limit
    "c-hist8": {"caps.fast_conv": 0, "caps.fast_fc": 1, "conv1_fwd.kernel": "k_gemm<ConvFwdProb<GeomC1>>", "fc_h_fwd.kernel": "k_nl_fwd3<2>",
                "feat_block_copy.kernel": "k_block_copy", "dfeat_finish.splits": 1, "fc_h_bwd.lazy_dfeat": 0, "conv_dw_all": None,
                "act_path.covered": 1, "act_path.rg": (4, 9, 7)},
    "c-hist16": {"caps.fast_conv": 0, "caps.fast_fc": 1, "conv1_fwd.kernel": "k_gemm<ConvFwdProb<GeomC1>>", "fc_h_fwd.kernel": "k_nl_fwd3<2>",
                 "feat_block_copy.kernel": "k_block_copy", "dfeat_finish.splits": 1, "fc_h_bwd.lazy_dfeat": 0, "conv_dw_all": None,
                 "act_path.covered": 1, "act_path.rg": (1, 9, 7)},
    "d-hist16": {"caps.fast_conv": 0, "caps.fast_fc": 1, "conv1_fwd.kernel": "k_gemm<ConvFwdProb<GeomD1>>", "fc_h_fwd.kernel": "k_nl_fwd3<2>",
                 "feat_block_copy.kernel": "k_block_copy", "dfeat_finish.splits": 1, "fc_h_bwd.lazy_dfeat": 0, "conv_dw_all": None,
                 "act_path.covered": 1, "act_path.rg": (2, 3, 0)},
    # hidden 1 / 3: generic FC, and rb_learner_act on the training forward
    "d-h1": {"caps.fast_fc": 0, "caps.fast_conv": 1, "fc_h_fwd.kernel": "k_gemm", "fc_h_dx.kernel": "k_gemm<FcHDxProb>", "fc_h_bwd": None,
             "act_path.covered": 0},
    "d-h3": {"caps.fast_fc": 0, "caps.fast_conv": 1, "fc_h_fwd.kernel": "k_gemm", "fc_h_dx.kernel": "k_gemm<FcHDxProb>", "fc_h_bwd": None,
             "act_path.covered": 0},
    # row splits of the hidden layer's input gradient, summed by the last conv layer's backward kernels (lazy_dfeat)
    "d-h128": {"caps.fast_fc": 1, "caps.xs": 1, "fc_h_bwd.hsplits": 1, "fc_h_bwd.rows_per_split": 256, "fc_h_bwd.lazy_dfeat": 1},
    "d-h160": {"caps.fast_fc": 1, "caps.xs": 2, "fc_h_bwd.hsplits": 2, "fc_h_bwd.rows_per_split": 160, "fc_h_bwd.lazy_dfeat": 1},
    "d-h288": {"caps.fast_fc": 1, "caps.xs": 3, "fc_h_bwd.hsplits": 3, "fc_h_bwd.rows_per_split": 192, "fc_h_bwd.lazy_dfeat": 1},
    "d-h352": {"caps.fast_fc": 1, "caps.xs": 3, "fc_h_bwd.hsplits": 3, "fc_h_bwd.rows_per_split": 240, "fc_h_bwd.lazy_dfeat": 1},    # 240 / 240 / 224
    # both sides of the fast_fc limit, and the accepted maximum
    "d-h4096": {"caps.fast_fc": 1, "caps.xs": 4, "fc_h_fwd.kernel": "k_nl_fwd3<2>", "fc_z_fwd.kernel": "k_nl_fwd3<2>", "fc_h_bwd.kernel": "k_nl_bwd<false>",
                "fc_h_bwd.hsplits": 4, "fc_h_bwd.fuse_norm": 1, "act_path.covered": 1},
    "d-h4128": {"caps.fast_fc": 0, "caps.xs": 52, "fc_h_fwd.kernel": "k_gemm", "fc_z_fwd.kernel": "k_gemm", "fc_h_dx.kernel": "k_gemm<FcHDxProb>",
                "dfeat_finish.splits": 52, "fc_h_bwd": None, "act_path.covered": 0},
    "d-h8192": {"caps.fast_fc": 0, "caps.xs": 54, "fc_h_fwd.kernel": "k_gemm", "fc_z_fwd.kernel": "k_gemm", "fc_h_dx.kernel": "k_gemm<FcHDxProb>",
                "dfeat_finish.splits": 54, "fc_h_bwd": None, "act_path.covered": 0},
    # the fused norm's 16 384 sum-of-squares slots at batch 33
    "c-b33-h2176": {"caps.fast_fc": 1, "fc_h_fwd.kernel": "k_nl_fwd3<2>", "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_bwd.fuse_norm": 1,
                    "fc_h_bwd.norm_slots": 16227, "fc_h_bwd.implicit_sigma": 0, "fc_h_bwd.hsplits": 4},
    "c-b33-h2208": {"caps.fast_fc": 1, "fc_h_fwd.kernel": "k_nl_fwd3<2>", "fc_h_bwd.kernel": "k_nl_bwd<false>", "fc_h_bwd.fuse_norm": 0,
                    "fc_h_bwd.norm_slots": 0, "fc_h_bwd.implicit_sigma": 0, "fc_h_bwd.hsplits": 4},
    # the tiled forward GEMM beyond the tile count that lets it split K
    "d-b1024-h4096": {"caps.fast_fc": 1, "conv1_fwd.kernel": "k_conv_fwd_full<GeomD1>", "fc_h_fwd.kernel": "k_fc_gemm_fwd", "fc_h_fwd.tiles": 1536,
                      "fc_h_fwd.S": 1, "fc_h_bwd.kernel": "k_fc_gemm_bwd", "fc_h_bwd.fuse_norm": 1, "fc_h_bwd.hsplits": 4},
}


def test_every_row_of_the_history_and_hidden_table_is_pinned():
    import shape_range_scenarios as SR
    assert set(SHAPE_RANGE_PINS) == set(SR.CASES)


@pytest.mark.parametrize("case", sorted(SHAPE_RANGE_PINS))
def test_history_and_hidden_table_reaches_what_each_row_claims(emu, case):
    p = shape_range_plan(emu, case)
    for key, want in SHAPE_RANGE_PINS[case].items():
        tag, _, field = key.partition(".")
        if want is None:
            assert tag not in p, (case, tag, p[tag])
        else:
            assert tag in p and p[tag][field] == want, (case, key, p.get(tag), want)


@pytest.mark.parametrize("case", ["c-b33-h2176", "c-b33-h2208"])
def test_implicit_sigma_is_not_taken_at_batch_33(emu, case):
    """Neither the pipelined weight-gradient body (batch <= 32) nor the tiled GEMM (batch >= 128): the flag Agent sets changes
    nothing on either side of the fused norm's slot limit, and the noise snapshot behind the conv reduction is not taken."""
    p, q = shape_range_plan(emu, case), shape_range_plan(emu, case, flags=_lib.LEARNER_IMPLICIT_SIGMA)
    assert q["fc_h_bwd"]["implicit_sigma"] == 0 and q["reduce_conv_dw"]["snapshot"] == 0
    assert p == q


def test_act_path_rows_per_workgroup_follow_the_patch_limit(emu):
    """act_host.h act_conv_rows: at most 128 positions, and the rows' input patch within RB_ACT_LDS = 15 360 floats — canonical
    conv1 at history h stages h * ((rg - 1) * 4 + 8) * 84 floats."""
    want = {1: 6, 4: 6, 6: 6, 7: 5, 8: 4, 9: 4, 10: 3, 11: 3, 12: 2, 15: 2, 16: 1}
    for hist, rg in want.items():
        p = plan(emu, batch=4, history=hist, hidden=64)["act_path"]
        assert p["covered"] == 1 and p["rg"] == (rg, 9, 7), (hist, p)
        assert hist * ((rg - 1) * 4 + 8) * 84 <= 15360 and (rg == 6 or hist * (rg * 4 + 8) * 84 > 15360)
    assert plan(emu, opts="generic=2")["act_path"]["covered"] == 0
