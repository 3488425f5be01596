"""The optimiser pass in every form on the GPU against the float64 one-step reference of tests/optimizer_scenarios.py (the
scenarios of tests/test_optimizer_emu.py through librainbow_hip.so), plus the canonical hidden-512 network of BASELINE config 2:
other block and norm-partial counts, and the real pairing threshold instead of the test hook."""
import os

import pytest

import optimizer_scenarios as S
import scenarios

pytestmark = pytest.mark.gpu

CFG2 = "cfg2-canonical-h512-b32-a6"


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    yield _lib.load()
    out = os.environ.get("RB_OPTIMIZER_RATIOS")      # the observed error / bound table of profiles/optimizer_bounds.txt
    if out:
        with open(out, "a") as f:
            f.write(S.format_ratios("MI355X"))


@pytest.fixture
def Mem():
    from cabi_adapter import TorchMem
    return TorchMem


@pytest.fixture
def cfg2(monkeypatch):
    from test_learner_gpu import BASELINE_SHAPES
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, CFG2, BASELINE_SHAPES[CFG2])
    return CFG2


def test_clip_grad_against_f64_norm_and_one_product(hip, Mem):
    S.clip_grad_check(hip, Mem)


def test_plain_flush_and_hosted_forms_agree_with_the_reference_and_each_other(hip, Mem, monkeypatch):
    assert S.form_group_check(hip, Mem, monkeypatch) == set(S.STEPS)


def test_fifty_step_trajectory_every_step_checked_from_the_device_state(hip, Mem, monkeypatch):
    S.trajectory_check(hip, Mem, monkeypatch, steps=50)


def test_pair_pass_forms_the_sigma_gradient_from_the_noise_snapshot(hip, Mem, monkeypatch):
    S.pairs_check(hip, Mem, monkeypatch)


def test_fused_tile_pass_against_the_reference_and_the_oracle(hip, Mem):
    S.fused_tile_check(hip, Mem)


def test_hosted_pass_skips_the_update_of_a_failed_draw(hip, Mem):
    S.skipped_update_check(hip, Mem)


def test_canonical_clip_grad_with_the_partials_of_a_learn_call(hip, Mem, cfg2):
    """6.4 M parameters: 1024 k_sumsq blocks, and k_clip_scale capped at 256 blocks when a learn call left the partials."""
    S.clip_grad_check(hip, Mem, name=cfg2, cases=(("scales", "idle"), ("zeros", "bite")))


def test_canonical_clip_adam_idle_and_biting(hip, Mem, cfg2):
    S.single_form_check(hip, Mem, cfg2, "value", (("scales", "idle", 1), ("zeros", "bite", 2 ** 32 + 3)))


def test_canonical_pair_pass_at_the_real_pairing_threshold(hip, Mem, monkeypatch, cfg2):
    S.pairs_check(hip, Mem, monkeypatch, name=cfg2, opts=None)


def test_canonical_fused_tile_pass(hip, Mem, cfg2):
    S.fused_tile_check(hip, Mem, name=cfg2)
