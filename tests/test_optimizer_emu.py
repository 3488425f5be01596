"""The optimiser pass in every form on the host interpreter (CPU) against the float64 one-step reference of
tests/optimizer_scenarios.py: the same kernel sources as librainbow_hip.so; the same scenarios run on the GPU in
tests/test_optimizer_gpu.py."""
import os

import pytest

import optimizer_scenarios as S
from cabi_adapter import NumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    yield loader.load()
    out = os.environ.get("RB_OPTIMIZER_RATIOS")      # the observed error / bound table of profiles/optimizer_bounds.txt
    if out:
        with open(out, "a") as f:
            f.write(S.format_ratios("host interpreter"))


def test_clip_grad_against_f64_norm_and_one_product(emu):
    S.clip_grad_check(emu, NumpyMem)


def test_plain_flush_and_hosted_forms_agree_with_the_reference_and_each_other(emu, monkeypatch):
    """Step numbers 1, 2, 10, 1000, 10^6 and 2^32 + 3 (the device counter's high word), by value and from the counter; max_norm
    far from the norm, 1e-4 to either side of it, +inf with and without a norm buffer; zero ranges, 1e-8 .. 1e2 tensor scales,
    one dominant element, the all-zero gradient."""
    assert S.form_group_check(emu, NumpyMem, monkeypatch) == set(S.STEPS)


def test_fifty_step_trajectory_every_step_checked_from_the_device_state(emu, monkeypatch):
    S.trajectory_check(emu, NumpyMem, monkeypatch, steps=50)


def test_pair_pass_forms_the_sigma_gradient_from_the_noise_snapshot(emu, monkeypatch):
    S.pairs_check(emu, NumpyMem, monkeypatch)


def test_fused_tile_pass_against_the_reference_and_the_oracle(emu):
    S.fused_tile_check(emu, NumpyMem)


def test_hosted_pass_skips_the_update_of_a_failed_draw(emu):
    S.skipped_update_check(emu, NumpyMem)
