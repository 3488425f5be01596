"""The per-row-noise act path (rb_learner_noise_rows, rb_learner_act_batch_rows) on the host interpreter, from the SAME kernel
sources as librainbow_hip.so: the streamed two-contraction kernels (k10, canon), the plain fallback (atoms21: H = 48), the
generator.  The device runs the same checks at more shapes, and the Python surface, in test_noise_rows_gpu.py."""
import os
import subprocess
import sys

import pytest

import noise_rows_scenarios as NR
from cabi_adapter import NumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


def _ctx(emu, name, n_max):
    c = NR.RowsContext(emu, NumpyMem(), name, n_max)
    yield c
    c.close()


@pytest.fixture(scope="module")
def k10(emu):
    yield from _ctx(emu, "k10", 33)


@pytest.fixture(scope="module")
def canon(emu):
    yield from _ctx(emu, "canon", 17)


@pytest.fixture(scope="module")
def atoms21(emu):
    yield from _ctx(emu, "atoms21", 3)


# both sides of the 16-row MFMA tile and of the 32-row chunk
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33])
def test_rows_parity_k10(k10, n):
    NR.check_parity(k10, n)


@pytest.mark.parametrize("n", [5, 17])
def test_rows_parity_canon(canon, n):
    NR.check_parity(canon, n)


def test_rows_parity_atoms21_fallback(atoms21):
    NR.check_parity(atoms21, 3)


@pytest.mark.parametrize("n", [1, 17])
def test_rows_consistent_with_the_shared_noise_path(k10, n):
    NR.check_consistency(k10, n)


def test_rows_consistent_with_the_shared_noise_path_fallback(atoms21):
    NR.check_consistency(atoms21, 3)


def test_rows_locality(k10):
    NR.check_locality(k10, 33, 16)


def test_rows_locality_fallback(atoms21):
    NR.check_locality(atoms21, 3, 1)


def test_noise_rows_generator(k10):
    NR.check_generator(k10)


@pytest.mark.parametrize("shape", ["k10", "canon", "atoms21"])
def test_noise_rows_injected_normals_are_make_noise(shape, request):
    NR.check_injected_normals(request.getfixturevalue(shape))


def test_rows_refusals(k10):
    NR.check_refusals(k10)


def test_rows_kernels_stay_inside_their_buffers():
    """The out-of-bounds write hunt (tests/noise_rows_guard_run.py) in a child process: RB_GUARD is read when the library
    first allocates."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "noise_rows_guard_run.py"), "emu"], env=dict(os.environ, RB_GUARD="1"),
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "guard run ok" in p.stdout, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
