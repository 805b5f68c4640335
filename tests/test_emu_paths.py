"""CPU tier: the pathwise posterior samples (gpmpc_paths_*, gpmpc_rollout_paths, GP.sample_paths / paths_eval /
rollout_paths) on the emulated build of the unmodified HIP sources (tests/emu).  Models (paths_cases.py): A N = 130 (Np = 192,
two blocks of the evaluation kernel, the second with two points), d = 3, Ny = 2 with F = 6 (three frequencies: a ragged
feature block) and 64 (two feature blocks), S = 96 and 300 (two particle blocks, the second ragged); B N = 330 (three
training-point blocks, the last ragged), d = 4, sn = 0.1 and 1e-2; C d = 1 and 16.  The checks live in paths_cases.py; the GPU
tier runs the same ones."""
import os
import subprocess

import pytest

import paths_cases as pc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    lib = GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))
    yield lib
    pc.close_models()


def test_emu_generator_path_equals_array_path_bitwise(emu):
    pc.check_generator_path_equals_array_path(emu, 96, 6, **pc.A)
    pc.check_generator_path_equals_array_path(emu, 300, 64, **pc.A)
    pc.check_generator_path_equals_array_path(emu, 601, 6, **pc.A)     # odd S, two setup panels, the second ragged


def test_emu_zero_draw_is_the_predictive_mean(emu):
    pc.check_zero_draw(emu, 96, 6, **pc.A)
    pc.check_zero_draw(emu, 96, 64, mean_func='const', **pc.A)


def test_emu_path_weights_against_longdouble(emu):
    pc.check_weights(emu, 96, 6, **pc.A)
    pc.check_weights(emu, 300, 64, **pc.A)
    pc.check_weights(emu, 601, 6, **pc.A)
    pc.check_weights(emu, 96, 64, **pc.B1)
    pc.check_weights(emu, 96, 64, **pc.B2)


def test_emu_evaluation_against_longdouble(emu):
    pc.check_eval(emu, 96, 6, **pc.A)
    pc.check_eval(emu, 300, 64, **pc.A)
    pc.check_eval(emu, 96, 64, **pc.B1)
    pc.check_eval(emu, 96, 64, **pc.B2)
    pc.check_eval(emu, 96, 64, **pc.C1)
    pc.check_eval(emu, 96, 64, **pc.C16)


def test_emu_grid_evaluation_against_longdouble(emu):
    pc.check_eval_grid(emu, 96, 64, **pc.A)


def test_emu_rollout_replay(emu):
    pc.check_rollout_replay(emu, 96, 64, **pc.A)


def test_emu_distribution_is_that_of_consistent_paths(emu):
    """Seed pc.DIST_SEED = 2024, S = 4096, F = 64, 8 probes (two of them 0.05 apart).  The numpy replay with the same normals
    (pc.numpy_dist_ratios(**pc.A), the test below): worst ratio 2.27 standard errors (a covariance entry of output 1; the
    means within 1.77 / 2.24), below the 4 that fixes a seed; it was the first seed tried."""
    pc.check_distribution(emu, **pc.A)


def test_emu_numpy_replay_of_the_distribution_seed():
    """DIST_SEED = 2024, the first seed tried.  Per output (mean ratio, worst covariance ratio, correlation of the close
    probes): (1.77, 2.19, 0.9994) and (2.24, 2.27, 0.9993); worst ratio 2.27 < 4."""
    for rm, rc, rho in pc.numpy_dist_ratios(**pc.A):
        assert rm <= 4.0 and rc <= 4.0 and rho > 0.9, (rm, rc, rho)


def test_emu_staleness_and_argument_errors(emu):
    pc.check_staleness_and_errors(emu, **pc.A)


def test_emu_python_surface(emu, tank):
    pc.check_python_surface(emu, tank)
