"""GPU tier (-m gpu): the pathwise posterior samples (gpmpc_paths_*, gpmpc_rollout_paths) on a real MI355X, at the emulator
tier's sizes (paths_cases.py: models A, B, C), plus N = 1024, S = 512, F = 256, Ny = 2 with "gemm_tile" 128: the setup's and
the grid evaluation's products through the large tiles."""
import pytest

import paths_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    yield lib
    pc.close_models()


def test_generator_path_equals_array_path_bitwise(lib):
    pc.check_generator_path_equals_array_path(lib, 96, 6, **pc.A)
    pc.check_generator_path_equals_array_path(lib, 300, 64, **pc.A)
    pc.check_generator_path_equals_array_path(lib, 601, 6, **pc.A)     # odd S, two setup panels, the second ragged


def test_zero_draw_is_the_predictive_mean(lib):
    pc.check_zero_draw(lib, 96, 6, **pc.A)
    pc.check_zero_draw(lib, 96, 64, mean_func='const', **pc.A)


def test_path_weights_against_longdouble(lib):
    pc.check_weights(lib, 96, 6, **pc.A)
    pc.check_weights(lib, 300, 64, **pc.A)
    pc.check_weights(lib, 601, 6, **pc.A)
    pc.check_weights(lib, 96, 64, **pc.B1)
    pc.check_weights(lib, 96, 64, **pc.B2)


def test_evaluation_against_longdouble(lib):
    pc.check_eval(lib, 96, 6, **pc.A)
    pc.check_eval(lib, 300, 64, **pc.A)
    pc.check_eval(lib, 96, 64, **pc.B1)
    pc.check_eval(lib, 96, 64, **pc.B2)
    pc.check_eval(lib, 96, 64, **pc.C1)
    pc.check_eval(lib, 96, 64, **pc.C16)


def test_grid_evaluation_against_longdouble(lib):
    pc.check_eval_grid(lib, 96, 64, **pc.A)


def test_weights_and_evaluation_through_the_large_tiles(lib):
    """N = 1024, S = 512, F = 256: check 3 over all (s, i), check 4 on the own inputs and on a grid."""
    lib.set_tuning('gemm_tile', 128)
    try:
        pc.check_weights(lib, 512, 256, **pc.BIG)
        pc.check_eval(lib, 512, 256, **pc.BIG)
        pc.check_eval_grid(lib, 512, 256, Bs=(65,), **pc.BIG)
    finally:
        lib.set_tuning('gemm_tile', 0)


def test_rollout_replay(lib):
    pc.check_rollout_replay(lib, 96, 64, **pc.A)


def test_distribution_is_that_of_consistent_paths(lib):
    """Seed pc.DIST_SEED = 2024, S = 4096, F = 64, 8 probes.  numpy replay with the same normals (the CPU tier's
    test_emu_numpy_replay_of_the_distribution_seed): worst ratio 2.27 standard errors (< 4); the first seed tried."""
    pc.check_distribution(lib, **pc.A)


def test_staleness_and_argument_errors(lib):
    pc.check_staleness_and_errors(lib, **pc.A)
